"""Timing of the pruning step (fov3dgs_amd.pruning, csrc/prune.hip) on the MI355X against the reference's torch operations.

On the S-6M cloud with Adam state (6 M Gaussians x 59 floats, two moments each), in ONE process, the torch path and the fused
path alternating repetition by repetition, each between two device events on the current stream; --warmup rounds, then --reps
timed ones; median, min, max and spread (max - min) in ms, per stage:
  metric   three views' updates of the metric: prune.py:82-86 literally (ten elementwise passes per view) / update_metric_;
           the per-view statistics are those of three real pcheck_obb_loss_weighted_max_count renders (camera_ring 0..2, 1080p)
  select   the mask of the lowest 2 %: prune.py:101-107 literally (torch.sort, slice, zeros, scatter, bool) / lowest_k_mask
  gather   the cut of the full tensor set of gaussian_model.py:624-664 (six parameters, two moments each, three side arrays,
           indexes: 22 tensors): ~mask and 22 tensor[mask] calls / compact_rows with the count given (one plan, one launch)
A stage "wins" when the torch median exceeds the fused median by more than the larger of the two spreads of this run. The
gather line also carries its algorithmic bytes (the mask, plus the kept rows read and written) and the achieved bytes/s.

usage: python tools/prune_bench.py [--reps 20] [--warmup 3] [--P 6000000] [--ratio 0.02] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fov3dgs_amd  # noqa: E402,F401
from fov3dgs_amd import pruning  # noqa: E402
from fov3dgs_amd import synthetic as syn  # noqa: E402
from fov3dgs_amd.gaussian_renderer import render  # noqa: E402

W, H = 1920, 1080


class Pipe:
    debug = False


def torch_metric(metrics, views):
    """The torch operations of prune.py:82-86, one for one and in their order, on [P,1] columns: two casts, an add, a divide,
    a compare with a masked fill, then the compare done twice, once for a boolean gather and once for the masked store."""
    for contribs, counts in views:
        value, tests = contribs.unsqueeze(1).float(), counts.unsqueeze(1).float()
        cur = value / (tests + 1e-7)
        cur[tests < 1] = 0
        raised = cur[metrics < cur]
        metrics[metrics < cur] = raised
    return metrics


def torch_select(metrics, k):
    """The torch operations of prune.py:101-107 on the [P,1] metrics: the default (unstable) ascending sort along the rows, its
    first k indices, a float [P,1] of zeros with ones stored at them, the cast to bool."""
    lowest = metrics.sort(dim=0).indices[:k]
    flags = torch.zeros((metrics.shape[0], 1), device=metrics.device)
    flags[lowest] = 1
    return flags.bool().squeeze()


def torch_gather(mask, tensors):
    """gaussian_model.py:624-664 as torch operations: the mask's complement, then one boolean gather per tensor."""
    valid = ~mask
    return [t[valid] for t in tensors]


def timed(pairs, reps, warmup):
    """pairs: {name: (torch_fn, fused_fn)} -> {name: {"torch": [ms], "fused": [ms]}}, alternating inside every repetition."""
    ms = {n: {"torch": [], "fused": []} for n in pairs}
    for it in range(warmup + reps):
        for n, fns in pairs.items():
            for which, fn in zip(("torch", "fused"), fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                torch.cuda.synchronize()
                del out
                if it >= warmup:
                    ms[n][which].append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--P", type=int, default=6_000_000)
    ap.add_argument("--ratio", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "prune_bench needs the MI355X"
    dev = "cuda:0"
    P, k = a.P, int(a.P * a.ratio)
    cloud = syn.scene_bicycle_scale(P=P).to(dev)
    bg, ones = torch.zeros(3, device=dev), torch.ones(3, H, W, device=dev)
    views = []
    with torch.no_grad():
        for i in range(3):
            pkg = render(syn.camera_ring(i, width=W, height=H).to(dev), cloud, Pipe(), bg,
                         cuda_type="pcheck_obb_loss_weighted_max_count", loss_map=ones)
            views.append((pkg["contribs"].clone(), pkg["gs_count"].clone()))
    metrics = pruning.update_metric_(torch.zeros(P, device=dev), *views[0])
    for v in views[1:]:
        pruning.update_metric_(metrics, *v)
    assert torch.equal(metrics, torch_metric(torch.zeros((P, 1), device=dev), views).squeeze(1))
    mask = pruning.lowest_k_mask(metrics, k)
    assert int(mask.sum()) == k
    g = torch.Generator(device=dev).manual_seed(0)
    params = [cloud._xyz, cloud._features_dc, cloud._features_rest, cloud._opacity, cloud._scaling, cloud._rotation]
    tensors = []
    for p in params:
        tensors += [p, torch.randn(p.shape, generator=g, device=dev), torch.rand(p.shape, generator=g, device=dev)]
    tensors += [torch.rand(P, 1, device=dev), torch.rand(P, 1, device=dev), torch.rand(P, device=dev), torch.arange(P, device=dev)]
    for x, y in zip(torch_gather(mask, tensors), pruning.compact_rows(mask, tensors, n_keep=P - k, invert=True)):
        assert torch.equal(x, y)
    row_bytes = sum(t.element_size() * (t.numel() // P) for t in tensors)
    gather_bytes = P + 2 * (P - k) * row_bytes

    def fused_metric():
        m = torch.zeros(P, device=dev)
        for v in views:
            pruning.update_metric_(m, *v)
        return m
    pairs = {
        "metric": (lambda: torch_metric(torch.zeros((P, 1), device=dev), views), fused_metric),
        "select": (lambda: torch_select(metrics.unsqueeze(1), k), lambda: pruning.lowest_k_mask(metrics, k)),
        "gather": (lambda: torch_gather(mask, tensors), lambda: pruning.compact_rows(mask, tensors, n_keep=P - k, invert=True)),
    }
    ms = timed(pairs, a.reps, a.warmup)
    lines = []
    for n, d in ms.items():
        line = {"stage": n, "P": P, "k": k, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
        for which in ("torch", "fused"):
            v = d[which]
            line.update({f"{which}_median_ms": round(statistics.median(v), 4), f"{which}_min_ms": round(min(v), 4),
                         f"{which}_max_ms": round(max(v), 4), f"{which}_spread_ms": round(max(v) - min(v), 4)})
        line["torch_over_fused"] = round(line["torch_median_ms"] / line["fused_median_ms"], 2)
        line["fused_wins_beyond_spread"] = bool(line["torch_median_ms"] - line["fused_median_ms"] > max(line["torch_spread_ms"], line["fused_spread_ms"]))
        if n == "metric":
            line["zero_metrics"] = int((metrics == 0).sum())
        if n == "gather":
            line.update({"tensors": len(tensors), "row_bytes": row_bytes, "algorithmic_bytes": gather_bytes,
                         "fused_bytes_per_s": round(gather_bytes / (line["fused_median_ms"] * 1e-3), 0),
                         "torch_bytes_per_s": round(gather_bytes / (line["torch_median_ms"] * 1e-3), 0)})
        lines.append(line)
    for l in lines:
        print(json.dumps(l), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
