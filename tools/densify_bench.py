"""Timing of densify_and_prune (fov3dgs_amd.densify, csrc/densify.hip) on the MI355X against the reference's torch sequence.

On the S-6M cloud with Adam state (6 M Gaussians x 59 floats, two moments each, plus `indexes`), in ONE process, the torch path
(tests/densify_ref.densify_and_prune: the literal four passes of gaussian_model.py:820-834 -- cat for the clones, cat for the
children, prune_points for the split parents, prune_points for the opacity / size cut) and the fused path alternating repetition
by repetition, each on a fresh copy of the model (copied outside the timed region) between two device events on the current
stream, so the host synchronisations of either path count as the device time they leave idle; --warmup rounds, then --reps timed
ones; median, min, max and spread (max - min) in ms. The thresholds are taken from the cloud's own quantiles so that roughly 5 %
of the rows are cloned, 5 % split and 2 % die. The line also carries the algorithmic bytes -- the state read once plus the new
state written once -- and the achieved bytes/s of both paths. The fused path "wins" when the torch median exceeds the fused
median by more than the larger of the two spreads of this run.

usage: python tools/densify_bench.py [--reps 20] [--warmup 5] [--P 6000000] [--N 2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fov3dgs_amd  # noqa: E402,F401
from fov3dgs_amd import densify, optim  # noqa: E402
from fov3dgs_amd import synthetic as syn  # noqa: E402
from tests import densify_ref, prune_ref  # noqa: E402
from tests.adam_ref import ATTRS, NAMES  # noqa: E402

PEAK_BYTES_PER_S = 8e12  # MI355X HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--P", type=int, default=6_000_000)
    ap.add_argument("--N", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "densify_bench needs the MI355X"
    dev = "cuda:0"
    P, N = a.P, a.N
    base = prune_ref.Model(syn.scene_bicycle_scale(P=P), optim.Adam, device=dev)
    base.percent_dense = 0.01
    g = torch.Generator(device=dev).manual_seed(0)
    for n in NAMES:  # one step: every group has its moments
        p = getattr(base, ATTRS[n])
        p.grad = 1e-3 * torch.randn(p.shape, generator=g, device=dev)
    base.optimizer.step()
    base.optimizer.zero_grad(set_to_none=True)
    base.xyz_gradient_accum = torch.rand(P, 1, generator=g, device=dev)
    base.denom = torch.ones(P, 1, device=dev)
    smax = torch.exp(base._scaling.detach()).max(dim=1).values
    max_grad = 0.9                                                                            # 10 % of the rows are hot ...
    extent = float(smax[::max(P // 1_000_000, 1)].median()) / base.percent_dense             # ... half of them small, half large
    min_opacity = float(torch.sigmoid(base._opacity.detach())[::max(P // 1_000_000, 1)].flatten().quantile(0.02))
    max_screen_size = 20
    # (as in the GPU tests: no scale or opacity within 1e-4 of a threshold, so both paths take the same decisions)
    assert densify_ref.open_gaps(base, (base.percent_dense * extent, 0.1 * extent), min_opacity, Ns=(N,)) == 0
    keep, clone, split, child = densify_ref.plan_classes(base, max_grad, min_opacity, extent, max_screen_size, N)
    n_keep, n_clone, n_split, n_child = (int(x.sum()) for x in (keep, clone, split, child))
    n_new = n_keep + n_clone + N * n_child
    noise = torch.randn(N * n_split, 3, generator=g, device=dev)
    row_bytes = sum(t.element_size() * (t.numel() // P) for k, t in prune_ref.state_tensors(base).items()
                    if t.dim() and t.shape[0] == P and k not in ("xyz_gradient_accum", "denom", "max_radii2D"))
    algorithmic = (P + n_new) * row_bytes

    def fused(m):
        return densify.densify_and_prune(m, max_grad, min_opacity, extent, max_screen_size, N=N, noise=noise)

    def reference(m):
        return densify_ref.densify_and_prune(m, max_grad, min_opacity, extent, max_screen_size, N, noise)
    # the two paths agree (layout and copies; the children's arithmetic is the GPU tests' business)
    x, y = prune_ref.clone_model(base), prune_ref.clone_model(base)
    assert tuple(fused(x)) == (n_keep, n_clone, n_split, n_child)
    reference(y)
    assert len(x) == len(y) == n_new
    for k, t in prune_ref.state_tensors(x).items():
        if k not in ("xyz", "scaling"):
            assert prune_ref.same_bits(t, prune_ref.state_tensors(y)[k]), k
    del x, y
    ms = {"torch": [], "fused": []}
    for it in range(a.warmup + a.reps):
        for which, fn in (("torch", reference), ("fused", fused)):
            m = prune_ref.clone_model(base)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(m)
            e1.record()
            torch.cuda.synchronize()
            del m
            if it >= a.warmup:
                ms[which].append(e0.elapsed_time(e1))
    line = {"stage": "densify_and_prune", "P": P, "N": N, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
            "kept": n_keep, "cloned": n_clone, "split": n_split, "children_per_copy": n_child, "rows_after": n_new,
            "cloned_fraction": round(n_clone / P, 4), "split_fraction": round(n_split / P, 4),
            "died_fraction": round((P - n_split - n_keep) / P, 4), "row_bytes": row_bytes, "algorithmic_bytes": algorithmic}
    for which in ("torch", "fused"):
        v = ms[which]
        line.update({f"{which}_median_ms": round(statistics.median(v), 4), f"{which}_min_ms": round(min(v), 4),
                     f"{which}_max_ms": round(max(v), 4), f"{which}_spread_ms": round(max(v) - min(v), 4),
                     f"{which}_bytes_per_s": round(algorithmic / (statistics.median(v) * 1e-3), 0),
                     f"{which}_fraction_of_peak": round(algorithmic / (statistics.median(v) * 1e-3) / PEAK_BYTES_PER_S, 4)})
    line["torch_over_fused"] = round(line["torch_median_ms"] / line["fused_median_ms"], 2)
    line["fused_wins_beyond_spread"] = bool(line["torch_median_ms"] - line["fused_median_ms"] > max(line["torch_spread_ms"], line["fused_spread_ms"]))
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
