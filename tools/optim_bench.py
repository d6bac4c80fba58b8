"""Timing of the optimizer step (fov3dgs_amd.optim.Adam, csrc/optim.hip) on the MI355X: one JSON line per candidate.

On the S-6M shapes (6 M Gaussians x 59 floats), in ONE process, the candidates alternating step by step, each step between
two device events on the current stream; --warmup rounds, then --steps timed rounds; median, min and max in ms:
  torch_adam        torch.optim.Adam(l, lr=0.0, eps=1e-15) as the reference constructs it (gaussian_model.py:289): the baseline
  torch_adam_fused  torch.optim.Adam(..., fused=True), if this torch build accepts it
  hip_dense         this optimizer on dense gradients
  hip_exact         this optimizer, sparse="exact", on the row-sparse gradients of a real pcheck_obb_sum backward (camera_ring(0))
  hip_exact_search  the same with the binary-search lookup instead of the 4 B / Gaussian inverse map (Adam.exact_lookup)
  hip_lazy          the same gradients, sparse="lazy"
Each line carries the algorithmic bytes computed from the shapes (16 B read + 12 B written per updated element; the sparse
modes add the compact gradient and 8 B per listed row and tensor) and the achieved fraction of 6.29 TB/s, the measured copy
rate of the chip. --train times eff_finetune.py's whole iteration WITH the optimizer (render -> fused L1 + SSIM -> backward
-> step, wall clock of back-to-back iterations and the optimizer's share from events) in four forms. Per-kernel times: run
this under `rocprofv3 --kernel-trace --stats` (e.g. with --steps 5) in a run of its own.

usage: python tools/optim_bench.py [--steps 50] [--warmup 10] [--train] [--out FILE] [--P 6000000]"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fov3dgs_amd  # noqa: E402,F401
from fov3dgs_amd import optim  # noqa: E402
from fov3dgs_amd import synthetic as syn  # noqa: E402
from fov3dgs_amd.gaussian_renderer import render  # noqa: E402
from fov3dgs_amd.loss_utils import l1_ssim_loss  # noqa: E402

COPY_RATE = 6.29e12  # B/s, the measured copy rate of the MI355X
ARGS = SimpleNamespace(position_lr_init=0.00016, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
W, H = 1920, 1080


class Pipe:
    debug = False


def clone_model(cloud):
    c = syn.GaussianCloud(*[p.detach().clone() for p in cloud.parameters()], sh_degree=cloud.active_sh_degree)
    return c.requires_grad_(True)


def backward_grads(cloud, cam, bg, target, row_sparse):
    cloud.fuse_activations, cloud.row_sparse_grads = True, row_sparse
    for p in cloud.parameters():
        p.grad = None
    l1_ssim_loss(render(cam, cloud, Pipe(), bg, cuda_type="pcheck_obb_sum")["render"], target, 0.2).backward()
    g = {n: getattr(cloud, n).grad for n in NAMES}
    for p in cloud.parameters():
        p.grad = None
    return g


def step_bench(a, dev):
    cloud = syn.scene_bicycle_scale(P=a.P).to(dev).requires_grad_(True)
    cam, bg, target = syn.camera_ring(0, width=W, height=H).to(dev), torch.zeros(3, device=dev), torch.rand(3, H, W, device=dev)
    dense = backward_grads(cloud, cam, bg, target, False)
    sparse = backward_grads(cloud, cam, bg, target, True)
    n_rows = int(sparse["_xyz"]._values().shape[0])
    elems = sum(getattr(cloud, n).numel() for n in NAMES)
    per_row = elems // a.P
    bytes_of = {"dense": 28 * elems, "exact": 24 * elems + n_rows * (4 * per_row + 8 * len(NAMES)),
                "lazy": n_rows * (28 * per_row + 8 * len(NAMES))}

    def candidate(kind, make, grads):
        m = clone_model(cloud)
        opt = make(optim.reference_param_groups(m, ARGS))
        for n in NAMES:
            getattr(m, n).grad = grads[n]
        return dict(name=kind, opt=opt, model=m, ms=[])
    cands = [(candidate("torch_adam", lambda l: torch.optim.Adam(l, lr=0.0, eps=1e-15), dense), "dense")]
    try:
        c = candidate("torch_adam_fused", lambda l: torch.optim.Adam(l, lr=0.0, eps=1e-15, fused=True), dense)
        c["opt"].step()
        cands.append((c, "dense"))
    except Exception as e:  # this torch build has no fused Adam for the device
        print(json.dumps({"case": "torch_adam_fused", "unavailable": str(e)[:200]}), flush=True)
    cands.append((candidate("hip_dense", lambda l: optim.Adam(l, lr=0.0, eps=1e-15), dense), "dense"))
    cands.append((candidate("hip_exact", lambda l: optim.Adam(l, lr=0.0, eps=1e-15, sparse="exact"), sparse), "exact"))
    c = candidate("hip_exact_search", lambda l: optim.Adam(l, lr=0.0, eps=1e-15, sparse="exact"), sparse)
    c["opt"].exact_lookup = "search"
    cands.append((c, "exact"))
    cands.append((candidate("hip_lazy", lambda l: optim.Adam(l, lr=0.0, eps=1e-15, sparse="lazy"), sparse), "lazy"))
    for it in range(a.warmup + a.steps):
        evs = []
        for c, _ in cands:  # the candidates alternate step by step
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c["opt"].step()
            e1.record()
            evs.append((c, e0, e1))
        torch.cuda.synchronize()
        if it >= a.warmup:
            for c, e0, e1 in evs:
                c["ms"].append(e0.elapsed_time(e1))
    lines = []
    for c, kind in cands:
        med = statistics.median(c["ms"])
        lines.append({"case": c["name"], "P": a.P, "elements": elems, "median_ms": round(med, 4), "min_ms": round(min(c["ms"]), 4),
                      "max_ms": round(max(c["ms"]), 4), "steps": a.steps, "algorithmic_bytes": bytes_of[kind],
                      "floor_ms_at_6.29TBps": round(bytes_of[kind] / COPY_RATE * 1e3, 4),
                      "fraction_of_copy_rate": round(bytes_of[kind] / (med * 1e-3) / COPY_RATE, 4),
                      "device": torch.cuda.get_device_name(0)})
    med = {l["case"]: l["median_ms"] for l in lines}
    lines.append({"rows_listed": n_rows, "sparse_grads_coalesced": bool(sparse["_xyz"].is_coalesced()), "algorithmic_lazy_over_dense": round(n_rows / a.P, 4),
                  "measured_lazy_over_dense": round(med["hip_lazy"] / med["hip_dense"], 4),
                  "hip_dense_over_torch_adam": round(med["hip_dense"] / med["torch_adam"], 4),
                  "hip_dense_over_torch_adam_fused": round(med["hip_dense"] / med["torch_adam_fused"], 4) if "torch_adam_fused" in med else None,
                  "hip_exact_over_hip_dense": round(med["hip_exact"] / med["hip_dense"], 4)})
    return lines


def train_bench(a, dev):
    """eff_finetune.py:107-147 with the optimizer: wall clock per iteration of n back-to-back iterations (the forward call's wait
    for its instance count is the only synchronisation) and the median of the events around optimizer.step()."""
    cam, bg, target = syn.camera_ring(0, width=W, height=H).to(dev), torch.zeros(3, device=dev), torch.rand(3, H, W, device=dev)
    base = syn.scene_bicycle_scale(P=a.P).to(dev)
    forms = (("refmodel_torch_adam", False, False, lambda l: torch.optim.Adam(l, lr=0.0, eps=1e-15)),
             ("refmodel_hip_dense", False, False, lambda l: optim.Adam(l, lr=0.0, eps=1e-15)),
             ("sparse_hip_exact", True, True, lambda l: optim.Adam(l, lr=0.0, eps=1e-15, sparse="exact")),
             ("sparse_hip_lazy", True, True, lambda l: optim.Adam(l, lr=0.0, eps=1e-15, sparse="lazy")))
    lines = []
    for name, raw, sparse, make in forms:
        m = clone_model(base)
        m.fuse_activations, m.row_sparse_grads = raw, sparse
        model = m if raw else syn.ReferenceShapedModel(m)  # the attributes and getters of the reference's GaussianModel
        opt = make(optim.reference_param_groups(m, ARGS))
        n, warm = a.steps, a.warmup
        evs, t0 = [], 0.0
        for it in range(warm + n):
            if it == warm:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            out = render(cam, model, Pipe(), bg, cuda_type="pcheck_obb_sum")
            l1_ssim_loss(out["render"], target, 0.2).backward()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt.step()
            e1.record()
            opt.zero_grad(set_to_none=True)
            evs.append((e0, e1))
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / n * 1e3
        lines.append({"train": name, "P": a.P, "iteration_ms": round(wall, 3),
                      "optimizer_ms": round(statistics.median(e0.elapsed_time(e1) for e0, e1 in evs[warm:]), 3), "iterations": n,
                      "device": torch.cuda.get_device_name(0)})
        del m, model, opt
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--P", type=int, default=6_000_000)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "optim_bench needs the MI355X"
    dev = "cuda:0"
    lines = train_bench(a, dev) if a.train else step_bench(a, dev)
    for l in lines:
        print(json.dumps(l), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
