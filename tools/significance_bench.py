"""LightGaussian's global-significance pruning (fov3dgs_amd.lightgaussian; csrc/render.hip FR_VARIANT_COUNT, csrc/prune.hip
fr_select_kth, csrc/significance.hip) on S-6M at 1080p on the MI355X, in ONE process, the candidates alternating round by round;
--warmup rounds, then the timed rounds; median, p10-p90, min and max in ms:
  (1) render         one frame of camera_ring(0): the plain `original` render, the `pcheck_obb_max` render (the other per-pixel
                     count of the project), and the counting render -- with --lanes-lib also the counting render of a second build
                     of the library (tools/scratch/count_lanes.patch applied and built with EXTRA=-DFR_COUNT_LANES=1: lane j of a
                     wave keeps the count of entry j of the batch and the wave adds the batch's counts with one vector atomic
                     instruction; the library's own form is one atomic of lane 0 per (wave, entry) with a non-zero count). Device
                     events around the call.
                     lanes_faster_beyond_spread: the lane form's p90 lies below the per-entry form's p10.
  (2) prune_list     count_render over --views cameras and torch's += of their outputs. Host time between synchronisations.
  (3) cut            score + threshold + mask + cut at percent 0.66 of a 6 M-row model with Adam state, fed by (2)'s sums.
                     fused: calculate_v_imp_score(v_pow 0.1) + prune_gaussians. torch_form: LightGaussian/prune.py:120-127 and
                     scene/gaussian_model.py:776-782 -- two full torch.sorts, pow, a comparison -- and the 21 boolean gathers of
                     prune_points. Host time between synchronisations (the cut ends with a readback in both forms).
No GPU, no run: there is no fallback.

usage: python tools/significance_bench.py [--rounds 20] [--slow-rounds 5] [--warmup 2] [--P 6000000] [--views 8]
                                          [--lanes-lib PATH] [--out profiles/significance_bench.json]"""
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
from fov3dgs_amd import _native, lightgaussian, optim  # noqa: E402
from fov3dgs_amd import synthetic as syn  # noqa: E402
from fov3dgs_amd.rasterizer import GaussianRasterizationSettings, _forward_begin  # noqa: E402

ARGS = SimpleNamespace(position_lr_init=0.00016, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
W, H = 1920, 1080
PERCENT, V_POW = 0.66, 0.1


class Pipe:
    debug = False


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "p10_ms": round(sorted(ms)[len(ms) // 10], 4), "p90_ms": round(sorted(ms)[(9 * len(ms)) // 10], 4), "n": len(ms)}


def beyond_spread(fast, slow):
    return bool(fast["p90_ms"] < slow["p10_ms"])


def second_library(path):
    """another build of the library beside the package's own (same ABI check), for A / B rounds under one Python"""
    own = _native.load()
    _native._lib, keep = None, _native.LIB_PATH
    try:
        _native.LIB_PATH = path
        other = _native.load()
    finally:
        _native.LIB_PATH, _native._lib = keep, own
    return own, other


def renders(base, dev, a):
    import math
    cam, bg = syn.camera_ring(0, width=W, height=H).to(dev), torch.zeros(3, device=dev)
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), bg, 1.0, cam.world_view_transform,
                                       cam.full_proj_transform, base.active_sh_degree, cam.camera_center, False, False)
    with torch.no_grad():
        s, q, o = base.get_activated
        dc, rest = base.get_features_split
    own = _native.load()
    libs = {"own": own}
    if a.lanes_lib:
        libs["own"], libs["lanes"] = second_library(a.lanes_lib)

    def call(variant, count, lib):
        _native._lib = libs[lib]
        try:
            return _forward_begin(variant, rs, base.get_xyz, dc, None, o, s, q, None, persistent=True, sh_rest=rest, count=count).finish()
        finally:
            _native._lib = own
    cands = [("original", (_native.VARIANT_ORIGINAL, False, "own")), ("pcheck_obb_max", (_native.VARIANT_PCHECK_OBB_MAX, False, "own")),
             ("count_per_entry_atomic", (_native.VARIANT_ORIGINAL, True, "own"))]
    if a.lanes_lib:
        cands.append(("count_lane_registers", (_native.VARIANT_ORIGINAL, True, "lanes")))
    ms, counts = {k: [] for k, _ in cands}, {}
    with torch.no_grad():
        for it in range(a.warmup + a.rounds):
            evs = []
            for k, args in cands:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res = call(*args)
                e1.record()
                evs.append((k, e0, e1))
                if args[1]:
                    counts[k] = res[6].clone()
            torch.cuda.synchronize()
            if it >= a.warmup:
                for k, e0, e1 in evs:
                    ms[k].append(e0.elapsed_time(e1))
    r = {k: summary(v) for k, v in ms.items()}
    r["hits"] = {k: int(v.long().sum()) for k, v in counts.items()}
    r["rows_hit"] = {k: int((v > 0).sum()) for k, v in counts.items()}
    if a.lanes_lib:
        r["same_counts"] = bool(torch.equal(counts["count_per_entry_atomic"], counts["count_lane_registers"]))
        r["lanes_faster_beyond_spread"] = beyond_spread(r["count_lane_registers"], r["count_per_entry_atomic"])
    return r


def prune_list(base, dev, a):
    bg = torch.zeros(3, device=dev)
    cams = [syn.camera_ring(i, n=a.views, width=W, height=H).to(dev) for i in range(a.views)]
    ms = []
    for it in range(a.warmup + a.slow_rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = lightgaussian.prune_list(base, cams, Pipe(), bg)
        torch.cuda.synchronize()
        if it >= a.warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    r = summary(ms)
    r["views"] = a.views
    r["rows_hit"] = int((out[0] > 0).sum())
    return r, out


def model_of(base):
    m = syn.GaussianCloud(*[p.detach().clone() for p in base.parameters()], sh_degree=base.active_sh_degree).requires_grad_(True)
    m.optimizer = optim.Adam(optim.reference_param_groups(m, ARGS), lr=0.0, eps=1e-15)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    m.optimizer.step()   # (every group has its two moments)
    m.optimizer.zero_grad(set_to_none=True)
    P, dev = len(m), m._xyz.device
    m.xyz_gradient_accum, m.denom, m.max_radii2D = torch.zeros(P, 1, device=dev), torch.zeros(P, 1, device=dev), torch.zeros(P, device=dev)
    return m


_ATTRS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}


def torch_cut(m, imp_list):
    """prune.py:120-127, gaussian_model.py:776-782 and prune_points (:642-664 of the Fov-3DGS model: the same surgery)"""
    volume = torch.prod(m.get_scaling, dim=1)
    index = int(len(volume) * 0.9)
    sorted_volume, _ = torch.sort(volume, descending=True)
    v_list = torch.pow(volume / sorted_volume[index], V_POW) * imp_list
    sorted_tensor, _ = torch.sort(v_list, dim=0)
    prune_mask = (v_list <= sorted_tensor[int(PERCENT * (sorted_tensor.shape[0] - 1))]).squeeze()
    keep = ~prune_mask
    opt = m.optimizer
    for group in opt.param_groups:
        old = group["params"][0]
        st = opt.state.get(old, None)
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][keep], st["exp_avg_sq"][keep]
            del opt.state[old]
        group["params"][0] = torch.nn.Parameter(old.detach()[keep].requires_grad_(True))
        if st is not None:
            opt.state[group["params"][0]] = st
        setattr(m, _ATTRS[group["name"]], group["params"][0])
    m.xyz_gradient_accum, m.denom, m.max_radii2D = m.xyz_gradient_accum[keep], m.denom[keep], m.max_radii2D[keep]


def fused_cut(m, imp_list):
    lightgaussian.prune_gaussians(m, PERCENT, lightgaussian.calculate_v_imp_score(m, imp_list, V_POW))


def cut(base, dev, a, imp_list):
    forms = (("fused", fused_cut), ("torch_form", torch_cut))
    ms, kept = {k: [] for k, _ in forms}, {}
    with torch.no_grad():
        for it in range(a.warmup + a.slow_rounds):
            for k, fn in forms:
                m = model_of(base)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(m, imp_list)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    ms[k].append(1e3 * (time.perf_counter() - t0))
                kept[k] = len(m)
                del m
    r = {k: summary(v) for k, v in ms.items()}
    r["rows"], r["rows_kept"] = len(base), kept
    r["fused_faster_beyond_spread"] = beyond_spread(r["fused"], r["torch_form"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--slow-rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--P", type=int, default=6_000_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--lanes-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "significance_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "significance_bench needs the MI355X"
    dev = "cuda:0"
    base = syn.scene_bicycle_scale(P=a.P).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "scene": "S-6M" if a.P == 6_000_000 else f"scene_bicycle_scale(P={a.P})",
              "size": [H, W], "rounds": a.rounds, "slow_rounds": a.slow_rounds, "warmup": a.warmup,
              "protocol": "one process, the candidates alternate round by round; render: device events around one call; "
                          "prune_list and cut: host time between device synchronisations"}
    result["render"] = renders(base, dev, a)
    print(json.dumps({"render": result["render"]}), flush=True)
    result["prune_list"], sums = prune_list(base, dev, a)
    print(json.dumps({"prune_list": result["prune_list"]}), flush=True)
    torch.cuda.empty_cache()
    result["cut"] = cut(base, dev, a, sums[1])
    print(json.dumps({"cut": result["cut"]}), flush=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
