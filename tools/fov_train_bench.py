"""The joint fine-tune step through the foveated renderer (render(..., appearance_only=True) -> foveated metameric loss -> backward ->
Adam on the per-level opacities and DC colours), on the MI355X, beside the only thing there is to compare it with: the mask-learning
step on a uniform render (gaussian_renderer.render(masking=True, appearance_only=True), pcheck_obb_sum).

S-6M at 1080p, ring view 0, gazes (0.5, 0.5) and (0.25, 0.75); everything in ONE process, the candidates alternating round by round,
each call between two device events; --warmup rounds, then --steps timed rounds; median, min, max, p10 and p90 in ms:
  inference_frame      render() under no_grad on the caller's stream alone (serial_frames: no overlap with a neighbour)
  keep_forward         the state-keeping forward by direct call (fr_forward_begin_fov_keep + finish)
  backward             fr_backward_fov_appearance over that state, with its two stages from stage_events: tile_pass, per_gaussian
  fov_step             forward, MetamericLoss with HVSLoss's defaults at the frame's gaze, backward, optim.Adam on the two tensors
  mask_step            the pcheck_obb_sum masking step with appearance_only=True and the same loss, in the same rounds
--full adds, in the same rounds, the FULL backward pass (render(..., differentiable=True), fr_backward_fov) and writes
profiles/fov_full_backward_bench.json:
  full_forward         the _full state-keeping forward by direct call (fr_forward_begin_fov_keep_full + finish)
  full_backward        fr_backward_fov over that state, with its two stages: tile_pass (k_render_bwd_fov_full), per_gaussian (k_fov_full_bwd)
  full_step            forward, the same loss, backward, optim.Adam on positions, scales, rotations, rest SH, per-level opacities and DCs
  sum_backward         pcheck_obb_sum's fr_backward on the same cloud (k_render_bwd + k_preprocess_bwd), through autograd, with its stages
next to the appearance backward of the same frames (`backward`); and `tile_pass_valu_per_pair`, VALU instructions per (band, entry)
pair of the new tile pass counted in the kernel's inner loop (k_render_bwd: 96), when given with --valu.
No target is fixed: the numbers are reported, and `beyond_spread` says which differences exceed the spread (one series' p10 above the
other's p90). No GPU, no run: there is no fallback.

usage: python tools/fov_train_bench.py [--steps 50] [--warmup 10] [--P 6000000] [--full] [--valu N] [--out profiles/fov_appearance_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fov3dgs_amd  # noqa: E402,F401
from fov3dgs_amd import _native, optim, profiling  # noqa: E402
from fov3dgs_amd import synthetic as syn  # noqa: E402
from fov3dgs_amd.gaussian_renderer import render as render_plain  # noqa: E402
from fov3dgs_amd.gaussian_renderer_fov import render as render_fov  # noqa: E402
from fov3dgs_amd.hvs_loss_calc import HVSLoss  # noqa: E402
from fov3dgs_amd.rasterizer import (GaussianRasterizationSettings, _backward_fov_full_native, _backward_fov_native, _forward_begin,  # noqa: E402
                                    serial_frames)
from tests import hvs_ref  # noqa: E402

W, H = 1920, 1080
GAZES = ((0.5, 0.5), (0.25, 0.75))
ALPHA = 0.05


class Pipe:
    debug = False


def summary(ms):
    s = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4),
            "p10_ms": round(s[len(s) // 10], 4), "p90_ms": round(s[(9 * len(s)) // 10], 4), "n": len(s)}


def beyond_spread(a, b):
    """-> "a<b", "a>b" or None: the two series differ by more than their spread"""
    if a["p90_ms"] < b["p10_ms"]:
        return "a<b"
    if a["p10_ms"] > b["p90_ms"]:
        return "a>b"
    return None


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    return out, e0, e1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--P", type=int, default=6_000_000)
    ap.add_argument("--full", action="store_true", help="also measure the full backward pass (fr_backward_fov)")
    ap.add_argument("--valu", type=int, default=None, help="VALU instructions per (band, entry) pair of k_render_bwd_fov_full, to record")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "fov_full_backward_bench.json" if a.full else "fov_appearance_bench.json")
    assert torch.cuda.is_available(), "fov_train_bench needs the MI355X"
    dev = "cuda:0"
    import math
    cam, bg = syn.camera_ring(0, 8, W, H).to(dev), torch.zeros(3, device=dev)
    cpu = syn.scene_bicycle_scale(P=a.P, seed=1, opacity_logit=syn.OPACITY_LOGIT_S6M)
    highest, dcs0, opac0 = [t.to(dev) for t in syn.foveation_layers(cpu, seed=2)]
    cloud = cpu.to(dev)
    filt = hvs_ref.filters_from_npz(np.load(os.path.join(ROOT, "tests", "golden", "ref_hvs.npz")), 6)
    hvs = HVSLoss(device=dev, filters=filt)
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0,
        viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=3, campos=cam.camera_center, prefiltered=False,
        debug=False)
    e = torch.Tensor([])
    xyz, scales, rots, rest = cloud.get_xyz.detach(), cloud.get_scaling.detach(), cloud.get_rotation.detach(), cloud.get_rest_features.detach()
    result = {"device": torch.cuda.get_device_name(0), "cloud": "S-6M", "P": a.P, "size": [W, H], "alpha": ALPHA, "view": "camera_ring(0)",
              "steps": a.steps, "warmup": a.warmup, "gazes": {}}
    if a.full:
        result["tile_pass_valu_per_pair"] = {"k_render_bwd_fov_full": a.valu, "k_render_bwd": 96}
    rounds = a.warmup + a.steps
    for gaze in GAZES:
        with torch.no_grad():
            target = render_fov(cam, cloud, bg, alpha=ALPHA, gazeArray=gaze, blending=True, highest_levels=highest, shs_dcs=dcs0,
                                opacities=(opac0 * 0.8).contiguous())["render"].clone()
        # the fine-tuned tensors of the foveated step, and the masking step's model, each with its own Adam
        opac, dcs = opac0.clone().requires_grad_(True), dcs0.clone().requires_grad_(True)
        opt_f = optim.Adam([{"params": [opac], "lr": 0.01}, {"params": [dcs], "lr": 0.0025}], lr=0.0, eps=1e-15)
        m = syn.GaussianCloud(*[p.detach().clone() for p in cloud.parameters()], sh_degree=cloud.active_sh_degree).requires_grad_(True)
        model = syn.ReferenceShapedModel(m)
        opt_m = optim.Adam([{"params": [m._opacity], "lr": 0.05}, {"params": [m._features_dc], "lr": 0.0025}], lr=0.0, eps=1e-15)
        series = {k: [] for k in ("inference_frame", "keep_forward", "backward", "fov_step", "mask_step")
                  + (("full_forward", "full_backward", "full_step", "sum_backward") if a.full else ())}
        if a.full:
            # the full step's model (every parameter a leaf, its own Adam) and the pcheck_obb_sum model of the baseline backward
            mf = syn.GaussianCloud(*[p.detach().clone() for p in cloud.parameters()], sh_degree=cloud.active_sh_degree).requires_grad_(True)
            opac_f, dcs_f = opac0.clone().requires_grad_(True), dcs0.clone().requires_grad_(True)
            opt_full = optim.Adam([{"params": [mf._xyz], "lr": 1.6e-6}, {"params": [mf._scaling], "lr": 0.005}, {"params": [mf._rotation], "lr": 0.001},
                                   {"params": [mf._features_rest], "lr": 0.000125}, {"params": [opac_f], "lr": 0.01}, {"params": [dcs_f], "lr": 0.0025}],
                                  lr=0.0, eps=1e-15)
            ms = syn.GaussianCloud(*[p.detach().clone() for p in cloud.parameters()], sh_degree=cloud.active_sh_degree).requires_grad_(True)
            full_calls, sum_calls = [], []
        lib = _native.load()
        dpix = torch.randn(3, H, W, device=dev) * 1e-3
        info = {}
        with profiling.BackwardTimer((6 if a.full else 3) * rounds) as bt:
            direct_calls = []
            for it in range(rounds):
                evs = {}
                with torch.no_grad(), serial_frames():
                    _, *evs["inference_frame"] = timed(lambda: render_fov(cam, cloud, bg, alpha=ALPHA, gazeArray=gaze, blending=True,
                                                                          highest_levels=highest, shs_dcs=dcs0, opacities=opac0))
                state = _native.FovState()
                state.size = C.sizeof(_native.FovState)
                res, *evs["keep_forward"] = timed(lambda: _forward_begin(_native.VARIANT_FOV_PCHECK_OBB, rs, xyz, rest, e, opac0, scales, rots, e,
                                                                         dcs0, highest, gaze, ALPHA, persistent=False, keep_state=state).finish())
                direct_calls.append(bt.used)
                g, *evs["backward"] = timed(lambda: _backward_fov_native(state, bg, dpix, stage_events=bt._next()))
                info = {"D": int(state.num_rendered), "work_items": int(state.num_items)}
                del g, res

                def fov_step():
                    out = render_fov(cam, cloud, bg, alpha=ALPHA, gazeArray=gaze, blending=True, highest_levels=highest, shs_dcs=dcs,
                                     opacities=opac, appearance_only=True)
                    hvs.calc_fov_loss(out["render"], target, gaze=list(gaze)).backward()
                    opt_f.step()
                    opt_f.zero_grad(set_to_none=True)
                _, *evs["fov_step"] = timed(fov_step)

                def mask_step():
                    out = render_plain(cam, model, Pipe(), bg, masking=True, cuda_type="pcheck_obb_sum", appearance_only=True)
                    hvs.calc_fov_loss(out["render"], target, gaze=list(gaze)).backward()
                    opt_m.step()
                    opt_m.zero_grad(set_to_none=True)
                _, *evs["mask_step"] = timed(mask_step)
                if a.full:
                    fstate = _native.FovState()
                    fstate.size = C.sizeof(_native.FovState)
                    res, *evs["full_forward"] = timed(lambda: _forward_begin(_native.VARIANT_FOV_PCHECK_OBB, rs, xyz, rest, e, opac0, scales, rots, e,
                                                                             dcs0, highest, gaze, ALPHA, persistent=False, keep_state=fstate,
                                                                             keep_full=True).finish())
                    full_calls.append(bt.used)
                    g, *evs["full_backward"] = timed(lambda: _backward_fov_full_native(fstate, rs, xyz, scales, rots, rest, dpix, stage_events=bt._next()))
                    del g, res

                    def full_step():
                        out = render_fov(cam, mf, bg, alpha=ALPHA, gazeArray=gaze, blending=True, highest_levels=highest, shs_dcs=dcs_f,
                                         opacities=opac_f, differentiable=True)
                        hvs.calc_fov_loss(out["render"], target, gaze=list(gaze)).backward()
                        opt_full.step()
                        opt_full.zero_grad(set_to_none=True)
                    _, *evs["full_step"] = timed(full_step)
                    out = render_plain(cam, ms, Pipe(), bg, cuda_type="pcheck_obb_sum")
                    loss = (out["render"] * dpix).sum()
                    sum_calls.append(bt.used)
                    _, *evs["sum_backward"] = timed(loss.backward)
                    for p_ in ms.parameters():
                        p_.grad = None
                    del out, loss
                torch.cuda.synchronize()
                if it >= a.warmup:
                    for k, (e0, e1) in evs.items():
                        series[k].append(e0.elapsed_time(e1))
            stages = bt.stage_ms()
        bt.close()
        r = {k: summary(v) for k, v in series.items()}
        mine = [stages[i] for it, i in enumerate(direct_calls) if it >= a.warmup]
        r["backward_stages"] = {"tile_pass": summary([d["render_bwd"] for d in mine]), "per_gaussian": summary([d["preprocess_bwd"] for d in mine])}
        if a.full:
            mine = [stages[i] for it, i in enumerate(full_calls) if it >= a.warmup]
            r["full_backward_stages"] = {"tile_pass": summary([d["render_bwd"] for d in mine]), "per_gaussian": summary([d["preprocess_bwd"] for d in mine])}
            mine = [stages[i] for it, i in enumerate(sum_calls) if it >= a.warmup and i < len(stages)]
            if mine:
                r["sum_backward_stages"] = {"tile_pass": summary([d["render_bwd"] for d in mine]), "per_gaussian": summary([d["preprocess_bwd"] for d in mine])}
        r.update(info)
        r["beyond_spread"] = {"keep_forward_vs_inference_frame": beyond_spread(r["keep_forward"], r["inference_frame"]),
                              "fov_step_vs_mask_step": beyond_spread(r["fov_step"], r["mask_step"])}
        if a.full:
            r["beyond_spread"].update(full_forward_vs_keep_forward=beyond_spread(r["full_forward"], r["keep_forward"]),
                                      full_backward_vs_appearance_backward=beyond_spread(r["full_backward"], r["backward"]),
                                      full_backward_vs_sum_backward=beyond_spread(r["full_backward"], r["sum_backward"]),
                                      full_step_vs_fov_step=beyond_spread(r["full_step"], r["fov_step"]))
            del mf, opac_f, dcs_f, opt_full, ms
        result["gazes"][f"{gaze[0]},{gaze[1]}"] = r
        print(json.dumps({str(gaze): r}), flush=True)
        del opac, dcs, opt_f, m, model, opt_m
        torch.cuda.empty_cache()
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
