"""The mask-learning step (metric_mask_learn.py:213: render(masking=True) -> loss -> backward -> optimizer) with and without the
appearance-only backward pass (fr_backward_appearance, render(..., appearance_only=True)), on the MI355X.

On S-6M and S-6M-T, ring view 0, pcheck_obb_sum, a ReferenceShapedModel; everything in ONE process, the two candidates alternating
call by call, each call between two device events; --warmup rounds, then --steps timed rounds; median, min and max in ms:
  (a) the backward call alone, fr_backward against fr_backward_appearance over ONE forward state (raw parameters, split SH), with
      the per-stage times of fr_backward_args.stage_events (tile pass, per-Gaussian pass, zero fill);
  (b) the whole step: render(masking=True[, appearance_only=True]) -> fused l1_ssim_loss -> backward -> optim.Adam.step().
Algorithmic bytes of the lean pass: 40 D + 20 Px + 64 V read, 16 V written, 16 P zeroed (D list entries, Px pixels, V visible
Gaussians); of the full pass: 40 D + 20 Px + 80 V for the tile pass, 276 V + 256 V + 68 (P - V) for the
per-Gaussian pass, 180 P zeroed. No GPU, no run: there is no fallback.

usage: python tools/mask_step_bench.py [--steps 50] [--warmup 10] [--P 6000000] [--out profiles/mask_step_bench.json]"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fov3dgs_amd  # noqa: E402,F401
from fov3dgs_amd import _native, optim, profiling  # noqa: E402
from fov3dgs_amd import synthetic as syn  # noqa: E402
from fov3dgs_amd.gaussian_renderer import render  # noqa: E402
from fov3dgs_amd.loss_utils import l1_ssim_loss  # noqa: E402
from fov3dgs_amd.rasterizer import GaussianRasterizationSettings, _backward_native, _forward_native  # noqa: E402

ARGS = SimpleNamespace(position_lr_init=0.00016, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
W, H = 1920, 1080
VARIANT = "pcheck_obb_sum"


class Pipe:
    debug = False


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "p10_ms": round(sorted(ms)[len(ms) // 10], 4), "p90_ms": round(sorted(ms)[(9 * len(ms)) // 10], 4), "n": len(ms)}


def settings(cam, bg):
    import math
    return GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0,
        viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=3, campos=cam.camera_center,
        prefiltered=False, debug=False)


def backward_alone(cloud, cam, bg, a):
    """(a): one forward state, the two backward calls alternating over it (either leaves the gradient sums cleared for the other)."""
    lib = _native.load()
    vid = _native.VARIANT_IDS[VARIANT]
    rs = settings(cam, bg)
    e = torch.Tensor([])
    P = cloud._xyz.shape[0]
    with torch.no_grad():
        res = _forward_native(vid, rs, cloud._xyz, cloud._features_dc, e, cloud._opacity, cloud._scaling, cloud._rotation, e,
                              sh_rest=cloud._features_rest, raw_activations=True)
    num_rendered, color, radii, geom, binb, img = res[:6]
    target = torch.rand(3, H, W, device=color.device)
    img_leaf = color.detach().requires_grad_(True)
    l1_ssim_loss(img_leaf, target, 0.2).backward()
    dpix = img_leaf.grad.contiguous()
    n_vis = int(geom[lib.fr_geometry_vis_count(vid, P, geom.data_ptr()) - geom.data_ptr():][:4].view(torch.int32).item())
    args = (vid, rs, cloud._xyz, radii, e, cloud._opacity, cloud._scaling, cloud._rotation, e, dpix, cloud._features_dc, geom,
            num_rendered, binb, img)
    kinds = (("full", {}), ("lean", {"appearance_only": True}))
    total = {k: [] for k, _ in kinds}
    rounds = a.warmup + a.steps
    with profiling.BackwardTimer(2 * rounds) as bt:
        evs = []
        for it in range(rounds):
            for k, kw in kinds:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g = _backward_native(*args, sh_rest=cloud._features_rest, raw_activations=True, **kw)
                e1.record()
                evs.append((it, k, e0, e1))
                del g
            torch.cuda.synchronize()
        for it, k, e0, e1 in evs:
            if it >= a.warmup:
                total[k].append(e0.elapsed_time(e1))
        stages = bt.stage_ms()
    bt.close()
    per_stage = {k: {} for k, _ in kinds}
    for i, (k, _) in enumerate(kinds):
        mine = [stages[2 * it + i] for it in range(a.warmup, rounds)]
        for name in ("render_bwd", "preprocess_bwd", "fill_zero"):
            per_stage[k]["per_gaussian" if name == "preprocess_bwd" else name] = summary([d[name] for d in mine])
    D, Px, V = int(num_rendered), W * H, n_vis
    bytes_ = {"lean": {"read": 40 * D + 20 * Px + 64 * V, "written": 16 * V, "zeroed": 16 * P},
              "full": {"read": 40 * D + 20 * Px + 80 * V + 276 * V, "written": 256 * V + 68 * (P - V), "zeroed": 180 * P}}
    return {"D": D, "Px": Px, "V": V, "P": P, "backward_call": {k: summary(total[k]) for k, _ in kinds}, "stages": per_stage,
            "algorithmic_bytes": bytes_}


def whole_step(base, cam, bg, a):
    """(b): two models of the same cloud, one stepped with the full masking backward, one with the appearance-only one, alternating."""
    target = torch.rand(3, H, W, device=bg.device)
    cands = []
    for name, kw in (("masking", {}), ("masking_appearance_only", {"appearance_only": True})):
        m = syn.GaussianCloud(*[p.detach().clone() for p in base.parameters()], sh_degree=base.active_sh_degree).requires_grad_(True)
        cands.append(dict(name=name, kw=kw, cloud=m, model=syn.ReferenceShapedModel(m),
                          opt=optim.Adam(optim.reference_param_groups(m, ARGS), lr=0.0, eps=1e-15), ms=[]))
    for it in range(a.warmup + a.steps):
        evs = []
        for c in cands:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = render(cam, c["model"], Pipe(), bg, masking=True, cuda_type=VARIANT, **c["kw"])
            l1_ssim_loss(out["render"], target, 0.2).backward()
            c["opt"].step()
            c["opt"].zero_grad(set_to_none=True)
            e1.record()
            evs.append((c, e0, e1))
        torch.cuda.synchronize()
        if it >= a.warmup:
            for c, e0, e1 in evs:
                c["ms"].append(e0.elapsed_time(e1))
    return {c["name"]: summary(c["ms"]) for c in cands}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--P", type=int, default=6_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_step_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mask_step_bench needs the MI355X"
    assert a.steps >= 50, "at least 50 timed repetitions per candidate"
    dev = "cuda:0"
    cam, bg = syn.camera_ring(0, width=W, height=H).to(dev), torch.zeros(3, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "variant": VARIANT, "view": "camera_ring(0)", "steps": a.steps, "warmup": a.warmup,
              "clouds": {}}
    for name, make in (("S-6M", syn.scene_bicycle_scale), ("S-6M-T", syn.scene_translucent)):
        cloud = make(P=a.P).to(dev)
        r = backward_alone(cloud, cam, bg, a)
        r["mask_step"] = whole_step(cloud, cam, bg, a)
        f, l = r["backward_call"]["full"], r["backward_call"]["lean"]
        # faster by more than the spread: the lean series' slow end (p90) below the full series' fast end (p10)
        r["lean_backward_faster_beyond_spread"] = bool(l["p90_ms"] < f["p10_ms"])
        result["clouds"][name] = r
        print(json.dumps({name: r}), flush=True)
        del cloud
        torch.cuda.empty_cache()
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    for name, r in result["clouds"].items():
        assert r["lean_backward_faster_beyond_spread"], f"{name}: the lean backward call is not faster than the full one beyond the spread"


if __name__ == "__main__":
    main()
