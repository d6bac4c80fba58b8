#!/usr/bin/env python
"""The metamer on the MI355X: what gen_metamer costs, and what a fine-tune step costs with MetamerMSELoss in place of MetamericLoss.

Everything in ONE process, the candidates alternating round by round, each call between two device events; --warmup rounds, then
--steps timed rounds; median, p10-p90, min and max in ms. No target is fixed: the numbers are reported as measured, a result
where the fused form is not faster included, and `beyond_spread` says which differences exceed the spread (one series' p10 above
the other's p90).
  gen_metamer   1088 x 1920, five levels, six orientations, HVSLoss's display geometry, a fixed noise picture:
                fused   MetamerMSELoss.gen_metamer (fr_hvs_metamer, csrc/metamer.hip)
                torch   the same computation in torch operators, float32 on the device: tests/metamer_ref.gen_metamer (the
                        restatement the tests judge the kernels by; F.conv2d, F.interpolate and elementwise operators)
                with the two results' distance, and torch.cuda.max_memory_allocated over one call of each above what is resident;
  roundtrip     pyramid_roundtrip against tests/metamer_ref.roundtrip, likewise;
  loss          the loss alone at that size, forward + backward: MetamerMSELoss with the metamer kept against F.l1_loss;
  train_step    the foveated fine-tune step of tools/fov_train_bench.py --full (S-6M, ring view 0, render(..., differentiable=True),
                backward, optim.Adam on positions, scales, rotations, rest SH, per-level opacities and DCs) at 1088 x 1920, so that
                neither loss resizes: once with MetamericLoss (HVSLoss.calc_fov_loss) and once with MetamerMSELoss whose metamer
                of the target is kept from the warm-up on; `metamer_once` is the first call, which pays for the metamer.
Writes profiles/metamer_bench.json. No GPU, no run: there is no fallback.

usage: python tools/metamer_bench.py [--steps 30] [--warmup 5] [--P 6000000] [--no-train] [--out profiles/metamer_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fov3dgs_amd  # noqa: E402,F401
from fov3dgs_amd import optim  # noqa: E402
from fov3dgs_amd import synthetic as syn  # noqa: E402
from fov3dgs_amd.gaussian_renderer_fov import render as render_fov  # noqa: E402
from fov3dgs_amd.hvs_loss_calc import HVSLoss  # noqa: E402
from fov3dgs_amd.odak_perception import MetamerMSELoss, pyramid_roundtrip  # noqa: E402
from fov3dgs_amd.odak_perception._native_metamer import workspace_floats  # noqa: E402
from tests import hvs_ref, metamer_ref  # noqa: E402
from fov_train_bench import beyond_spread, summary, timed  # noqa: E402

W, H = 1920, 1088
LEVELS, ORIENTATIONS = 5, 6
ALPHA, WIDTH, DISTANCE = 0.05, 1.0, 0.5   # HVSLoss's defaults
GAZE = (0.25, 0.75)


def alternate(candidates, rounds, warmup):
    """{name: callable} -> {name: [ms]}: every round runs each candidate once, in order, between device events"""
    series = {k: [] for k in candidates}
    for it in range(rounds):
        evs = {k: timed(fn)[1:] for k, fn in candidates.items()}
        torch.cuda.synchronize()
        if it >= warmup:
            for k, (e0, e1) in evs.items():
                series[k].append(e0.elapsed_time(e1))
    return series


def peak_above_resident(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--P", type=int, default=6_000_000)
    ap.add_argument("--no-train", action="store_true", help="skip the fine-tune step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metamer_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "metamer_bench needs the MI355X"
    dev = "cuda:0"
    rounds = a.warmup + a.steps
    filt = hvs_ref.filters_from_npz(np.load(os.path.join(ROOT, "tests", "golden", "ref_hvs.npz")), ORIENTATIONS)
    f32 = hvs_ref.filters_to(filt, dtype=torch.float32, device=dev)
    fn = MetamerMSELoss(device=dev, alpha=ALPHA, real_image_width=WIDTH, real_viewing_distance=DISTANCE, n_pyramid_levels=LEVELS,
                        n_orientations=ORIENTATIONS, loss_type="L1", avg_pooling_downup=True, filters=filt)
    g = torch.Generator(device="cpu").manual_seed(3)
    yy, xx = torch.meshgrid(torch.linspace(0, 3, H), torch.linspace(0, 2, W), indexing="ij")
    base = torch.stack([0.5 + 0.2 * torch.sin(xx * (c + 1) + yy) * torch.cos(yy * 1.7 - c) for c in range(3)])
    picture = (base + 0.5 * (torch.rand(base.shape, generator=g) - 0.5)).clamp(0, 1)[None].to(dev)
    noise = torch.rand(picture.shape, generator=g).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "size": [W, H], "levels": LEVELS, "orientations": ORIENTATIONS, "alpha": ALPHA,
              "real_image_width": WIDTH, "real_viewing_distance": DISTANCE, "gaze": list(GAZE), "steps": a.steps, "warmup": a.warmup,
              "workspace_bytes": {"gen_metamer": 4 * workspace_floats(H, W, LEVELS, ORIENTATIONS, False),
                                  "roundtrip": 4 * workspace_floats(H, W, LEVELS, ORIENTATIONS, True)}}

    def torch_metamer():
        with torch.no_grad():
            return metamer_ref.gen_metamer(picture, noise, f32, gaze=GAZE, alpha=ALPHA, real_image_width=WIDTH, real_viewing_distance=DISTANCE,
                                           n_pyramid_levels=LEVELS, mode="quadratic")

    def torch_roundtrip():
        with torch.no_grad():
            return metamer_ref.roundtrip(picture, f32, LEVELS)

    cands = {"fused": lambda: fn.gen_metamer(picture, list(GAZE), noise=noise), "torch": torch_metamer}
    r = {k: summary(v) for k, v in alternate(cands, rounds, a.warmup).items()}
    d = (cands["fused"]() - cands["torch"]()).abs()
    r["fused_vs_torch_float32"] = {"max_abs": float(d.max()), "mean_abs": float(d.mean())}
    r["peak_bytes_above_resident"] = {k: peak_above_resident(v) for k, v in cands.items()}
    r["beyond_spread"] = beyond_spread(r["fused"], r["torch"])
    result["gen_metamer"] = r
    print(json.dumps({"gen_metamer": r}), flush=True)

    cands = {"fused": lambda: pyramid_roundtrip(picture, LEVELS, ORIENTATIONS, filters=filt), "torch": torch_roundtrip}
    r = {k: summary(v) for k, v in alternate(cands, rounds, a.warmup).items()}
    r["peak_bytes_above_resident"] = {k: peak_above_resident(v) for k, v in cands.items()}
    r["beyond_spread"] = beyond_spread(r["fused"], r["torch"])
    result["roundtrip"] = r
    print(json.dumps({"roundtrip": r}), flush=True)

    image = (picture + 0.05 * torch.randn(picture.shape, generator=g).to(dev)).requires_grad_(True)
    kept = fn.gen_metamer(picture, list(GAZE))

    def fused_loss():
        fn(image, picture, gaze=list(GAZE)).backward()
        image.grad = None

    def torch_loss():
        F.l1_loss(image, kept).backward()
        image.grad = None
    r = {k: summary(v) for k, v in alternate({"fused": fused_loss, "torch": torch_loss}, rounds, a.warmup).items()}
    r["beyond_spread"] = beyond_spread(r["fused"], r["torch"])
    result["loss"] = r
    print(json.dumps({"loss": r}), flush=True)
    del image, kept

    if not a.no_train:
        cam, bg = syn.camera_ring(0, 8, W, H).to(dev), torch.zeros(3, device=dev)
        cpu = syn.scene_bicycle_scale(P=a.P, seed=1, opacity_logit=syn.OPACITY_LOGIT_S6M)
        highest, dcs0, opac0 = [t.to(dev) for t in syn.foveation_layers(cpu, seed=2)]
        cloud = cpu.to(dev)
        hvs = HVSLoss(device=dev, filters=filt)
        with torch.no_grad():
            target = render_fov(cam, cloud, bg, alpha=ALPHA, gazeArray=GAZE, blending=True, highest_levels=highest, shs_dcs=dcs0,
                                opacities=(opac0 * 0.8).contiguous())["render"].clone()

        def make_step(loss_of):
            m = syn.GaussianCloud(*[p.detach().clone() for p in cloud.parameters()], sh_degree=cloud.active_sh_degree).requires_grad_(True)
            opac, dcs = opac0.clone().requires_grad_(True), dcs0.clone().requires_grad_(True)
            opt = optim.Adam([{"params": [m._xyz], "lr": 1.6e-6}, {"params": [m._scaling], "lr": 0.005}, {"params": [m._rotation], "lr": 0.001},
                              {"params": [m._features_rest], "lr": 0.000125}, {"params": [opac], "lr": 0.01}, {"params": [dcs], "lr": 0.0025}],
                             lr=0.0, eps=1e-15)

            def step():
                out = render_fov(cam, m, bg, alpha=ALPHA, gazeArray=GAZE, blending=True, highest_levels=highest, shs_dcs=dcs, opacities=opac,
                                 differentiable=True)
                loss_of(out["render"]).backward()
                opt.step()
                opt.zero_grad(set_to_none=True)
            return step
        step_fov = make_step(lambda x: hvs.calc_fov_loss(x, target, gaze=list(GAZE)))
        step_met = make_step(lambda x: fn(x, target, gaze=list(GAZE)))
        step_fov()
        torch.cuda.synchronize()
        _, e0, e1 = timed(step_met)   # its first call: it makes the metamer of the target
        torch.cuda.synchronize()
        once = e0.elapsed_time(e1)
        r = {k: summary(v) for k, v in alternate({"metameric_loss_step": step_fov, "metamer_mse_step": step_met}, rounds, a.warmup).items()}
        r["metamer_once_ms"] = round(once, 4)
        r["beyond_spread"] = beyond_spread(r["metamer_mse_step"], r["metameric_loss_step"])
        r.update(cloud="S-6M", P=a.P, view="camera_ring(0)")
        result["train_step"] = r
        print(json.dumps({"train_step": r}), flush=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
