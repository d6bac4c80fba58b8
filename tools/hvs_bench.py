"""The uniform metameric (HVS) loss, fused (fov3dgs_amd.odak_perception.MetamericLossUniform, csrc/hvs.hip) against its torch
form (tests/hvs_ref.py in float32 on the GPU: the reference's operators, each channel filtered on its own and without the
reference's host synchronisation per call, so the torch side is if anything flattered), on the MI355X, in ONE process, the two
candidates alternating call by call, each call between two device events; --warmup rounds, then --steps timed rounds; median,
p10-p90, min and max in ms:
  (a) loss + backward at 1088x1920 (the size metric_mask_learn.py / eff_finetune.py resize 1080p to), 5 levels, 6 orientations,
      L1, pooling 1, 9 and 25; a new target tensor every call, as in the training loops (both pyramids are computed);
  (b) the mask-learning step as the method runs it: render(masking=True, appearance_only=True) -> bilinear resize to 1088x1920
      (a torch call in the caller) -> this loss (pooling 9) -> backward -> optim.Adam.step(), on S-6M and S-6M-T, beside the
      same step with the torch loss.
and, from pictures of 1080x1920 as the scripts hold them (section "resized" of the result), the resize the parent of this
keyword left to the caller against the resize inside the kernels, the same protocol:
  (a') loss + backward at pooling 9, a new target tensor every round: interpolate_then_fused (F.interpolate of both pictures to
       1088x1920, the fused loss, backward through both) against fused_resize (resize="pyramid");
  (b') the mask-learning step on S-6M with targets at 1080x1920 in the same two forms, and fused_resize_fixed_target: one target
       object held across the rounds, whose pyramid state the loss object then reuses (a caller with its ground truth on the GPU);
  per form torch.cuda.max_memory_allocated of one step above what was allocated before it, and whether the image gradient of
  two identical rounds is the same bits (torch lists upsample_bilinear2d_backward as non-deterministic; ours is a gather).
  fused_resize_not_slower_beyond_spread: fused_resize's p10 does not lie above interpolate_then_fused's p90.
--foveated measures the gaze-dependent loss instead (fov3dgs_amd.odak_perception.MetamericLoss, csrc/hvs_fov.hip) and writes
profiles/hvs_fov_bench.json: HVSLoss's defaults (alpha 0.05, width 1.0, distance 0.5, 5 levels, 6 orientations, MSE), at 1088x1920
and from 1080x1920 pictures with the resize (resize="pyramid" against F.interpolate in front of the torch form), gaze at the
centre and at (0.1, 0.1); loss + backward and the forward alone; three candidates alternating call by call, a new target tensor
every round: fused_fov, torch_fov (tests/hvs_fov_ref.py in float32 on the GPU with its LOD maps built once, as the reference
caches them) and fused_uniform_p9 (the uniform loss at pooling 9, MSE). Per candidate the peak memory of one step, and the
relative difference of the two foveated losses. fused_faster_beyond_spread: fused_fov's p90 lies below torch_fov's p10.
The filter coefficients come from tests/golden/ref_hvs.npz. No GPU, no run: there is no fallback.

usage: python tools/hvs_bench.py [--steps 50] [--warmup 10] [--step-rounds 30] [--P 6000000] [--skip-step] [--resized-only]
                                 [--foveated] [--out profiles/hvs_bench.json]
--resized-only measures the section "resized" alone and keeps the other sections of an existing --out file as they are."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fov3dgs_amd  # noqa: E402,F401
from fov3dgs_amd import optim  # noqa: E402
from fov3dgs_amd import synthetic as syn  # noqa: E402
from fov3dgs_amd.gaussian_renderer import render  # noqa: E402
from fov3dgs_amd.odak_perception import MetamericLoss, MetamericLossUniform, _native_hvs, _native_hvs_fov  # noqa: E402
from tests import hvs_fov_ref, hvs_ref  # noqa: E402

ARGS = SimpleNamespace(position_lr_init=0.00016, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
W, H = 1920, 1080
HL, WL = 1088, 1920
LEVELS, ORIENTATIONS = 5, 6
VARIANT = "pcheck_obb_sum"


class Pipe:
    debug = False


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "p10_ms": round(sorted(ms)[len(ms) // 10], 4), "p90_ms": round(sorted(ms)[(9 * len(ms)) // 10], 4), "n": len(ms)}


def filters():
    return hvs_ref.filters_from_npz(np.load(os.path.join(ROOT, "tests", "golden", "ref_hvs.npz")), ORIENTATIONS)


def candidates(pooling, dev):
    f = filters()
    fused = MetamericLossUniform(device=dev, pooling_size=pooling, n_pyramid_levels=LEVELS, n_orientations=ORIENTATIONS, loss_type="L1",
                                 bilinear_downsampling=True, filters=f)
    f32 = hvs_ref.filters_to(f, dtype=torch.float32, device=dev)
    return (("fused", lambda x, t: fused(x, t)), ("torch", lambda x, t: hvs_ref.hvs_loss(x, t, f32, pooling, LEVELS, "L1")))


def loss_alone(pooling, dev, a):
    gen = torch.Generator(device=dev).manual_seed(1)
    base = torch.rand(1, 3, HL, WL, device=dev, generator=gen)
    image = (base + 0.05 * torch.randn(1, 3, HL, WL, device=dev, generator=gen)).clamp(0, 1)
    cands = candidates(pooling, dev)
    ms, values = {k: [] for k, _ in cands}, {}
    for it in range(a.warmup + a.steps):
        evs = []
        target = base.clone()  # a new tensor every round: nothing is reused from call to call
        for k, fn in cands:
            x = image.clone().requires_grad_(True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = fn(x, target)
            loss.backward()
            e1.record()
            evs.append((k, e0, e1))
            values[k] = loss.detach()
        torch.cuda.synchronize()
        if it >= a.warmup:
            for k, e0, e1 in evs:
                ms[k].append(e0.elapsed_time(e1))
    st = _native_hvs.Settings(HL, WL, float(pooling), LEVELS, ORIENTATIONS, 0, 1)
    r = {k: summary(v) for k, v in ms.items()}
    r["loss"] = {k: float(v) for k, v in values.items()}
    r["state_bytes_per_picture"] = 4 * _native_hvs.floats(st, 0)
    r["backward_workspace_bytes"] = 4 * _native_hvs.floats(st, 1)
    r["fused_faster_beyond_spread"] = bool(r["fused"]["p90_ms"] < r["torch"]["p10_ms"])
    return r


def mask_step(base, cam, bg, dev, a, pooling=9):
    gen = torch.Generator(device=dev).manual_seed(2)
    target_pool = [torch.rand(1, 3, HL, WL, device=dev, generator=gen) for _ in range(2)]
    cands = []
    for name, fn in candidates(pooling, dev):
        m = syn.GaussianCloud(*[p.detach().clone() for p in base.parameters()], sh_degree=base.active_sh_degree).requires_grad_(True)
        cands.append(dict(name=name, fn=fn, model=syn.ReferenceShapedModel(m),
                          opt=optim.Adam(optim.reference_param_groups(m, ARGS), lr=0.0, eps=1e-15), ms=[]))
    for it in range(a.warmup + a.step_rounds):
        evs = []
        target = target_pool[it % 2].clone()
        for c in cands:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = render(cam, c["model"], Pipe(), bg, masking=True, cuda_type=VARIANT, appearance_only=True)
            img = F.interpolate(out["render"].unsqueeze(0), size=(HL, WL), mode="bilinear")
            c["fn"](img, target).backward()
            c["opt"].step()
            c["opt"].zero_grad(set_to_none=True)
            e1.record()
            evs.append((c, e0, e1))
        torch.cuda.synchronize()
        if it >= a.warmup:
            for c, e0, e1 in evs:
                c["ms"].append(e0.elapsed_time(e1))
    r = {"mask_step_" + c["name"] + "_loss": summary(c["ms"]) for c in cands}
    r["fused_faster_beyond_spread"] = bool(r["mask_step_fused_loss"]["p90_ms"] < r["mask_step_torch_loss"]["p10_ms"])
    return r


def resize_forms(pooling, dev):
    """(name, fn(image [3,H,W] requiring grad, target [3,H,W]) -> loss): the two ways to the loss from 1080x1920 pictures"""
    def make():
        return MetamericLossUniform(device=dev, pooling_size=pooling, n_pyramid_levels=LEVELS, n_orientations=ORIENTATIONS, loss_type="L1",
                                    bilinear_downsampling=True, filters=filters())
    before, inside = make(), make()

    def interpolate_then_fused(x, t):  # metric_mask_learn.py:221-227
        t = F.interpolate(t.unsqueeze(0), size=(HL, WL), mode="bilinear", align_corners=False)
        x = F.interpolate(x.unsqueeze(0), size=(HL, WL), mode="bilinear", align_corners=False)
        return before(x, t)

    def fused_resize(x, t):  # t itself, not a view of it: the target state is keyed by the object
        return inside(x, t, resize="pyramid")

    fused_resize.loss_object = inside
    return (("interpolate_then_fused", interpolate_then_fused), ("fused_resize", fused_resize))


def peak_bytes(step):
    """torch.cuda.max_memory_allocated of one call of step() above what was allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def resized_loss_alone(dev, a, pooling=9):
    gen = torch.Generator(device=dev).manual_seed(3)
    base = torch.rand(3, H, W, device=dev, generator=gen)
    image = (base + 0.05 * torch.randn(3, H, W, device=dev, generator=gen)).clamp(0, 1)
    forms = resize_forms(pooling, dev)
    ms, values, grads = {k: [] for k, _ in forms}, {}, {k: [] for k, _ in forms}

    def step(fn, target):
        x = image.clone().requires_grad_(True)
        loss = fn(x, target)
        loss.backward()
        return loss, x.grad

    for it in range(a.warmup + a.steps):
        evs = []
        target = base.clone()  # a new tensor every round
        for k, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss, grad = step(fn, target)
            e1.record()
            evs.append((k, e0, e1))
            values[k] = loss.detach()
            if it < 2:
                grads[k].append(grad.clone())
        torch.cuda.synchronize()
        if it >= a.warmup:
            for k, e0, e1 in evs:
                ms[k].append(e0.elapsed_time(e1))
    r = {k: summary(v) for k, v in ms.items()}
    r["loss"] = {k: float(v) for k, v in values.items()}
    r["image_gradient_of_two_identical_rounds_equal"] = {k: bool(torch.equal(*g)) for k, g in grads.items()}
    r["peak_bytes_of_one_step"] = {k: peak_bytes(lambda fn=fn: step(fn, base.clone())) for k, fn in forms}
    r["fused_resize_not_slower_beyond_spread"] = bool(r["fused_resize"]["p10_ms"] <= r["interpolate_then_fused"]["p90_ms"])
    return r


def resized_mask_step(base, cam, bg, dev, a, pooling=9):
    gen = torch.Generator(device=dev).manual_seed(4)
    target_pool = [torch.rand(3, H, W, device=dev, generator=gen) for _ in range(2)]
    fixed = target_pool[0].clone()
    forms = list(resize_forms(pooling, dev))
    forms.append(("fused_resize_fixed_target", resize_forms(pooling, dev)[1][1]))  # a loss object of its own: its state is its own
    cands = []
    for name, fn in forms:
        m = syn.GaussianCloud(*[p.detach().clone() for p in base.parameters()], sh_degree=base.active_sh_degree).requires_grad_(True)
        cands.append(dict(name=name, fn=fn, model=syn.ReferenceShapedModel(m),
                          opt=optim.Adam(optim.reference_param_groups(m, ARGS), lr=0.0, eps=1e-15), ms=[]))

    def step(c, target):
        out = render(cam, c["model"], Pipe(), bg, masking=True, cuda_type=VARIANT, appearance_only=True)
        c["fn"](out["render"], target).backward()
        c["opt"].step()
        c["opt"].zero_grad(set_to_none=True)

    for it in range(a.warmup + a.step_rounds):
        evs = []
        target = target_pool[it % 2].clone()
        for c in cands:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(c, fixed if c["name"].endswith("fixed_target") else target)
            e1.record()
            evs.append((c, e0, e1))
        torch.cuda.synchronize()
        if it >= a.warmup:
            for c, e0, e1 in evs:
                c["ms"].append(e0.elapsed_time(e1))
    r = {"mask_step_" + c["name"]: summary(c["ms"]) for c in cands}
    held = cands[2]["fn"].loss_object._target  # the fixed target's state must be the one object from the first round on
    state_ptr = held[2].data_ptr()
    step(cands[2], fixed)
    r["fixed_target_state_reused"] = bool(cands[2]["fn"].loss_object._target[2].data_ptr() == state_ptr and held[0]() is fixed)
    r["peak_bytes_of_one_step"] = {c["name"]: peak_bytes(lambda c=c: step(c, fixed if c["name"].endswith("fixed_target") else target_pool[1]))
                                   for c in cands}
    r["fused_resize_not_slower_beyond_spread"] = bool(r["mask_step_fused_resize"]["p10_ms"] <= r["mask_step_interpolate_then_fused"]["p90_ms"])
    return r


def resized(dev, a):
    r = {"source_size": [H, W], "pooling": 9, "loss_and_backward": resized_loss_alone(dev, a)}
    print(json.dumps({"resized_loss_and_backward": r["loss_and_backward"]}), flush=True)
    torch.cuda.empty_cache()
    if not a.skip_step:
        cam, bg = syn.camera_ring(0, width=W, height=H).to(dev), torch.zeros(3, device=dev)
        cloud = syn.scene_bicycle_scale(P=a.P).to(dev)
        r["mask_step"] = {"S-6M": resized_mask_step(cloud, cam, bg, dev, a)}
        r["mask_step_rounds"] = a.step_rounds
        print(json.dumps({"resized_mask_step": r["mask_step"]}), flush=True)
        del cloud
        torch.cuda.empty_cache()
    else:
        r["mask_step"] = "not measured (--skip-step)"
    return r


FOV = dict(alpha=0.05, real_image_width=1.0, real_viewing_distance=0.5, mode="quadratic")  # hvs_loss_calc.py:22-23, :40


def foveated_forms(dev, gaze, source):
    """(name, fn(image [1,3,h,w], target) -> loss) for pictures of size `source`, (HL, WL) or (H, W) with the resize"""
    f = filters()
    resize = None if source == (HL, WL) else "pyramid"
    fov = MetamericLoss(device=dev, n_pyramid_levels=LEVELS, n_orientations=ORIENTATIONS, use_l2_foveal_loss=False, loss_type="MSE",
                        use_bilinear_downup=True, filters=f, **FOV)
    uni = MetamericLossUniform(device=dev, pooling_size=9, n_pyramid_levels=LEVELS, n_orientations=ORIENTATIONS, loss_type="MSE",
                               bilinear_downsampling=True, filters=f)
    f32 = hvs_ref.filters_to(f, dtype=torch.float32, device=dev)
    lods = hvs_fov_ref.lod_maps(gaze, HL, WL, LEVELS, FOV["alpha"], FOV["real_image_width"], FOV["real_viewing_distance"], FOV["mode"],
                                torch.float32, dev)

    def torch_fov(x, t):
        if resize:
            x = F.interpolate(x, size=(HL, WL), mode="bilinear", align_corners=False)
            t = F.interpolate(t, size=(HL, WL), mode="bilinear", align_corners=False)
        return hvs_fov_ref.fov_loss(x, t, f32, n_pyramid_levels=LEVELS, loss_type="MSE", lods=lods)

    return (("fused_fov", lambda x, t: fov(x, t, gaze=gaze, resize=resize)), ("torch_fov", torch_fov),
            ("fused_uniform_p9", lambda x, t: uni(x, t, resize=resize)))


def foveated_one(dev, a, gaze, source):
    gen = torch.Generator(device=dev).manual_seed(5)
    base = torch.rand(1, 3, *source, device=dev, generator=gen)
    image = (base + 0.05 * torch.randn(1, 3, *source, device=dev, generator=gen)).clamp(0, 1)
    forms = foveated_forms(dev, gaze, source)

    def step(fn, target, backward):
        if not backward:
            with torch.no_grad():
                return fn(image, target), None
        x = image.clone().requires_grad_(True)
        loss = fn(x, target)
        loss.backward()
        return loss.detach(), x.grad

    r = {}
    for what, backward in (("loss_and_backward", True), ("forward_only", False)):
        ms, values, grads = {k: [] for k, _ in forms}, {}, {k: [] for k, _ in forms}
        for it in range(a.warmup + a.steps):
            evs = []
            target = base.clone()  # a new tensor every round: nothing of the target is reused from call to call
            for k, fn in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                loss, grad = step(fn, target, backward)
                e1.record()
                evs.append((k, e0, e1))
                values[k] = loss
                if backward and it < 2:
                    grads[k].append(grad.clone())
            torch.cuda.synchronize()
            if it >= a.warmup:
                for k, e0, e1 in evs:
                    ms[k].append(e0.elapsed_time(e1))
        q = {k: summary(v) for k, v in ms.items()}
        q["loss"] = {k: float(v) for k, v in values.items()}
        q["fov_loss_relative_difference_fused_vs_torch"] = abs(q["loss"]["fused_fov"] - q["loss"]["torch_fov"]) / q["loss"]["torch_fov"]
        if backward:
            q["image_gradient_of_two_identical_rounds_equal"] = {k: bool(torch.equal(*g)) for k, g in grads.items()}
            q["fov_gradient_relative_l2_fused_vs_torch"] = float((grads["fused_fov"][0] - grads["torch_fov"][0]).norm() / grads["torch_fov"][0].norm())
        del grads
        q["peak_bytes_of_one_step"] = {k: peak_bytes(lambda fn=fn: step(fn, base.clone(), backward)) for k, fn in forms}
        q["fused_faster_beyond_spread"] = bool(q["fused_fov"]["p90_ms"] < q["torch_fov"]["p10_ms"])
        r[what] = q
        torch.cuda.empty_cache()
    return r


def foveated(dev, a):
    st = _native_hvs_fov.Settings(HL, WL, FOV["alpha"], FOV["real_image_width"], FOV["real_viewing_distance"], 1, 0.5, 0.5, LEVELS, ORIENTATIONS, 1, 1)
    result = {"device": torch.cuda.get_device_name(0), "size": [HL, WL], "resized_from": [H, W], "levels": LEVELS, "orientations": ORIENTATIONS,
              "loss_type": "MSE", "settings": FOV, "steps": a.steps, "warmup": a.warmup,
              "torch_form": "tests/hvs_fov_ref.py, float32, grouped convolutions, LOD maps built once, no host synchronisation",
              "state_bytes_per_picture": 4 * _native_hvs_fov.floats(st, 0), "backward_workspace_bytes": 4 * _native_hvs_fov.floats(st, 1),
              "lod_bytes": 4 * _native_hvs_fov.floats(st, 3), "runs": {}}
    for source in ((HL, WL), (H, W)):
        for gaze in ([0.5, 0.5], [0.1, 0.1]):
            name = f"{source[0]}x{source[1]}{'' if source == (HL, WL) else '_resized'}/gaze_{gaze[0]}_{gaze[1]}"
            result["runs"][name] = foveated_one(dev, a, gaze, source)
            print(json.dumps({name: result["runs"][name]}), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=30)
    ap.add_argument("--P", type=int, default=6_000_000)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--resized-only", action="store_true")
    ap.add_argument("--foveated", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "hvs_fov_bench.json" if a.foveated else "hvs_bench.json")
    assert torch.cuda.is_available(), "hvs_bench needs the MI355X"
    dev = "cuda:0"
    if a.foveated:
        result = foveated(dev, a)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        return
    if a.resized_only:
        with open(a.out) as fh:
            result = json.load(fh)
        result["resized"] = dict(resized(dev, a), steps=a.steps, warmup=a.warmup)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        return
    result = {"device": torch.cuda.get_device_name(0), "size": [HL, WL], "levels": LEVELS, "orientations": ORIENTATIONS, "loss_type": "L1",
              "steps": a.steps, "warmup": a.warmup, "torch_form": "tests/hvs_ref.py, float32, grouped convolutions, no host synchronisation",
              "loss_and_backward": {}, "mask_step": {}}
    for pooling in (1, 9, 25):
        r = loss_alone(pooling, dev, a)
        result["loss_and_backward"][f"pooling_{pooling}"] = r
        print(json.dumps({f"pooling_{pooling}": r}), flush=True)
        torch.cuda.empty_cache()
    if not a.skip_step:
        cam, bg = syn.camera_ring(0, width=W, height=H).to(dev), torch.zeros(3, device=dev)
        result["mask_step_rounds"] = a.step_rounds
        for name, make in (("S-6M", syn.scene_bicycle_scale), ("S-6M-T", syn.scene_translucent)):
            cloud = make(P=a.P).to(dev)
            r = mask_step(cloud, cam, bg, dev, a)
            result["mask_step"][name] = r
            print(json.dumps({name: r}), flush=True)
            del cloud
            torch.cuda.empty_cache()
    else:
        result["mask_step"] = "not measured (--skip-step)"
    result["resized"] = dict(resized(dev, a), steps=a.steps, warmup=a.warmup)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
