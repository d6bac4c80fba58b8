"""Three steps of prune.py's loop, fused (fov3dgs_amd.quality, fov3dgs_amd.pruning; csrc/quality.hip, csrc/prune_step.hip) against
their torch form, on S-6M at 1080p on the MI355X, in ONE process, the two candidates alternating round by round; --warmup rounds,
then the timed rounds; median, p10-p90, min and max in ms:
  (a) gate           the quality gate over 8 views (prune.py:284-290). fused: quality.evaluate_views -- one render (pcheck_obb,
                     no_grad) and the meter's two launches per view, ONE readback. reference_form: test_ssim_loss then
                     test_psnr_loss (prune.py:137-174) -- two renders per view with this package's renderer, the torch SSIM (five
                     grouped 121-tap convolutions) and the torch psnr, the sums kept as device scalars and read back once each
                     (the reference's comparison with the target). Host time between two device synchronisations: the gate ends
                     with a readback, so the host is part of it.
  (b) train_step     prune.py:242-276 with the scale-decay term: render(pcheck_obb_sum) -> l1_ssim_loss + scale term * 1e-4 ->
                     backward -> optim.Adam.step(). fused: pruning.scale_decay_loss(model._scaling, gs_count, raw=True);
                     torch_term: (max(get_scaling, dim=1) * (gs_count - 4) * (gs_count > 4)).mean(). Device events.
  (c) cap            reset_opacity_max(max=0.1) on the [P,1] opacities with their Adam state. fused: pruning.reset_opacity_max;
                     torch_sequence: gaussian_model.py:427-431 with replace_tensor_to_optimizer :609-622 (sigmoid, min, logit, two
                     zeros_like, a new Parameter, the swap of the state). Device events.
<a>_faster_beyond_spread: the fused form's p90 lies below the other form's p10. No GPU, no run: there is no fallback.

usage: python tools/prune_step_bench.py [--rounds 30] [--gate-rounds 10] [--warmup 3] [--P 6000000] [--views 8]
                                        [--out profiles/prune_step_bench.json]"""
import argparse
import json
import math
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fov3dgs_amd  # noqa: E402,F401
from fov3dgs_amd import optim, pruning, quality  # noqa: E402
from fov3dgs_amd import synthetic as syn  # noqa: E402
from fov3dgs_amd.gaussian_renderer import render  # noqa: E402
from fov3dgs_amd.loss_utils import l1_ssim_loss  # noqa: E402

ARGS = SimpleNamespace(position_lr_init=0.00016, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
W, H = 1920, 1080
SCALE_WEIGHT = 1e-4


class Pipe:
    debug = False


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "p10_ms": round(sorted(ms)[len(ms) // 10], 4), "p90_ms": round(sorted(ms)[(9 * len(ms)) // 10], 4), "n": len(ms)}


def beyond_spread(fast, slow):
    return bool(fast["p90_ms"] < slow["p10_ms"])


def torch_window(dev):
    g = torch.tensor([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().expand(3, 1, 11, 11).contiguous().to(dev)


def torch_ssim(a, b, w):
    """loss_utils.py:57-76 in torch's own operators"""
    mu1, mu2 = F.conv2d(a, w, padding=5, groups=3), F.conv2d(b, w, padding=5, groups=3)
    s1 = F.conv2d(a * a, w, padding=5, groups=3) - mu1.pow(2)
    s2 = F.conv2d(b * b, w, padding=5, groups=3) - mu2.pow(2)
    s12 = F.conv2d(a * b, w, padding=5, groups=3) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1.pow(2) + mu2.pow(2) + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return m.mean()


def torch_psnr(a, b):
    """image_utils.py:17-19"""
    mse = ((a - b) ** 2).view(a.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def model_of(base):
    m = syn.GaussianCloud(*[p.detach().clone() for p in base.parameters()], sh_degree=base.active_sh_degree).requires_grad_(True)
    m.optimizer = optim.Adam(optim.reference_param_groups(m, ARGS), lr=0.0, eps=1e-15)
    return m


def gate(base, dev, a):
    bg = torch.zeros(3, device=dev)
    cams = [syn.camera_ring(i, n=a.views, width=W, height=H).to(dev) for i in range(a.views)]
    gen = torch.Generator(device=dev).manual_seed(1)
    with torch.no_grad():
        for c in cams:
            r = render(c, base, Pipe(), bg, cuda_type="pcheck_obb")["render"]
            c.original_image = (r + 0.02 * torch.randn(r.shape, device=dev, generator=gen)).clamp(0, 1)
    w = torch_window(dev)

    def fused():
        r = quality.evaluate_views(base, cams, Pipe(), bg)
        return r["ssim"], r["psnr"]

    def reference_form():
        ssim_sum = 0.0
        for c in cams:
            with torch.no_grad():
                image = render(c, base, Pipe(), bg, cuda_type="pcheck_obb")["render"]
                ssim_sum += torch_ssim(image.unsqueeze(0), c.original_image.unsqueeze(0), w)
        psnr_sum = 0.0
        for c in cams:
            with torch.no_grad():
                image = render(c, base, Pipe(), bg, cuda_type="pcheck_obb")["render"]
                psnr_sum += torch_psnr(image.unsqueeze(0), c.original_image.unsqueeze(0)).mean()
        return float(ssim_sum / len(cams)), float(psnr_sum / len(cams))

    forms = (("fused", fused), ("reference_form", reference_form))
    ms, values = {k: [] for k, _ in forms}, {}
    for it in range(a.warmup + a.gate_rounds):
        for k, fn in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            values[k] = fn()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ms[k].append(1e3 * (time.perf_counter() - t0))
    r = {k: summary(v) for k, v in ms.items()}
    r["views"] = a.views
    r["ssim_psnr"] = {k: list(v) for k, v in values.items()}
    r["fused_faster_beyond_spread"] = beyond_spread(r["fused"], r["reference_form"])
    return r


def train_step(base, dev, a):
    cam, bg = syn.camera_ring(0, width=W, height=H).to(dev), torch.zeros(3, device=dev)
    target = torch.rand(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(2))

    def fused_term(m, gs_count):
        return pruning.scale_decay_loss(m._scaling, gs_count, raw=True)

    def torch_term(m, gs_count):  # prune.py:258-260
        scale_max, _ = torch.max(m.get_scaling, dim=1)
        return (scale_max * (gs_count - 4) * (gs_count > 4)).mean()

    cands = [dict(name=n, term=t, model=model_of(base), ms=[]) for n, t in (("fused", fused_term), ("torch_term", torch_term))]
    values = {}
    for it in range(a.warmup + a.rounds):
        evs = []
        for c in cands:
            m = c["model"]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pkg = render(cam, m, Pipe(), bg, cuda_type="pcheck_obb_sum")
            loss = l1_ssim_loss(pkg["render"], target, 0.2)
            term = c["term"](m, pkg["gs_count"])
            loss = loss + term * SCALE_WEIGHT
            loss.backward()
            m.optimizer.step()
            m.optimizer.zero_grad(set_to_none=True)
            e1.record()
            evs.append((c, e0, e1))
            values[c["name"]] = term.detach()
        torch.cuda.synchronize()
        if it >= a.warmup:
            for c, e0, e1 in evs:
                c["ms"].append(e0.elapsed_time(e1))
    r = {c["name"]: summary(c["ms"]) for c in cands}
    r["scale_loss"] = {k: float(v) for k, v in values.items()}
    r["fused_faster_beyond_spread"] = beyond_spread(r["fused"], r["torch_term"])
    return r


def torch_reset_opacity_max(m, cap):
    """gaussian_model.py:427-431 and :609-622"""
    op = torch.sigmoid(m._opacity)
    x = torch.min(op, torch.ones_like(op) * cap)
    new = torch.log(x / (1 - x))
    opt = m.optimizer
    for group in opt.param_groups:
        if group["name"] == "opacity":
            st = opt.state.get(group["params"][0], None)
            st["exp_avg"] = torch.zeros_like(new)
            st["exp_avg_sq"] = torch.zeros_like(new)
            del opt.state[group["params"][0]]
            group["params"][0] = torch.nn.Parameter(new.requires_grad_(True))
            opt.state[group["params"][0]] = st
            m._opacity = group["params"][0]


def cap(base, dev, a):
    cands = [dict(name=n, fn=f, model=model_of(base), ms=[]) for n, f in
             (("fused", lambda m: pruning.reset_opacity_max(m, max=0.1)), ("torch_sequence", lambda m: torch_reset_opacity_max(m, 0.1)))]
    for c in cands:  # one step: the opacity group has state
        c["model"]._opacity.grad = torch.zeros_like(c["model"]._opacity)
        c["model"].optimizer.step()
        c["model"].optimizer.zero_grad(set_to_none=True)
    start = base._opacity.detach().clone()
    for it in range(a.warmup + a.rounds):
        evs = []
        for c in cands:
            with torch.no_grad():
                c["model"]._opacity.copy_(start)  # the same work every round (rows_above_the_cap of them are capped)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            with torch.no_grad():
                c["fn"](c["model"])
            e1.record()
            evs.append((c, e0, e1))
        torch.cuda.synchronize()
        if it >= a.warmup:
            for c, e0, e1 in evs:
                c["ms"].append(e0.elapsed_time(e1))
    r = {c["name"]: summary(c["ms"]) for c in cands}
    r["rows_above_the_cap"] = int((torch.sigmoid(start) > 0.1).sum())
    r["largest_opacity_after"] = {c["name"]: float(torch.sigmoid(c["model"]._opacity.detach()).max()) for c in cands}
    r["fused_faster_beyond_spread"] = beyond_spread(r["fused"], r["torch_sequence"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--gate-rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--P", type=int, default=6_000_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_step_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "prune_step_bench needs the MI355X"
    dev = "cuda:0"
    base = syn.scene_bicycle_scale(P=a.P).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "scene": "S-6M" if a.P == 6_000_000 else f"scene_bicycle_scale(P={a.P})",
              "size": [H, W], "rounds": a.rounds, "gate_rounds": a.gate_rounds, "warmup": a.warmup,
              "protocol": "one process, the candidates alternate round by round; gate: host time between device synchronisations; "
                          "train_step and cap: device events around one round"}
    for name, fn in (("gate", gate), ("train_step", train_step), ("cap", cap)):
        result[name] = fn(base, dev, a)
        print(json.dumps({name: result[name]}), flush=True)
        torch.cuda.empty_cache()
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
