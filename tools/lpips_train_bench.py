#!/usr/bin/env python
"""LPIPS (VGG16) as a training loss on one 1080 x 1920 picture pair, N = 1, seeded random weights (tests/lpips_cases.weights):
the fused differentiable call (fov3dgs_amd.lpipsPyTorch.LPIPSLoss: fr_lpips_forward_keep + fr_lpips_backward, csrc/lpips.hip)
against the same network written with F.conv2d, F.max_pool2d and the torch head under torch.autograd (tools/lpips_bench.py's torch
form, float32, the weights resident on the device; y's branch under no_grad, as the target carries no gradient). The candidates
alternate round by round, each call between device events; --warmup rounds, then --steps timed rounds; median, p10-p90, min, max.
  call            forward + backward of each form, and the two halves of it;
  backward_stages the fused backward's 13 stages (fr_lpips_backward_args.stage_events), medians of a separate pass, with the
                  achieved TFLOP/s of the twelve matrix-core convolutions (2 x 9 Cin Cout H W of ONE picture) against the 157.3
                  TFLOP/s of the f32 matrix cores; forward_stages likewise for the keeping forward;
  peak_bytes      torch.cuda.max_memory_allocated over one forward + backward of each form, above what is resident before it
                  (pictures, weights; the fused form's workspace and kept state are counted);
  train_step      --train: render (pcheck_obb_sum, --P Gaussians, 1080 x 1920) -> l1_ssim_loss + lambda * LPIPS -> backward ->
                  optim.Adam (row-sparse, exact), once with the fused term and once with the torch one, alternating, and without
                  the term for scale.
Writes profiles/lpips_backward_bench.json."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import fov3dgs_amd  # noqa: E402,F401
from fov3dgs_amd import lpipsPyTorch, optim  # noqa: E402
from fov3dgs_amd import synthetic as syn  # noqa: E402
from fov3dgs_amd.gaussian_renderer import render  # noqa: E402
from fov3dgs_amd.loss_utils import l1_ssim_loss  # noqa: E402
from tests import lpips_cases, lpips_ref  # noqa: E402
from lpips_bench import PEAK_F32_TFLOPS, _stats, torch_form  # noqa: E402
from optim_bench import ARGS, Pipe, clone_model  # noqa: E402


def _timed(fn):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    v = fn()
    e[1].record()
    v.sum().backward()
    e[2].record()
    e[2].synchronize()
    return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])


def conv_flops(H, W):
    """{stage: 2 x 9 Cin Cout H_l W_l} of one picture, by the forward's stage names"""
    names = [n for n in lpipsPyTorch.STAGES if n.startswith("conv")]
    per, h, w = {}, H, W
    for name, (ci, co) in zip(names, lpips_ref.CHANNELS):
        per[name] = 2 * 9 * ci * co * h * w
        if name in ("conv1_2", "conv2_2", "conv3_3", "conv4_3"):
            h, w = h // 2, w // 2
    return per


def call_bench(a, dev, result):
    H, W = a.height, a.width
    w = lpips_cases.weights()
    g = torch.Generator().manual_seed(11)
    x = torch.rand(1, 3, H, W, generator=g).to(dev)
    y = (x + 0.1 * torch.randn(1, 3, H, W, generator=g).to(dev)).clamp(0, 1)
    crit = lpipsPyTorch.LPIPSLoss("vgg", weights=w)
    ref = torch_form(w, dev)
    leaf = x.clone().requires_grad_(True)

    def torch_call():
        # y does not require grad: its branch builds no graph and its activations are freed as they go
        return ref(leaf, y)
    cands = {"fused": lambda: crit(leaf, y), "torch": torch_call}
    peaks, values, grads = {}, {}, {}
    for name, fn in cands.items():
        leaf.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        v = fn()
        v.sum().backward()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated(dev) - base
        values[name], grads[name] = v.item(), leaf.grad.clone()
        del v
    result["peak_bytes"] = peaks
    gd = (grads["fused"].double() - grads["torch"].double()).norm() / grads["torch"].double().norm()
    result["agreement"] = {"value_relative_difference": abs(values["fused"] - values["torch"]) / abs(values["torch"]),
                           "gradient_relative_l2": float(gd), "gradient_finite": bool(torch.isfinite(grads["fused"]).all())}
    lib = fov3dgs_amd._native.load()
    result["fused_bytes"] = {"kept_state": int(lib.fr_lpips_keep_workspace_bytes(1, H, W)), "workspace": int(lib.fr_lpips_workspace_bytes(1, H, W)),
                             "kept_state_bound": 4 * (2 * 559_779_840 + 2 * 64 * 1080 * 1920) + (1 << 20) if (H, W) == (1080, 1920) else None}
    print(json.dumps({"peak_bytes": peaks, "agreement": result["agreement"], "fused_bytes": result["fused_bytes"]}), flush=True)
    del grads
    times = {k: {"forward": [], "backward": [], "both": []} for k in cands}
    for r in range(a.warmup + a.steps):
        for name, fn in cands.items():
            leaf.grad = None
            f, b = _timed(fn)
            if r >= a.warmup:
                times[name]["forward"].append(f)
                times[name]["backward"].append(b)
                times[name]["both"].append(f + b)
    result["call"] = {k: {part: _stats(v) for part, v in t.items()} for k, t in times.items()}
    fb, tb = result["call"]["fused"]["both"], result["call"]["torch"]["both"]
    result["call"]["fused_faster_beyond_spread"] = fb["p90_ms"] < tb["p10_ms"]
    result["call"]["torch_faster_beyond_spread"] = tb["p90_ms"] < fb["p10_ms"]
    print(json.dumps({"call": result["call"]}), flush=True)
    fwd = {n: [] for n in lpipsPyTorch.STAGES}
    bwd = {n: [] for n in lpipsPyTorch.BACKWARD_STAGES}
    for r in range(a.warmup + a.steps):
        sf, sb = crit.stage_times(x, y)
        if r >= a.warmup:
            for n, v in sf.items():
                fwd[n].append(v)
            for n, v in sb.items():
                bwd[n].append(v)
    flops = conv_flops(H, W)
    rows, mfma_ms, mfma_flop = {}, 0.0, 0
    for n in lpipsPyTorch.BACKWARD_STAGES:
        ms = statistics.median(bwd[n])
        rows[n] = {"ms": round(ms, 4), "gflop": round(flops[n] / 1e9, 1), "tflops": round(flops[n] / (ms * 1e-3) / 1e12, 2)}
        if n != "conv1_1":  # the first layer's backward is plain VALU
            mfma_ms, mfma_flop = mfma_ms + ms, mfma_flop + flops[n]
    result["backward_stages"] = rows
    result["backward_convolutions"] = {"flop": mfma_flop, "ms": round(mfma_ms, 3), "tflops": round(mfma_flop / (mfma_ms * 1e-3) / 1e12, 2),
                                       "peak": PEAK_F32_TFLOPS}
    result["forward_stages"] = {n: round(statistics.median(v), 4) for n, v in fwd.items()}
    print(json.dumps({"backward_convolutions": result["backward_convolutions"], "backward_stages": rows}), flush=True)


def train_bench(a, dev, result):
    """eff_finetune.py:107-147 with a perceptual term: wall time per iteration between device events around the whole step"""
    W, H = 1920, 1080
    w = lpips_cases.weights()
    cam, bg = syn.camera_ring(0, width=W, height=H).to(dev), torch.zeros(3, device=dev)
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
    base = syn.scene_bicycle_scale(P=a.P).to(dev)
    crit, ref = lpipsPyTorch.LPIPSLoss("vgg", weights=w), torch_form(w, dev)
    terms = {"l1_ssim_only": None, "fused_lpips": lambda img: crit(img[None], target[None]).sum(), "torch_lpips": lambda img: ref(img[None], target[None]).sum()}
    forms = {}
    for name in terms:
        m = clone_model(base)
        m.fuse_activations, m.row_sparse_grads = True, True
        forms[name] = (m, optim.Adam(optim.reference_param_groups(m, ARGS), lr=0.0, eps=1e-15, sparse="exact"), [])
    for it in range(a.warmup + a.train_steps):
        for name, term in terms.items():
            m, opt, ms = forms[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            image = render(cam, m, Pipe(), bg, cuda_type="pcheck_obb_sum")["render"]
            total = l1_ssim_loss(image, target, 0.2)
            if term is not None:
                total = total + a.lam * term(image)
            total.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                ms.append(e0.elapsed_time(e1))
    out = {name: _stats(ms) for name, (_, _, ms) in forms.items()}
    out["P"], out["lambda"] = a.P, a.lam
    out["fused_faster_beyond_spread"] = out["fused_lpips"]["p90_ms"] < out["torch_lpips"]["p10_ms"]
    out["torch_faster_beyond_spread"] = out["torch_lpips"]["p90_ms"] < out["fused_lpips"]["p10_ms"]
    result["train_step"] = out
    print(json.dumps({"train_step": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--train", action="store_true", help="also time the training step on --P Gaussians")
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--P", type=int, default=6_000_000)
    ap.add_argument("--lam", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_backward_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lpips_train_bench needs the MI355X"
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "size": [a.height, a.width], "N": 1, "steps": a.steps, "warmup": a.warmup,
              "weights": "tests/lpips_cases.weights (seeded)",
              "torch_form": "tests/lpips_ref.py's network, float32, F.conv2d / F.max_pool2d under torch.autograd, weights resident, no graph for the target"}
    call_bench(a, dev, result)
    if a.train:
        torch.cuda.empty_cache()
        train_bench(a, dev, result)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
