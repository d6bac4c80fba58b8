#!/usr/bin/env python
"""LPIPS (VGG16) of one 1080 x 1920 picture pair, N = 1, seeded random weights (tests/lpips_cases.weights): the fused call
(fov3dgs_amd.lpipsPyTorch.LPIPS, csrc/lpips.hip) against the same network written with F.conv2d, F.max_pool2d and the torch head
(tests/lpips_ref.py in float32 on the GPU, the weights resident there: the reference's per-call rebuild and download are NOT
charged to it). The two candidates alternate call by call, each call between two device events; --warmup rounds, then --steps
timed rounds; median, p10-p90, min and max in ms. Beside them:
  per_layer       the fused call's 18 stages (fr_lpips_args.stage_events) and the torch form's layers, each between two events,
                  medians over the timed rounds of a separate pass;
  trunk_tflops    the 13 convolutions' 2 K M N operations of both pictures over the sum of their median times, against the 157.3
                  TFLOP/s of the f32 matrix cores;
  peak_bytes      torch.cuda.max_memory_allocated over one call of each form, above what is resident before it (pictures, weights;
                  the fused form's workspace is counted: it is allocated at the first call and kept).
Writes profiles/lpips_bench.json."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fov3dgs_amd  # noqa: E402,F401
from fov3dgs_amd import lpipsPyTorch  # noqa: E402
from tests import lpips_cases, lpips_ref  # noqa: E402

PEAK_F32_TFLOPS = 157.3


def _stats(ms):
    ms = sorted(ms)
    q = statistics.quantiles(ms, n=10) if len(ms) >= 2 else [ms[0]] * 9
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
            "p10_ms": round(q[0], 4), "p90_ms": round(q[-1], 4), "n": len(ms)}


def _torch_layers(w, dev):
    """[(name, fn)] over vgg16().features as tests/lpips_ref.features walks it; the weights on the device"""
    feats = {k: v.to(dev) for k, v in w["features"].items()}
    names = iter(n for n in lpipsPyTorch.STAGES if n.startswith("conv"))
    layers, idx = [], 0
    for v in lpips_ref.CFG:
        if v == "M":
            layers.append(("pool", lambda t: F.max_pool2d(t, 2, 2)))
            idx += 1
        else:
            wt, b = feats[f"{idx}.weight"], feats[f"{idx}.bias"]
            layers.append((next(names), lambda t, wt=wt, b=b: F.relu(F.conv2d(t, wt, b, padding=1))))
            idx += 2
    return layers


def torch_form(w, dev):
    layers = _torch_layers(w, dev)
    lin = [w["lin"][f"lin{k}.model.1.weight"].to(dev) for k in range(5)]
    mean = torch.tensor(lpips_ref.MEAN, device=dev)[None, :, None, None]
    std = torch.tensor(lpips_ref.STD, device=dev)[None, :, None, None]
    taps_after = {"conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3"}

    def feats(x, events=None):
        x, out = (x - mean) / std, []
        for name, fn in layers[:-1]:  # the fifth pool is never reached (networks.py:62-63)
            if events is not None:
                events.append((name, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                events[-1][1].record()
            x = fn(x)
            if events is not None:
                events[-1][2].record()
            if name in taps_after:
                out.append(lpips_ref.normalize_activation(x))
        return out

    def run(x, y, events=None):
        fx, fy = feats(x, events), feats(y, events)
        res = [F.conv2d((a - b) ** 2, l).mean((2, 3), True) for a, b, l in zip(fx, fy, lin)]
        return torch.sum(torch.cat(res, 0), 0, True)
    return run


def trunk_flops(H, W):
    total, per, h, w = 0, {}, H, W
    names = [n for n in lpipsPyTorch.STAGES if n.startswith("conv")]
    pools_after = {"conv1_2", "conv2_2", "conv3_3", "conv4_3"}
    for name, (ci, co) in zip(names, lpips_ref.CHANNELS):
        per[name] = 2 * 2 * 9 * ci * co * h * w  # both pictures
        total += per[name]
        if name in pools_after:
            h, w = h // 2, w // 2
    return total, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lpips_bench needs the MI355X"
    dev = torch.device("cuda:0")
    H, W = a.height, a.width
    w = lpips_cases.weights()
    g = torch.Generator().manual_seed(11)
    x = torch.rand(1, 3, H, W, generator=g).to(dev)
    y = (x + 0.1 * torch.randn(1, 3, H, W, generator=g).to(dev)).clamp(0, 1)
    crit = lpipsPyTorch.LPIPS("vgg", weights=w)
    ref = torch_form(w, dev)
    cands = {"fused": lambda: crit(x, y), "torch": lambda: ref(x, y)}
    result = {"device": torch.cuda.get_device_name(0), "size": [H, W], "N": 1, "steps": a.steps, "warmup": a.warmup,
              "weights": "tests/lpips_cases.weights (seeded)", "torch_form": "tests/lpips_ref.py's network, float32, F.conv2d / F.max_pool2d, weights resident"}
    # peak memory of one call each, in a fresh allocator state
    peaks, values = {}, {}
    with torch.no_grad():
        for name, fn in cands.items():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            values[name] = fn().item()
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated(dev) - base
        result["peak_bytes"] = peaks
        result["value"] = dict(values, relative_difference=abs(values["fused"] - values["torch"]) / abs(values["torch"]))
        print(json.dumps({"peak_bytes": peaks, "value": result["value"]}), flush=True)
        times = {k: [] for k in cands}
        for r in range(a.warmup + a.steps):
            for name, fn in cands.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    times[name].append(e0.elapsed_time(e1))
        result["call"] = {k: _stats(v) for k, v in times.items()}
        result["call"]["fused_faster_beyond_spread"] = result["call"]["fused"]["p90_ms"] < result["call"]["torch"]["p10_ms"]
        result["call"]["torch_faster_beyond_spread"] = result["call"]["torch"]["p90_ms"] < result["call"]["fused"]["p10_ms"]
        print(json.dumps({"call": result["call"]}), flush=True)
        # per layer, a pass of its own (the events between the layers cost a little)
        fused_l = {n: [] for n in lpipsPyTorch.STAGES}
        torch_l = {}
        for r in range(a.warmup + a.steps):
            st = crit.stage_times(x, y)
            ev = []
            ref(x, y, ev)
            torch.cuda.synchronize()
            if r >= a.warmup:
                for n, v in st.items():
                    fused_l[n].append(v)
                per = {}
                for n, e0, e1 in ev:  # x's pass and y's pass of a layer add up
                    per[n] = per.get(n, 0.0) + e0.elapsed_time(e1)
                for n, v in per.items():
                    torch_l.setdefault(n, []).append(v)
    flops, per_flops = trunk_flops(H, W)
    layer = {}
    for n in lpipsPyTorch.STAGES:
        row = {"fused_ms": round(statistics.median(fused_l[n]), 4)}
        if n in torch_l:
            row["torch_ms"] = round(statistics.median(torch_l[n]), 4)
            row["gflop"] = round(per_flops[n] / 1e9, 1)
            row["fused_tflops"] = round(per_flops[n] / (row["fused_ms"] * 1e-3) / 1e12, 2)
            row["torch_tflops"] = round(per_flops[n] / (row["torch_ms"] * 1e-3) / 1e12, 2)
        layer[n] = row
    layer["pools (torch form only)"] = {"torch_ms": round(statistics.median(torch_l["pool"]), 4)}
    result["per_layer"] = layer
    conv_names = [n for n in lpipsPyTorch.STAGES if n.startswith("conv")]
    fused_trunk = sum(layer[n]["fused_ms"] for n in conv_names)
    torch_trunk = sum(layer[n]["torch_ms"] for n in conv_names)
    result["trunk_tflops"] = {"flop": flops, "peak": PEAK_F32_TFLOPS,
                              "fused": round(flops / (fused_trunk * 1e-3) / 1e12, 2), "fused_trunk_ms": round(fused_trunk, 3),
                              "torch": round(flops / (torch_trunk * 1e-3) / 1e12, 2), "torch_trunk_ms": round(torch_trunk, 3)}
    result["fused_workspace_bytes"] = int(fov3dgs_amd._native.load().fr_lpips_workspace_bytes(1, H, W))
    print(json.dumps({"trunk_tflops": result["trunk_tflops"]}), flush=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
