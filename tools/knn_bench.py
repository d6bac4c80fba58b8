"""Timing of simple_knn.distCUDA2 (csrc/knn.hip) on the MI355X: one JSON line per case.

Cases: P in {100 k, 1 M, 6 M} x {uniform in a cube, COLMAP-like clustered (synthetic.points_colmap_like)} and the positions
of synthetic.scene_bicycle_scale (S-6M). Each case: warm-up calls, then --calls calls each between two device events on the
current stream; the median, min and max in ms. A last line gives t(6 M) / t(1 M) per cloud kind. Per-kernel times: run this
under `rocprofv3 --kernel-trace --stats` (e.g. with --calls 5) in a run of its own.

usage: python tools/knn_bench.py [--calls 25] [--warmup 3] [--out FILE] [--cases uniform,clustered,bicycle]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fov3dgs_amd  # noqa: E402,F401
from fov3dgs_amd import synthetic as syn  # noqa: E402
from fov3dgs_amd.simple_knn._C import distCUDA2  # noqa: E402


def time_case(x, calls, warmup):
    for _ in range(warmup):
        distCUDA2(x)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        distCUDA2(x)
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="uniform,clustered,bicycle")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "knn_bench needs the MI355X"
    kinds = a.cases.split(",")
    cases = []
    for P in (100_000, 1_000_000, 6_000_000):
        if "uniform" in kinds:
            g = torch.Generator().manual_seed(P)
            cases.append(("uniform", P, lambda P=P, g=g: torch.rand(P, 3, generator=g) * 20 - 10))
        if "clustered" in kinds:
            cases.append(("clustered", P, lambda P=P: syn.points_colmap_like(P)))
    if "bicycle" in kinds:
        cases.append(("bicycle_scale", 6_000_000, lambda: syn.scene_bicycle_scale().get_xyz))
    lines, med = [], {}
    for kind, P, make in cases:
        x = make().float().contiguous().to("cuda")
        t = time_case(x, a.calls, a.warmup)
        med[(kind, P)] = statistics.median(t)
        line = {"case": kind, "P": P, "median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4),
                "max_ms": round(max(t), 4), "calls": a.calls, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del x
    ratios = {k: round(med[(k, 6_000_000)] / med[(k, 1_000_000)], 3) for k in ("uniform", "clustered")
              if (k, 6_000_000) in med and (k, 1_000_000) in med}
    if ratios:
        line = {"scaling_t6M_over_t1M": ratios}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
