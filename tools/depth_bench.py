#!/usr/bin/env python3
"""What the depth / coverage outputs (fr_forward_aux; want_depth=True) cost a frame, on the S-6M scene at 1920x1080 (developer tool;
for information, no threshold).
usage: python tools/depth_bench.py [out.json=profiles/depth_bench.json] [points=6000000] [rounds=9]
Compared, each as ms per frame over the nine gazes of the FPS protocol (render_compose_gazes_fps.py:26), events on the caller's stream
around the nine frames, `rounds` alternating rounds (without, with, with, without, ...), median and p10-p90 over the rounds:
  fov_serial       the foveated frame without and with the outputs, every frame on the caller's stream (serial_frames)
  fov_overlapped   the same through the overlapped path (the default of inference calls)
  pcheck_obb       the plain inference renderer without and with them (its calls are not overlapped)
and the per-stage kernel times of the serial foveated frame in both kinds (mean over the gazes): `clear_ms` is the difference of the
tile_levels stage -- the tile-wise clear of the two planes' two-level tiles runs there, behind k_tile_levels -- and `blend_ms` the
difference of the render stage (the blend's depth instantiation)."""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fov3dgs_amd  # noqa
from fov3dgs_amd import _native, rasterizer as rz, synthetic as syn
from fov3dgs_amd.profiling import StageTimer

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "depth_bench.json")
P = int(sys.argv[2]) if len(sys.argv) > 2 else 6_000_000
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 9
dev = torch.device("cuda", 0)
cloud_cpu = syn.scene_bicycle_scale(P=P, seed=1)
cloud = cloud_cpu.to(dev)
cam = syn.camera_ring(0, 8).to(dev)
W, H = cam.image_width, cam.image_height
with torch.no_grad():
    xyz, sc, rot = cloud.get_xyz, cloud.get_scaling.contiguous(), cloud.get_rotation.contiguous()
    rest, feats, op1 = cloud.get_rest_features.contiguous(), cloud.get_features.contiguous(), cloud.get_opacity.contiguous()
hl, dcs, op = (t.to(dev) for t in syn.foveation_layers(cloud_cpu, seed=2))
rs = rz.GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3, device=dev),
                                      1.0, cam.world_view_transform, cam.full_proj_transform, 3, cam.camera_center, False, False)
E = torch.Tensor([])
GAZES = [(0.25 * i, 0.25 * j) for i in range(1, 4) for j in range(1, 4)]


def fov_frame(g, want):
    return rz._forward_native(_native.VARIANT_FOV_PCHECK_OBB, rs, xyz, rest, E, op, sc, rot, E, dcs, hl, g, 0.05, persistent=True,
                              **({"want_depth": True} if want else {}))


def plain_frame(g, want):
    return rz._forward_begin(_native.VARIANT_PCHECK_OBB, rs, xyz, feats, E, op1, sc, rot, E, persistent=True,
                             **({"want_depth": True} if want else {})).finish()


def nine(frame, want):
    """ms per frame of the nine gazes"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for g in GAZES:
        r = frame(g, want)
    e1.record()
    torch.cuda.synchronize()
    del r
    return e0.elapsed_time(e1) / len(GAZES)


def summary(xs):
    return {"median_ms": round(float(np.median(xs)), 4), "p10_ms": round(float(np.quantile(xs, 0.1)), 4), "p90_ms": round(float(np.quantile(xs, 0.9)), 4),
            "rounds_ms": [round(float(x), 4) for x in xs]}


def compare(frame):
    for want in (False, True, False, True):   # (warm-up: workspaces, argument structs and clocks of both kinds)
        nine(frame, want)
    ms = {False: [], True: []}
    for r in range(rounds):
        for want in ((False, True) if r % 2 == 0 else (True, False)):
            ms[want].append(nine(frame, want))
    out = {"without": summary(ms[False]), "with": summary(ms[True])}
    out["added_ms_median"] = round(out["with"]["median_ms"] - out["without"]["median_ms"], 4)
    return out


results = {"points": P, "size": [W, H], "gazes": GAZES, "rounds": rounds,
           "clear": "k_aux_clear: one wave per two-level tile of the two planes, behind k_tile_levels, launched only in calls that ask for the outputs"}
with torch.no_grad():
    with rz.serial_frames():
        results["fov_serial"] = compare(fov_frame)
        stages = {}
        for want in (False, True):
            t = StageTimer(len(GAZES))
            with t:
                for g in GAZES:
                    fov_frame(g, want)
            torch.cuda.synchronize()
            ms = t.stage_ms()
            stages["with" if want else "without"] = {k: round(float(np.mean([m[k] for m in ms])), 4) for k in _native.STAGES}
        results["fov_serial_stages_ms"] = stages
        results["clear_ms"] = round(stages["with"]["tile_levels"] - stages["without"]["tile_levels"], 4)
        results["blend_ms"] = round(stages["with"]["render"] - stages["without"]["render"], 4)
    print("fov_serial", results["fov_serial"], results["fov_serial_stages_ms"], flush=True)
    results["fov_overlapped"] = compare(fov_frame)
    print("fov_overlapped", results["fov_overlapped"], flush=True)
    results["pcheck_obb"] = compare(plain_frame)
    print("pcheck_obb", results["pcheck_obb"], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(results, f, indent=1)
print(json.dumps(results))
