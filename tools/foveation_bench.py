#!/usr/bin/env python3
"""Foveated frames with run-time foveation settings on the S-6M scene (developer tool; for information, no threshold).
usage: python tools/foveation_bench.py [out.json] [points=6000000] [repeats=5]
For L = 3, 4, 6 and 8 layers (the cloud composed into L equally likely layers; L = 4 with the default settings spelled out, i.e.
through the entry point that takes them) at 1920x1080: serial frames/s over the nine gazes of the FPS protocol
(render_compose_gazes_fps.py:26) -- every frame on the caller's stream, events around the nine frames, median of `repeats` -- and
the per-stage kernel times (mean over the same gazes). "none" is the call without settings on the 4-layer model."""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fov3dgs_amd  # noqa
from fov3dgs_amd import _native, rasterizer as rz, synthetic as syn
from fov3dgs_amd.profiling import StageTimer

out_path = sys.argv[1] if len(sys.argv) > 1 else None
P = int(sys.argv[2]) if len(sys.argv) > 2 else 6_000_000
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda", 0)
cloud_cpu = syn.scene_bicycle_scale(P=P, seed=1)
cloud = cloud_cpu.to(dev)
cam = syn.camera_ring(0, 8).to(dev)
W, H = cam.image_width, cam.image_height
with torch.no_grad():
    xyz, sc, rot = cloud.get_xyz, cloud.get_scaling.contiguous(), cloud.get_rotation.contiguous()
    rest = cloud.get_rest_features.contiguous()
rs = rz.GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3, device=dev),
                                      1.0, cam.world_view_transform, cam.full_proj_transform, 3, cam.camera_center, False, False)
vid = _native.VARIANT_FOV_PCHECK_OBB
E = torch.Tensor([])
GAZES = [(0.25 * i, 0.25 * j) for i in range(1, 4) for j in range(1, 4)]
results = {"points": P, "size": [W, H], "gazes": GAZES, "repeats": repeats, "cases": {}}
for name, L, settings in (("none", 4, None), ("L4", 4, rz.FoveationSettings()), ("L3", 3, rz.FoveationSettings(levels=3)),
                          ("L6", 6, rz.FoveationSettings(levels=6)), ("L8", 8, rz.FoveationSettings(levels=8))):
    hl, dcs, op = (t.to(dev) for t in syn.foveation_layers(cloud_cpu, seed=2, fractions=(1.0 / L,) * L if L != 4 else syn.LEVEL_FRACTIONS))

    def frame(g):
        return rz._forward_native(vid, rs, xyz, rest, E, op, sc, rot, E, dcs, hl, g, 0.05, persistent=True, foveation=settings)

    with torch.no_grad(), rz.serial_frames():
        for g in GAZES:
            r = frame(g)
        torch.cuda.synchronize()
        fps = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for g in GAZES:
                r = frame(g)
            e1.record()
            torch.cuda.synchronize()
            fps.append(1000.0 * len(GAZES) / e0.elapsed_time(e1))
        t = StageTimer(len(GAZES))
        with t:
            for g in GAZES:
                r = frame(g)
        torch.cuda.synchronize()
    ms = t.stage_ms()
    stages = {k: round(float(np.mean([m[k] for m in ms])), 4) for k in _native.STAGES}
    results["cases"][name] = {"levels": L, "settings": None if settings is None else list(settings), "serial_fps_median": round(float(np.median(fps)), 1),
                              "serial_fps": [round(f, 1) for f in fps], "stages_ms": stages, "instances_last_gaze": int(r[0])}
    print(name, results["cases"][name], flush=True)
    del hl, dcs, op
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
print(json.dumps(results))
