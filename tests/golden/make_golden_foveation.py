"""Reference-written ground truth for the foveation SETTINGS (FoveationSettings / fr_foveation): the pooling-size map of the
reference's perception library for display geometries other than the one the rasterizer used to compile in.
    python tests/golden/make_golden_foveation.py PATH_TO_THE_REFERENCE_CHECKOUT
Imports metamer/odak_perception/foveation.py:94-146 make_pooling_size_map_pixels (runs on a CPU) and records, at 1280x720,
  ref_pooling_geometry.npz   the map sampled at the tile centres (bilinear, as make_golden_r3.py samples it) for three settings
                             (levels, max_pooling_size, real_image_width, real_viewing_distance), each with its gaze and alpha
Only data (inputs + expected outputs) is written; no reference source is copied.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# (levels, max_pooling_size, real_image_width, real_viewing_distance, gaze, alpha): the test converts the pooling sizes to levels
# with each setting's own step and cap; gaze and alpha are chosen so that every level 0 .. levels-1 occurs in the frame
CASES = ((6, 16.0, 1.6, 0.8, (0.3, 0.6), 0.05),
         (3, 9.0, 2.4, 1.5, (0.62, 0.35), 0.05),
         (8, 25.0, 1.2, 1.0, (0.2, 0.7), 0.12))


def main(ref):
    sys.path.insert(0, os.path.join(ref, "metamer"))
    from odak_perception.foveation import make_pooling_size_map_pixels

    W, H = 1280, 720
    twn, thn = (W + 15) // 16, (H + 15) // 16
    tx, ty = np.meshgrid(np.arange(twn), np.arange(thn))
    u = (16 * tx + 8) / W * (W - 1)
    v = (16 * ty + 8) / H * (H - 1)
    u0 = np.clip(np.floor(u).astype(int), 0, W - 2)
    v0 = np.clip(np.floor(v).astype(int), 0, H - 2)
    fu, fv = u - u0, v - v0
    out = {"size": np.array([W, H]), "inside": (16 * tx + 8 <= W - 1) & (16 * ty + 8 <= H - 1),
           "cases": np.array([[c[0], c[1], c[2], c[3], c[4][0], c[4][1], c[5]] for c in CASES], np.float64)}
    for ci, (_, _, riw, rvd, gaze, alpha) in enumerate(CASES):
        m = make_pooling_size_map_pixels(list(gaze), (H, W), alpha=alpha, real_image_width=riw, real_viewing_distance=rvd).double().numpy()
        out[f"ps{ci}"] = ((1 - fu) * (1 - fv) * m[v0, u0] + fu * (1 - fv) * m[v0, u0 + 1] + (1 - fu) * fv * m[v0 + 1, u0]
                          + fu * fv * m[v0 + 1, u0 + 1]).astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "ref_pooling_geometry.npz"), **out)
    print("ref_pooling_geometry.npz written to", HERE)


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "metamer")):
        sys.exit("usage: make_golden_foveation.py PATH_TO_THE_REFERENCE_CHECKOUT (these vectors need the reference's metamer/ package)")
    main(sys.argv[1])
