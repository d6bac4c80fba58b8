"""The CPU oracle on frames of a tile or two, where tile centres lie outside the frame: a level gradient of two levels per tile gives
tile_min <= -1 (17 x 15: -1.95), and on 1 x 1, 2 x 2 and 3 x 40 every tile level is NaN.

The defect this file pins: for a tile with tile_min <= -1 the oracle followed the reference literally and indexed shs_dcs /
fov_colors / opacities at level int(tile_min) = -1 -- the previous Gaussian's level 3, and for Gaussian 0 twelve bytes in FRONT of
the arrays: compute_fov_colors wrote there, and glibc aborted the process at some later free ("free(): invalid next size",
"munmap_chunk(): invalid pointer"), typically while a later, smaller frame was rendered -- frames with a NaN level were where it
surfaced, not where it was written (they keep no Gaussian and index nothing). The reference's own indexing is undefined there; the
oracle, the numpy derivation and the HIP library now take level 0 for a negative tile_min (such a tile never blends).

  * oracle/sanitize_driver.c: the oracle's foveated variants under -fsanitize=address,undefined as a stand-alone program, one and 64
    Gaussians, those frames: must run clean.
  * the sequence 16 x 16, 17 x 15, 1 x 1, 2 x 2, 3 x 40 in one process: zero instances on the last three, and the independent numpy
    derivation (tests/numpy_fov_rasterizer.py) gives the same lists, level ranges and frame on all five."""
import os
import subprocess

import numpy as np

from oracle import oracle as orc
from tests import fov_backward_scenes as fs
from tests import numpy_fov_rasterizer as npr
from tests.checks import check_image
from tests.helpers import ROOT

DRIVER = os.path.join(ROOT, "oracle", "sanitize_driver.c")
FRAMES = ((16, 16), (17, 15), (1, 1), (2, 2), (3, 40))


def test_the_oracle_runs_clean_under_the_sanitizers(tmp_path):
    exe = tmp_path / "orc_san"
    subprocess.check_call(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fopenmp", "-ffp-contract=off",
                           "-o", str(exe), DRIVER, "-lm"])
    # (a stand-alone program with the sanitizer runtimes linked in statically: it runs in whatever environment the suite runs in)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "sanitize_driver: done" in res.stdout and "ERROR" not in res.stderr
    assert "frame 3x40: instances 0, visible 0, tiles with a NaN level 3" in res.stdout
    assert "variant 3 P 64 frame 17x15: instances 64" in res.stdout


def test_tiny_frames_in_one_process_match_the_derivation():
    for W, H in FRAMES:
        scene, cam = fs._faint_cloud((0.4, 0.55), width=W, height=H)
        want = orc.forward("fov_pcheck_obb", scene, cam)
        got = npr.rasterize("fov_pcheck_obb", scene, cam, np.float32)
        nan_tiles = int(np.isnan(want["tile_min"]).sum())
        print(f"{W} x {H}: instances {want['num_rendered']}, tile_min {want['tile_min']}, tiles with a NaN level {nan_tiles}")
        if (W, H) in FRAMES[2:]:
            assert want["num_rendered"] == 0 and not (want["radii"] > 0).any() and nan_tiles == len(want["tile_min"])
        else:
            assert want["num_rendered"] > 2000
        if (W, H) == (17, 15):
            assert want["tile_min"][0] <= -1.0 and int(want["ranges"][0, 1]) - int(want["ranges"][0, 0]) > 2000
        np.testing.assert_array_equal(got["radii"], want["radii"])
        np.testing.assert_array_equal(got["ranges"], want["ranges"])
        np.testing.assert_array_equal(got["point_list"], want["point_list"])
        vis = want["radii"] > 0
        np.testing.assert_array_equal(got["level_ranges"][vis], want["level_ranges"][vis])
        assert (want["level_ranges"][vis] >= 0).all() and (want["level_ranges"][vis] <= 3).all()
        check_image(got["color"], want["color"], name=f"{W} x {H} derivation vs oracle")
        assert np.isfinite(want["color"]).all()
