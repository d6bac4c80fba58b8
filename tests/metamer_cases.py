"""The cases of the metamer tests, read from tests/golden/ref_metamer.npz (+ ref_metamer_out.npz, ref_metamer_rt.npz; the filters from ref_hvs.npz),
with the float64 restatement (tests/metamer_ref.py) of each computed ONCE and shared.
Cases (tests/golden/make_metamer_golden.py), the smallest at which each part can go wrong:
  M0 32x64, 5 levels, 2 orientations: the lowpass residual is 2x4, the reflection halo of 2 sits on a 4x8 band
  M1 40x56, 3 levels, 6 orientations, linear mode, gaze (0.2, 0.7): sizes that are no powers of two
  M2 64x96, 5 levels, 6 orientations, alpha 0.5: the LOD reaches deep into the chains
  M3 64x64, alpha 0.001: LOD 0 everywhere, the variance exactly on its floor: the target's round trip plus noise * sqrt(1e-7)
  M4 64x96, 4 levels, gaze (1.2, -0.1) outside the picture, YCrCb input
  M5 96x160: every synthesis level down to 24x40 spans more than one 16x16 tile on both axes
The allowance of a comparison against the yardstick is FACTOR x the distance of the reference's own float32 run from it, as
stored in the fixture (the rule of the LPIPS tests)."""
import collections
import functools
import os

import numpy as np
import torch

from tests import hvs_cases as hc
from tests import hvs_ref, metamer_ref

NAMES = ["M0", "M1", "M2", "M3", "M4", "M5"]
FACTOR = 4.0
Case = collections.namedtuple("Case", "i name H W levels orientations alpha mode loss_type gaze width distance colorspace tgt img noise")


@functools.lru_cache(maxsize=None)
def golden():
    z = dict(np.load(os.path.join(hc.GOLDEN, "ref_metamer.npz")))
    z.update(np.load(os.path.join(hc.GOLDEN, "ref_metamer_out.npz")))
    z.update(np.load(os.path.join(hc.GOLDEN, "ref_metamer_rt.npz")))
    return z


def n_cases():
    return int(golden()["n"])


def case(i):
    z = golden()
    H, W, levels, no, alpha, quad, mse, gx, gy, width, dist, rgb = (float(v) for v in z[f"case_{i}"])
    return Case(i, NAMES[i], int(H), int(W), int(levels), int(no), alpha, "quadratic" if quad else "linear", "MSE" if mse else "L1",
                (gx, gy), width, dist, "RGB" if rgb else "YCrCb", hvs_ref.decode_u16(z[f"tgt_{i}"]), hvs_ref.decode_u16(z[f"img_{i}"]),
                z[f"noise_{i}"])


def restate(c, filters=None, drop=None, dtype=torch.float64):
    """the restatement's metamer of case c -> numpy [1,3,H,W]"""
    f = hvs_ref.filters_to(hc.filters(c.orientations) if filters is None else filters, dtype=dtype)
    with torch.no_grad():
        m = metamer_ref.gen_metamer(torch.tensor(c.tgt, dtype=dtype), torch.tensor(c.noise, dtype=dtype), f, gaze=c.gaze, alpha=c.alpha,
                                    real_image_width=c.width, real_viewing_distance=c.distance, n_pyramid_levels=c.levels, mode=c.mode,
                                    image_colorspace=c.colorspace, drop=drop)
    return m.numpy()


@functools.lru_cache(maxsize=None)
def yardstick(i):
    """float64 metamer of case i, computed once, never modified"""
    m = restate(case(i))
    m.setflags(write=False)
    return m


def restate_roundtrip(c, filters=None, drop=None):
    f = hvs_ref.filters_to(hc.filters(c.orientations) if filters is None else filters, dtype=torch.float64)
    with torch.no_grad():
        return metamer_ref.roundtrip(torch.tensor(c.tgt, dtype=torch.float64), f, c.levels, c.colorspace, drop=drop).numpy()


@functools.lru_cache(maxsize=None)
def yardstick_roundtrip(i):
    m = restate_roundtrip(case(i))
    m.setflags(write=False)
    return m


def distances(got, want):
    """(max |d|, relative L2) over every element"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = got - want
    return float(np.abs(d).max()), float(np.linalg.norm(d) / np.linalg.norm(want))


def allowance(i):
    """(max |d|, relative L2) a metamer of case i may lie from the yardstick: FACTOR x the reference's own float32 distance"""
    z = golden()
    return FACTOR * float(z[f"ref_max_abs_{i}"]), FACTOR * float(z[f"ref_rel_l2_{i}"])


def asymmetric_filters(n_orientations, seed=7):
    """a seeded filter set none of whose 5x5 blocks equals a mirror image of itself: the reference's own set plus uniform noise of
    half its largest coefficient (hc.asymmetry says by how much each block differs from its mirror images)"""
    rng = np.random.default_rng(seed)
    f = hc.filters(n_orientations)

    def bend(t):
        a = t.numpy().astype(np.float64)
        return torch.tensor((a + 0.5 * np.abs(a).max() * (rng.random(a.shape) - 0.5)).astype(np.float32))
    return {"l0": bend(f["l0"]), "h0": bend(f["h0"]), "b": [bend(b) for b in f["b"]]}
