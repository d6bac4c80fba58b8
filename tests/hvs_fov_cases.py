"""The cases of the foveated HVS loss tests, read from tests/golden/ref_hvs_fov.npz (+ ref_hvs_fov_maps.npz; the filters from
ref_hvs.npz), with the float64 restatement (tests/hvs_fov_ref.py) of each computed ONCE and shared. The allowance rule of the
comparisons is tests/hvs_cases.py's, unchanged."""
import collections
import functools
import os

import numpy as np
import torch

from tests import hvs_cases as hc
from tests import hvs_fov_ref, hvs_ref

NAMES = ["F0", "F1", "F2", "F3", "F4", "F5/L1", "F5/MSE", "F6"]
Case = collections.namedtuple("Case", "i name H W levels orientations alpha mode loss_type gaze width distance colorspace img tgt")


@functools.lru_cache(maxsize=None)
def golden():
    z = dict(np.load(os.path.join(hc.GOLDEN, "ref_hvs_fov.npz")))
    z.update(np.load(os.path.join(hc.GOLDEN, "ref_hvs_fov_maps.npz")))
    return z


def n_cases():
    return int(golden()["n"])


def case(i):
    z = golden()
    H, W, levels, no, alpha, quad, mse, gx, gy, width, dist, rgb = (float(v) for v in z[f"case_{i}"])
    return Case(i, NAMES[i], int(H), int(W), int(levels), int(no), alpha, "quadratic" if quad else "linear", "MSE" if mse else "L1",
                (gx, gy), width, dist, "RGB" if rgb else "YCrCb", hvs_ref.decode_u16(z[f"img_{i}"]), hvs_ref.decode_u16(z[f"tgt_{i}"]))


def restate(c, dtype, img=None, tgt=None, colorspace=None, gaze=None):
    """the restatement of case c in `dtype` on the CPU -> dict(loss, grad, maps, lods), numpy"""
    f = hvs_ref.filters_to(hc.filters(c.orientations), dtype=dtype)
    x = torch.tensor(c.img if img is None else img, dtype=dtype, requires_grad=True)
    t = torch.tensor(c.tgt if tgt is None else tgt, dtype=dtype)
    g = c.gaze if gaze is None else gaze
    lods = hvs_fov_ref.lod_maps(g, x.size(2), x.size(3), c.levels, c.alpha, c.width, c.distance, c.mode, dtype)
    loss, maps = hvs_fov_ref.fov_loss(x, t, f, n_pyramid_levels=c.levels, loss_type=c.loss_type,
                                      image_colorspace=c.colorspace if colorspace is None else colorspace, return_maps=True, lods=lods)
    loss.backward()
    return dict(loss=float(loss.detach()), grad=x.grad.numpy(), maps=[m.detach().numpy() for m in maps], lods=[m.numpy() for m in lods])


@functools.lru_cache(maxsize=None)
def yardstick(i):
    """float64 restatement of case i, computed once, never modified"""
    out = restate(case(i), torch.float64)
    for a in [out["grad"]] + out["maps"] + out["lods"]:
        a.setflags(write=False)
    return out


def pictures(H, W, seed, amp):
    """the fixtures' picture pair as 16-bit arrays [1,3,H,W] (image, target): smooth colour plus uniform noise of width `amp`,
    clipped to [0, 1] (tests/golden/make_hvs_golden.pictures with the noise width as a parameter); the generators draw their
    pictures here, and a fixture that stores only (seed, amp) gets the same ones back"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 3, H), np.linspace(0, 2, W), indexing="ij")
    base = np.stack([0.5 + 0.2 * np.sin(xx * (c + 1) + yy) * np.cos(yy * 1.7 - c) for c in range(3)])
    tgt = np.clip(base + amp * (rng.random(base.shape) - 0.5), 0, 1)
    img = np.clip(tgt + 0.05 * rng.standard_normal(base.shape), 0, 1)
    return np.round(img * 65535).astype(np.uint16)[None], np.round(tgt * 65535).astype(np.uint16)[None]


def max_abs(got, want):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())
