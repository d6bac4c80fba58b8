"""The cases of the HVS loss tests, read from tests/golden/ref_hvs.npz (+ ref_hvs_maps.npz), with the float64 restatement
(tests/hvs_ref.py) of each computed ONCE and shared, and the allowance rule of the comparisons."""
import functools
import os

import numpy as np
import torch

from tests import hvs_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS32 = float(np.finfo(np.float32).eps)
FLOOR = 16 * EPS32   # the reference can land on the float64 value by accident in a small case
FACTOR = 3.0         # the kernels add 25 taps and the pooling windows in another order than torch


@functools.lru_cache(maxsize=None)
def golden():
    z = dict(np.load(os.path.join(GOLDEN, "ref_hvs.npz")))
    z.update(np.load(os.path.join(GOLDEN, "ref_hvs_maps.npz")))
    return z


def n_cases():
    return int(golden()["n"])


def filters(n_orientations):
    return hvs_ref.filters_from_npz(golden(), n_orientations)


Case = __import__("collections").namedtuple("Case", "i H W pooling levels orientations loss_type img tgt")


def case(i):
    z = golden()
    H, W, pool, levels, no, mse = (int(v) for v in z[f"case_{i}"])
    return Case(i, H, W, pool, levels, no, "MSE" if mse else "L1", hvs_ref.decode_u16(z[f"img_{i}"]), hvs_ref.decode_u16(z[f"tgt_{i}"]))


@functools.lru_cache(maxsize=None)
def yardstick(i, colorspace="RGB"):
    """float64 restatement of case i -> dict(loss, grad, maps = the list of statistics), numpy, never modified"""
    c = case(i)
    f = hvs_ref.filters_to(filters(c.orientations), dtype=torch.float64)
    img = torch.tensor(c.img, dtype=torch.float64, requires_grad=True)
    tgt = torch.tensor(c.tgt, dtype=torch.float64)
    loss, maps = hvs_ref.hvs_loss(img, tgt, f, c.pooling, c.levels, c.loss_type, image_colorspace=colorspace, return_maps=True)
    loss.backward()
    out = dict(loss=float(loss.detach()), grad=img.grad.numpy(), maps=[m.detach().numpy() for m in maps])
    for a in [out["grad"]] + out["maps"]:
        a.setflags(write=False)
    return out


def distances(got, want):
    """the three figures of a comparison against the yardstick: relative L2, max |d| over max |want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = got - want
    return float(np.linalg.norm(d) / max(np.linalg.norm(want), 1e-300)), float(np.abs(d).max() / max(np.abs(want).max(), 1e-300))


def allowance(reference_figure):
    """what the library may differ by where the reference's own float32 run differs from the yardstick by reference_figure"""
    return max(FACTOR * reference_figure, FLOOR)
