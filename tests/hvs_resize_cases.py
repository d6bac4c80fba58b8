"""The cases of the resized HVS loss (MetamericLossUniform(..., resize=...)), read from tests/golden/ref_hvs_resize.npz
(tests/golden/make_hvs_resize_golden.py), with the yardstick of each computed ONCE and shared: F.interpolate(mode='bilinear',
align_corners=False) of both pictures in float64, then the float64 restatement tests/hvs_ref.hvs_loss, autograd to the SOURCE
picture. The allowance rule is tests/hvs_cases.allowance, unchanged. CASES lists R0 .. R4 and what each reaches.
Asymmetric cases run with the filter sets already stored in ref_hvs_edges.npz. That fixture holds sets for 1, 4, 6 and 8
orientations; a case with two orientations (R0, R1) takes l0, h0 and the first two band filters of the set of four."""
import collections
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import hvs_cases as hc
from tests import hvs_ref

#         source      resized    levels orientations pooling type asymmetric colour spaces
CASES = [((135, 16), (136, 16), 3, 2, 3, "L1", True, ("RGB",)),            # R0: the 1080 -> 1088 ratio at one eighth; width identity
         ((16, 135), (16, 136), 3, 2, 3, "MSE", True, ("RGB",)),           # R1: the same on the other axis
         ((21, 30), (24, 32), 3, 4, 5, "MSE", True, ("RGB", "YCrCb")),     # R2: both axes, different ratios; colour after the lerp
         ((33, 17), (64, 32), 5, 6, 9, "L1", False, ("RGB",)),             # R3: ratio ~1.9, tile seams, the halo through the lerp
         ((1, 5), (4, 8), 2, 1, 0.75, "L1", True, ("RGB",))]               # R4: one source row, a picture smaller than a tile
STORED_ASYMMETRIC = (1, 4, 6, 8)
ResizeCase = collections.namedtuple("ResizeCase", "i Hs Ws H W pooling levels orientations loss_type img tgt asymmetric spaces")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(hc.GOLDEN, "ref_hvs_resize.npz")))


def case(i):
    z = fixture()
    Hs, Ws, H, W, pool, levels, no, mse, asym, ycrcb = (float(v) for v in z[f"case_{i}"])
    pool = int(pool) if pool == int(pool) else pool
    return ResizeCase(i, int(Hs), int(Ws), int(H), int(W), pool, int(levels), int(no), "MSE" if mse else "L1",
                      hvs_ref.decode_u16(z[f"img_{i}"]), hvs_ref.decode_u16(z[f"tgt_{i}"]), bool(asym),
                      ("RGB", "YCrCb") if ycrcb else ("RGB",))


def asymmetric_filters(z, n_orientations):
    """the stored asymmetric set for n_orientations, or the first n_orientations bands of the next larger stored set"""
    have = min(n for n in STORED_ASYMMETRIC if n >= n_orientations)
    f = hvs_ref.filters_from_npz(z, have, prefix="afilters")
    return dict(f, b=f["b"][:n_orientations])


def filters_of(c):
    return asymmetric_filters(hc.edges(), c.orientations) if c.asymmetric else hc.filters(c.orientations)


def resize(x, H, W):
    """what the reference's scripts do before the loss (metric_mask_learn.py:222-223), in x's precision"""
    return F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)


def reference(i, colorspace="RGB"):
    """the reference's own float32 run stored in the fixture -> (loss, gradient with respect to the source picture)"""
    z, tag = fixture(), "" if colorspace == "RGB" else "_ycrcb"
    return float(z[f"loss_{i}{tag}"]), z[f"grad_{i}{tag}"]


@functools.lru_cache(maxsize=None)
def yardstick(i, colorspace="RGB"):
    """float64: resize, then the restatement, autograd to the source -> dict(loss, grad), numpy, never modified"""
    c = case(i)
    f = hvs_ref.filters_to(filters_of(c), dtype=torch.float64)
    img = torch.tensor(c.img, dtype=torch.float64, requires_grad=True)
    tgt = torch.tensor(c.tgt, dtype=torch.float64)
    loss = hvs_ref.hvs_loss(resize(img, c.H, c.W), resize(tgt, c.H, c.W), f, c.pooling, c.levels, c.loss_type, image_colorspace=colorspace)
    loss.backward()
    out = dict(loss=float(loss.detach()), grad=img.grad.numpy())
    out["grad"].setflags(write=False)
    return out
