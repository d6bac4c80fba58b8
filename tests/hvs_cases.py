"""The cases of the HVS loss tests, read from tests/golden/ref_hvs.npz (+ ref_hvs_maps.npz), with the float64 restatement
(tests/hvs_ref.py) of each computed ONCE and shared, and the allowance rule of the comparisons.
A second fixture, tests/golden/ref_hvs_edges.npz (+ ref_hvs_edges_maps.npz, from make_hvs_edge_golden.py), holds the edge cases
E0 .. E7 (edge_case, edge_yardstick): E0, E1 pooling 5 and 3 over five levels, where the halved pooling size falls below 1 and the
pooled map is larger than the band (ph > h); E2 one orientation; E3 an 8x8 picture at pooling 0.75 with two levels; E4 tile
remainders 8, 8 and 12, 4; E5 pooled maps of one row, in RGB and in YCrCb; E6 a pooled map of one column; E7 six levels and eight
orientations. E2 .. E7 run with ASYMMETRIC filter sets stored in that fixture (filters_of), because the reference's own filters
equal their mirror images and so cannot tell a right tap order from a wrong one (asymmetry)."""
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


# ---------------------------------------------------------------- the second fixture: tests/golden/ref_hvs_edges.npz
EDGES = 8             # E0 .. E7 (tests/golden/make_hvs_edge_golden.py lists what each is for)
ASYMMETRY = 0.5       # what every 5x5 block of an asymmetric filter set differs from each of its mirror images by, of its maximum
EdgeCase = __import__("collections").namedtuple("EdgeCase", "i H W pooling levels orientations loss_type img tgt asymmetric")


@functools.lru_cache(maxsize=None)
def edges():
    z = dict(np.load(os.path.join(GOLDEN, "ref_hvs_edges.npz")))
    z.update(np.load(os.path.join(GOLDEN, "ref_hvs_edges_maps.npz")))
    return z


def edge_case(i):
    z = edges()
    H, W, pool, levels, no, mse, asym = (float(v) for v in z[f"case_{i}"])
    pool = int(pool) if pool == int(pool) else pool
    return EdgeCase(i, int(H), int(W), pool, int(levels), int(no), "MSE" if mse else "L1", hvs_ref.decode_u16(z[f"img_{i}"]),
                    hvs_ref.decode_u16(z[f"tgt_{i}"]), bool(asym))


def filters_of(c):
    """the filter set a case runs with: the reference's own (ref_hvs.npz), or the asymmetric set of ref_hvs_edges.npz"""
    if getattr(c, "asymmetric", False):
        return hvs_ref.filters_from_npz(edges(), c.orientations, prefix="afilters")
    return filters(c.orientations)


def evaluate(c, f64, colorspace="RGB"):
    """the float64 restatement of case c with the filter set f64 -> dict(loss, grad, maps), numpy"""
    img = torch.tensor(c.img, dtype=torch.float64, requires_grad=True)
    tgt = torch.tensor(c.tgt, dtype=torch.float64)
    loss, maps = hvs_ref.hvs_loss(img, tgt, f64, c.pooling, c.levels, c.loss_type, image_colorspace=colorspace, return_maps=True)
    loss.backward()
    return dict(loss=float(loss.detach()), grad=img.grad.numpy(), maps=[m.detach().numpy() for m in maps])


@functools.lru_cache(maxsize=None)
def edge_yardstick(i, colorspace="RGB"):
    """float64 restatement of edge case i, computed once, never modified"""
    c = edge_case(i)
    out = evaluate(c, hvs_ref.filters_to(filters_of(c), dtype=torch.float64), colorspace)
    for a in [out["grad"]] + out["maps"]:
        a.setflags(write=False)
    return out


def edge_map_indices(pooling, levels, orientations):
    """the four statistics the fixture stores as maps: the mean of h, the mean of the first band and the std of the second band
    (of the first where there is one) of the DEEPEST level that is pooled (1/p no integer), the lowpass residual"""
    k = [1.0 / (float(pooling) / 2 ** l) for l in range(levels - 1)]
    pooled = [l for l in range(levels - 1) if not (k[l] >= 1.0 and k[l].is_integer())]
    mid = 2 * (1 + orientations * pooled[-1])
    return [0, mid, mid + (3 if orientations > 1 else 1), hvs_ref.n_stats(levels, orientations) - 1]


def asymmetry(a):
    """of a 5x5 block: the least of max |a - T(a)| over its rotation by 180 degrees, its transpose and its two flips, and of
    max |a + rot180(a)|, over max |a|. 0 for a block that one of these mirror images (or minus its rotation) reproduces."""
    a = np.asarray(a, np.float64).reshape(5, 5)
    rot = a[::-1, ::-1]
    return float(min([np.abs(a - t).max() for t in (rot, a.T, a[:, ::-1], a[::-1])] + [np.abs(a + rot).max()]) / np.abs(a).max())


def distances(got, want):
    """the three figures of a comparison against the yardstick: relative L2, max |d| over max |want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = got - want
    return float(np.linalg.norm(d) / max(np.linalg.norm(want), 1e-300)), float(np.abs(d).max() / max(np.abs(want).max(), 1e-300))


def allowance(reference_figure):
    """what the library may differ by where the reference's own float32 run differs from the yardstick by reference_figure"""
    return max(FACTOR * reference_figure, FLOOR)
