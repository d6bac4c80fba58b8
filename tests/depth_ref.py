"""Reference of the inference renderers' per-pixel depth and coverage outputs (include/fovraster.h: fr_forward_aux).

The quantities are the blend's own, so the reference is the blend's restatement the foveated backward tests already use:
tests/fov_backward_ref.FovBackwardRef, whose tiles hold the frozen fp32 decisions -- which (pixel, state, Gaussian) pairs are
accumulated, where a state stops, which state-1 pixels start finished -- and the states' shares of their pixels. Per state and pixel,
with alpha_j = min(0.99, o_j G_j) where the pair is accumulated (else 0), T_j = prod_{i<j} (1 - alpha_i) and z_j the Gaussian's
view-space depth (the forward dict's "depths"):

    depth    = sum over states of share * sum_j alpha_j T_j z_j
    coverage = sum over states of share * (1 - T_end)

in the dtype asked for: float64 is the reference, float32 the same arithmetic for a measure of the rounding. The background takes no
part; a pixel no Gaussian reaches holds 0 in both.

pcheck_obb has one state per pixel and no levels: plain_ref() restates its forward dict (oracle.forward("pcheck_obb", ...): lists,
means2D, conic, the scene's opacities) as a one-level frame whose every tile is single-level, and the same class does the rest.
"""
import numpy as np

from tests.fov_backward_ref import BLOCK, FovBackwardRef


def outputs(ref, depths, dtype=np.float64):
    """-> (depth [H,W], coverage [H,W]) of the frame `ref` (a FovBackwardRef) restates, in `dtype`."""
    F = np.dtype(dtype).type
    z = np.asarray(depths, F).reshape(-1)
    depth, cover = np.zeros((ref.H, ref.W), F), np.zeros((ref.H, ref.W), F)
    for tl in ref.tiles:
        G = ref._G(tl, F)
        d, c = np.zeros(256, F), np.zeros(256, F)
        for st in tl["states"]:
            alpha, _, Tb, Tfin = ref._state(tl, st, G, ref.opac, F)
            share = ref._wgt(st, F)
            d += share * ((alpha * Tb).T @ z[tl["g"]])
            c += share * (F(1) - Tfin)
        ins = tl["inside"]
        depth[tl["Y"][ins], tl["X"][ins]] = d[ins]
        cover[tl["Y"][ins], tl["X"][ins]] = c[ins]
    return depth, cover


def zmax_of(fwd):
    """the largest view-space depth among the Gaussians of the frame's tile lists: the scale depth is judged in"""
    pl = np.asarray(fwd["point_list"]).astype(np.int64)
    assert pl.size > 0
    return float(np.asarray(fwd["depths"], np.float64)[pl].max())


def two_level_tiles(ref):
    return sum(1 for tl in ref.tiles if tl["blend"])


def plain_ref(fwd, scene, cam):
    """The FovBackwardRef of a pcheck_obb frame: one level, every tile single-level, the Gaussian's own opacity and colour."""
    P = int(np.asarray(scene["means3D"]).shape[0])
    W, H = int(cam["image_width"]), int(cam["image_height"])
    T = ((W + BLOCK - 1) // BLOCK) * ((H + BLOCK - 1) // BLOCK)
    zeros = np.zeros(T, np.float32)
    f = dict(means2D=fwd["means2D"], conic=fwd["conic"], ranges=fwd["ranges"], point_list=fwd["point_list"], tile_min=zeros, tile_gx=zeros,
             tile_gy=zeros, tile_blend=np.zeros(T, np.uint8), fov_colors=np.asarray(fwd["rgb"], np.float32).reshape(P, 1, 3))
    s = dict(means3D=scene["means3D"], opacities=np.asarray(scene["opacities"], np.float32).reshape(P, 1), shs_dcs=np.zeros((P, 1, 3), np.float32),
             highest_levels=np.zeros(P, np.float32))
    return FovBackwardRef(f, s, cam, levels=1)


SH_C0 = 0.28209479177387814


def depth_as_colour(depths, zmax):
    """[P,3] float32: the colour (z / zmax, 1, 0) per Gaussian (negative where the Gaussian lies behind the camera: clamped by the blend's
    max(0, .), and such a Gaussian is in no list)"""
    P = np.asarray(depths).size
    c = np.zeros((P, 3), np.float32)
    c[:, 0] = (np.asarray(depths, np.float64).reshape(-1) / zmax).astype(np.float32)
    c[:, 1] = 1.0
    return c


def dc_of_colour(c):
    """the DC coefficient whose SH colour (rest SH zero) is c: dc = (c - 0.5) / SH_C0"""
    return ((np.asarray(c, np.float64) - 0.5) / SH_C0).astype(np.float32)
