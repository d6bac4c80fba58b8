"""The two C calls behind MetamericLoss (include/fovraster.h: fr_hvs_fov_forward / fr_hvs_fov_backward) as an autograd
Function, and the layout of the state they keep (for tests and tools)."""
import collections

import torch

from .. import _native
from ._native_hvs import MAX_LEVELS

# H, W: the size the loss runs at. Hs, Ws: the pictures' own size when they are resized to H x W in the kernels, else 0, 0.
# mode: 1 = "quadratic", 0 = "linear". gaze_x, gaze_y: normalised image coordinates.
Settings = collections.namedtuple("Settings", "H W alpha width distance mode gaze_x gaze_y levels orientations mse rgb Hs Ws",
                                  defaults=(0, 0))


def floats(st, which):
    """floats of 0 = one picture's forward state, 1 = the backward workspace, 2 = the partial sums, 3 = the LOD maps (doubles)"""
    n = _native.load().fr_hvs_fov_workspace_floats(st.Hs, st.Ws, st.H, st.W, st.levels, st.orientations, which)
    if n < 0:
        raise ValueError(f"MetamericLoss: {_native.last_error()}")
    return n


def lod_key(st):
    """what the LOD maps depend on"""
    return st.H, st.W, st.levels, st.alpha, st.width, st.distance, st.mode, st.gaze_x, st.gaze_y


def _head(st):
    return (st.Hs, st.Ws, st.H, st.W, st.alpha, st.width, st.distance, st.mode, st.gaze_x, st.gaze_y, st.levels, st.orientations,
            st.mse, st.rgb)


def _f32(t, H, W):
    t = t.detach().reshape(3, H, W)
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


class HvsFovLoss(torch.autograd.Function):
    """(image, target [3,H,W] fp32 or None = state_t is valid, state_t, lod (float64 device buffer), lod_valid, filters (device),
    settings) -> loss (device scalar); image and target are [3,Hs,Ws] where the settings resize"""

    @staticmethod
    def forward(ctx, image, tgt, state_t, lod, lod_valid, filters, st):
        lib = _native.load()
        x = _f32(image, st.Hs or st.H, st.Ws or st.W)
        dev = x.device
        state_i = torch.empty(floats(st, 0), dtype=torch.float32, device=dev)
        partials = torch.empty(floats(st, 2), dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.fr_hvs_fov_forward(*_head(st), filters.data_ptr(), x.data_ptr(), None if tgt is None else tgt.data_ptr(),
                                        state_i.data_ptr(), state_t.data_ptr(), lod.data_ptr(), 1 if lod_valid else 0,
                                        partials.data_ptr(), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"fovraster hvs_fov_forward failed ({rc}): {_native.last_error()}")
        ctx.st, ctx.shape, ctx.dtype = st, image.shape, image.dtype
        ctx.save_for_backward(state_i, state_t, lod, filters)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        lib, st = _native.load(), ctx.st
        state_i, state_t, lod, filters = ctx.saved_tensors
        dev = state_i.device
        work = torch.empty(floats(st, 1), dtype=torch.float32, device=dev)
        grad = torch.empty((3, st.Hs or st.H, st.Ws or st.W), dtype=torch.float32, device=dev)
        g = g.detach().reshape(-1)[:1]
        if g.dtype != torch.float32 or g.device != dev:
            g = g.to(device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            rc = lib.fr_hvs_fov_backward(*_head(st), filters.data_ptr(), state_i.data_ptr(), state_t.data_ptr(), lod.data_ptr(),
                                         work.data_ptr(), g.data_ptr(), grad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"fovraster hvs_fov_backward failed ({rc}): {_native.last_error()}")
        grad = grad.reshape(ctx.shape)
        return (grad if ctx.dtype == torch.float32 else grad.to(ctx.dtype)), None, None, None, None, None, None


def chain_sizes(h, w):
    """the sizes of a map's mip chain, [(h, w), (h // 2, w // 2), ..]: halved while both sides exceed 1; a chain that stops at
    1x2 gets one more level, 1x1. ValueError for a chain that ends anywhere else (csrc/hvs_fov.hip refuses those sizes)."""
    sizes = [(h, w)]
    while sizes[-1][0] > 1 and sizes[-1][1] > 1:
        sizes.append((sizes[-1][0] // 2, sizes[-1][1] // 2))
    if sizes[-1] == (1, 2):
        sizes.append((1, 1))
    if sizes[-1] != (1, 1):
        raise ValueError(f"the mip chain of a {h}x{w} map ends at {sizes[-1][0]}x{sizes[-1][1]}, not at 1x1 or 1x2")
    return sizes


def layout(st):
    """Where the forward state (floats(st, 0)) keeps what, as csrc/hvs_fov.hip lays it out: per band level a dict with h, w, the
    number of maps nm (h in front of the bands at level 0), `maps` -> offset of [nm,3,h,w], `chain` -> the sizes of the mip chain
    (chain[0] = (h, w)), `mean`[k], `square`[k] -> offsets of level k's [nm,3,h_k,w_k] for k >= 1 (None at 0: level 0 is the
    map, and its square is never stored), `lod` -> offset (in doubles) of the level's map in the LOD buffer, and `low_out` ->
    offset of the next level's lowpass [3,h/2,w/2] (the last one is the lowpass residual). For tests and tools."""
    levels, ws, nl = [], 0, 0
    for l in range(st.levels - 1):
        h, w, nm = st.H >> l, st.W >> l, st.orientations + (1 if l == 0 else 0)
        lv = dict(h=h, w=w, nm=nm, maps=ws, chain=chain_sizes(h, w), mean=[None], square=[None], lod=nl)
        ws += nm * 3 * h * w
        nl += h * w
        for hk, wk in lv["chain"][1:]:
            lv["mean"].append(ws)
            ws += nm * 3 * hk * wk
            lv["square"].append(ws)
            ws += nm * 3 * hk * wk
        lv["low_out"] = ws
        ws += 3 * (h // 2) * (w // 2)
        levels.append(lv)
    assert ws == floats(st, 0) and 2 * (nl + MAX_LEVELS) == floats(st, 3)  # (behind the maps: every level's largest LOD)
    return levels
