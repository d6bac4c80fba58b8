"""The two C calls behind MetamericLossUniform (include/fovraster.h: fr_hvs_forward / fr_hvs_backward, and their _resized forms
for pictures that are resized to the pyramid's size inside the kernels) as an autograd Function."""
import collections

import torch

from .. import _native

MAX_LEVELS, MAX_ORIENTATIONS = 6, 8
# H, W: the size the loss runs at. Hs, Ws: the pictures' own size when they are resized to H x W in the kernels, else 0, 0.
Settings = collections.namedtuple("Settings", "H W pooling levels orientations mse rgb Hs Ws", defaults=(0, 0))


def floats(st, which):
    """floats of 0 = one picture's forward state, 1 = the backward workspace, 2 = the partial sums"""
    n = _native.load().fr_hvs_workspace_floats(st.H, st.W, st.pooling, st.levels, st.orientations, which)
    if n < 0:
        raise ValueError(f"MetamericLossUniform: {_native.last_error()}")
    return n


def backward_floats(st):
    """floats of the backward workspace: the plain one, plus the gradient before the resize's adjoint when st resizes"""
    if not st.Hs:
        return floats(st, 1)
    n = _native.load().fr_hvs_resized_backward_floats(st.Hs, st.Ws, st.H, st.W, st.pooling, st.levels, st.orientations)
    if n < 0:
        raise ValueError(f"MetamericLossUniform: {_native.last_error()}")
    return n


def _f32(t, H, W):
    t = t.detach().reshape(3, H, W)
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


class HvsLoss(torch.autograd.Function):
    """(image, target [3,H,W] fp32 or None = state_t is valid, state_t, filters (device), settings) -> loss (device scalar);
    image and target are [3,Hs,Ws] where the settings resize"""

    @staticmethod
    def forward(ctx, image, tgt, state_t, filters, st):
        lib = _native.load()
        x = _f32(image, st.Hs or st.H, st.Ws or st.W)
        dev = x.device
        state_i = torch.empty(floats(st, 0), dtype=torch.float32, device=dev)
        partials = torch.empty(floats(st, 2), dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        call, size = (lib.fr_hvs_forward_resized, (st.Hs, st.Ws, st.H, st.W)) if st.Hs else (lib.fr_hvs_forward, (st.H, st.W))
        with torch.cuda.device(dev):
            rc = call(*size, st.pooling, st.levels, st.orientations, st.mse, st.rgb, filters.data_ptr(), x.data_ptr(),
                      None if tgt is None else tgt.data_ptr(), state_i.data_ptr(), state_t.data_ptr(),
                      partials.data_ptr(), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"fovraster hvs_forward failed ({rc}): {_native.last_error()}")
        ctx.st, ctx.shape, ctx.dtype = st, image.shape, image.dtype
        ctx.save_for_backward(state_i, state_t, filters)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        lib, st = _native.load(), ctx.st
        state_i, state_t, filters = ctx.saved_tensors
        dev = state_i.device
        work = torch.empty(backward_floats(st), dtype=torch.float32, device=dev)
        grad = torch.empty((3, st.Hs or st.H, st.Ws or st.W), dtype=torch.float32, device=dev)
        g = g.detach().reshape(-1)[:1]
        if g.dtype != torch.float32 or g.device != dev:
            g = g.to(device=dev, dtype=torch.float32)
        call, size = (lib.fr_hvs_backward_resized, (st.Hs, st.Ws, st.H, st.W)) if st.Hs else (lib.fr_hvs_backward, (st.H, st.W))
        with torch.cuda.device(dev):
            rc = call(*size, st.pooling, st.levels, st.orientations, st.mse, st.rgb, filters.data_ptr(),
                      state_i.data_ptr(), state_t.data_ptr(), work.data_ptr(), g.data_ptr(), grad.data_ptr(),
                      torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"fovraster hvs_backward failed ({rc}): {_native.last_error()}")
        grad = grad.reshape(ctx.shape)
        return (grad if ctx.dtype == torch.float32 else grad.to(ctx.dtype)), None, None, None, None


def layout(st):
    """Where the forward state (floats(st, 0)) keeps what, as csrc/hvs.hip lays it out: per band level a dict with h, w, the
    number of maps nm (h in front of the bands at level 0), `maps` -> offset of [nm,3,h,w], identity (1/p is an integer: the
    level is compared directly and not pooled), else ph, pw and `pool` -> offset of [2,nm,3,ph,pw] (mean, mean-square), and
    `low_out` -> offset of the next level's lowpass [3,h/2,w/2] (the last one is the lowpass residual). For tests and tools."""
    import math
    levels, ws, p = [], 0, float(st.pooling)
    for l in range(st.levels - 1):
        h, w, nm = st.H >> l, st.W >> l, st.orientations + (1 if l == 0 else 0)
        k = 1.0 / p
        lv = dict(h=h, w=w, nm=nm, identity=k >= 1.0 and k == math.floor(k), maps=ws)
        ws += nm * 3 * h * w
        if not lv["identity"]:
            lv.update(ph=int(math.floor(h * k)), pw=int(math.floor(w * k)), pool=ws)
            ws += 2 * nm * 3 * lv["ph"] * lv["pw"]
        lv["low_out"] = ws
        ws += 3 * (h // 2) * (w // 2)
        levels.append(lv)
        p /= 2
    assert ws == floats(st, 0)
    return levels
