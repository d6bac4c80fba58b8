"""The C calls behind MetamerMSELoss and pyramid_roundtrip (include/fovraster.h: fr_hvs_metamer_*): the metamer and the round
trip as plain functions, the L1 / MSE loss against a kept metamer as an autograd Function."""
import collections

import torch

from .. import _native

# mode: 1 = "quadratic", 0 = "linear". gaze_x, gaze_y: normalised image coordinates. rgb: 1 = the target is RGB, 0 = YCrCb.
Settings = collections.namedtuple("Settings", "H W alpha width distance mode gaze_x gaze_y levels orientations rgb")


def workspace_floats(H, W, levels, orientations, roundtrip):
    n = _native.load().fr_hvs_metamer_workspace_floats(H, W, levels, orientations, 1 if roundtrip else 0)
    if n < 0:
        raise ValueError(f"MetamerMSELoss: {_native.last_error()}")
    return n


def _f32(t, H, W):
    t = t.detach().reshape(3, H, W)
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def metamer(target, noise, filters, st):
    """(target, noise [3,H,W] on one GPU, filters (device), settings) -> the metamer [3,H,W] fp32, RGB"""
    lib = _native.load()
    x, z = _f32(target, st.H, st.W), _f32(noise, st.H, st.W)
    dev = x.device
    work = torch.empty(workspace_floats(st.H, st.W, st.levels, st.orientations, False), dtype=torch.float32, device=dev)
    out = torch.empty((3, st.H, st.W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.fr_hvs_metamer(st.H, st.W, st.alpha, st.width, st.distance, st.mode, st.gaze_x, st.gaze_y, st.levels, st.orientations,
                                st.rgb, filters.data_ptr(), x.data_ptr(), z.data_ptr(), work.data_ptr(), out.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise RuntimeError(f"fovraster hvs_metamer failed ({rc}): {_native.last_error()}")
    return out


def roundtrip(image, filters, H, W, levels, orientations, rgb):
    """-> reconstruct_from_pyramid(construct_pyramid(image)) [3,H,W] fp32"""
    lib = _native.load()
    x = _f32(image, H, W)
    dev = x.device
    work = torch.empty(workspace_floats(H, W, levels, orientations, True), dtype=torch.float32, device=dev)
    out = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.fr_hvs_metamer_roundtrip(H, W, levels, orientations, 1 if rgb else 0, filters.data_ptr(), x.data_ptr(), work.data_ptr(),
                                          out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise RuntimeError(f"fovraster hvs_metamer_roundtrip failed ({rc}): {_native.last_error()}")
    return out


_tickets = {}


def _loss_workspace(n, dev):
    """the partial sums and the ticket word of the forward kernel, per device and stream: zeroed once, every launch leaves the
    ticket zero (launches on one stream run in order, so they may share it)"""
    need = _native.load().fr_hvs_metamer_loss_workspace_doubles(n)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    buf = _tickets.get(key)
    if buf is None or buf.numel() != need:
        buf = _tickets[key] = torch.zeros(need, dtype=torch.float64, device=dev)
    return buf


class MetamerLoss(torch.autograd.Function):
    """(image, metamer [3,H,W] fp32 contiguous, mse) -> mean |image - metamer| or mean (image - metamer)^2, a device scalar;
    autograd to image only"""

    @staticmethod
    def forward(ctx, image, metamer, mse):
        lib = _native.load()
        x = image.detach().reshape(metamer.shape)
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        dev, n = x.device, x.numel()
        out = torch.empty(1, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            work = _loss_workspace(n, dev)
            rc = lib.fr_hvs_metamer_loss_forward(n, mse, x.data_ptr(), metamer.data_ptr(), work.data_ptr(), out.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"fovraster hvs_metamer_loss_forward failed ({rc}): {_native.last_error()}")
        ctx.mse, ctx.shape, ctx.dtype = mse, image.shape, image.dtype
        ctx.save_for_backward(x, metamer)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        lib = _native.load()
        x, metamer = ctx.saved_tensors
        dev = x.device
        grad = torch.empty_like(x)
        g = g.detach().reshape(-1)[:1]
        if g.dtype != torch.float32 or g.device != dev:
            g = g.to(device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            rc = lib.fr_hvs_metamer_loss_backward(x.numel(), ctx.mse, x.data_ptr(), metamer.data_ptr(), g.data_ptr(), grad.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"fovraster hvs_metamer_loss_backward failed ({rc}): {_native.last_error()}")
        grad = grad.reshape(ctx.shape)
        return (grad if ctx.dtype == torch.float32 else grad.to(ctx.dtype)), None, None
