"""Drop-ins for the reference's ``utils/image_utils.py`` (:14-19): ``mse`` and ``psnr`` per row of ``view(shape[0], -1)``, as ONE
HIP launch over the pair plus a one-workgroup finish (csrc/quality.hip, include/fovraster.h: fr_quality_*) instead of a
subtraction, a square, a mean, a sqrt, a division, a log10 and a scale.

As the reference does, a ``[1,3,H,W]`` input gives one value and a ``[3,H,W]`` input gives one per channel; the result is
``[N,1]``. ``mse == 0`` gives ``psnr == inf``. The squares and their sums are double and are added in a fixed order: the same bits
on every run. GPU tensors only: there is no CPU fallback."""
import torch

from . import _native


def _planes(img1, img2, what):
    """-> (x, y, N, C, H, W): the inputs as N rows of C / N planes of H x W, fp32 and contiguous"""
    for t in (img1, img2):
        if not torch.is_tensor(t):
            raise TypeError(f"fovraster {what} expects torch tensors, got {type(t).__name__}")
    if img1.shape != img2.shape:
        raise ValueError(f"{what}: the shapes {tuple(img1.shape)} and {tuple(img2.shape)} differ")
    if img1.dim() < 2 or img1.numel() == 0:
        raise ValueError(f"{what}: expected [N, ...] pictures with at least two dimensions and one element, got {tuple(img1.shape)}")
    if not img1.is_floating_point() or not img2.is_floating_point():
        raise ValueError(f"{what}: expected floating-point pictures, got {img1.dtype} and {img2.dtype}")
    if not img1.is_cuda or not img2.is_cuda:
        raise RuntimeError(f"fovraster {what} needs GPU tensors: there is no CPU fallback")
    if img1.device != img2.device:
        raise RuntimeError(f"fovraster {what}: tensors on {img1.device} and {img2.device}")
    N = img1.shape[0]
    H, W = (1, img1.shape[1]) if img1.dim() == 2 else (img1.shape[-2], img1.shape[-1])
    C = img1.numel() // (H * W)
    x = img1.detach().to(torch.float32).contiguous()
    y = img2.detach().to(torch.float32).contiguous()
    return x, y, N, C, H, W


def _measure(x, y, rows, C, H, W, with_ssim, per_view, slot, accum, partials=None):
    """Enqueue the pass over the pair and the finish on the current stream. per_view: float32 [capacity,4] whose rows
    slot .. slot + rows - 1 receive (ssim, psnr, l1, mse); accum: float64 [4] or None. Nothing synchronises."""
    lib = _native.load()
    nb = int(lib.fr_quality_blocks(C, H, W))
    if nb <= 0:
        raise ValueError(f"fovraster quality: a picture of {C} planes of {H}x{W} is outside what the kernels take")
    if partials is None or partials.numel() < 3 * nb:
        partials = torch.empty(3 * nb, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        rc = lib.fr_quality_forward(C, H, W, int(with_ssim), x.data_ptr(), y.data_ptr(), partials.data_ptr(), stream)
        if rc == 0:
            rc = lib.fr_quality_finish(C, H, W, rows, partials.data_ptr(), per_view.data_ptr(), slot, per_view.shape[0],
                                       None if accum is None else accum.data_ptr(), stream)
    if rc != 0:
        raise RuntimeError(f"fovraster quality failed ({rc}): {_native.last_error()}")
    return partials


def _rows(img1, img2, what):
    x, y, N, C, H, W = _planes(img1, img2, what)
    out = torch.empty((N, 4), dtype=torch.float32, device=x.device)
    _measure(x, y, N, C, H, W, False, out, 0, None)
    return out


def mse(img1, img2):
    """image_utils.py:14-15: ``((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)`` -> [N,1]"""
    return _rows(img1, img2, "mse")[:, 3:4]


def psnr(img1, img2):
    """image_utils.py:17-19: ``20 * log10(1 / sqrt(mse))`` per row -> [N,1]"""
    return _rows(img1, img2, "psnr")[:, 1:2]
