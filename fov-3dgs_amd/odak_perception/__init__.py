"""Drop-in for the reference's ``from odak_perception import MetamericLossUniform`` (metamer/odak_perception/
metameric_loss_uniform.py), the HVS loss of metric_mask_learn.py:148-149 / :227 and eff_finetune.py:61-62 / :122, as fused HIP
kernels (csrc/hvs.hip, include/fovraster.h: fr_hvs_*): one forward and one backward C call, no torch operator between the image
and the scalar or between the upstream gradient and dL/dimage (allocations and a dtype / layout conversion of an input that
is not contiguous fp32 excepted).

    from fov3dgs_amd.odak_perception import MetamericLossUniform
    loss_fn = MetamericLossUniform(device="cuda", pooling_size=9, n_pyramid_levels=5, n_orientations=6, loss_type="L1",
                                   bilinear_downsampling=True)
    loss = loss_fn(image, target)          # device scalar; autograd to `image` only (the reference detaches the target)

The filter coefficients are an INPUT. ``filters=`` takes the dict get_steerable_pyramid_filters(5, n, "cropped") returns
("l0", "h0": [1,1,5,5]; "b": a list of [1,1,5,5]). With ``filters=None`` the class imports
``odak_perception.steerable_pyramid_filters`` from the caller's environment (the reference's scripts put ../metamer on sys.path)
and calls that function; when the import fails it raises and says to pass ``filters=``. This package holds no coefficients.

Supported: bilinear_downsampling=True, 5x5 filters, loss_type "L1" / "MSE", [1,3,H,W] or [3,H,W] GPU tensors, image_colorspace
"RGB" / "YCrCb", n_pyramid_levels 2..6, any positive pooling_size, up to 8 orientations. Anything else raises and names what
is unsupported; a size that is no multiple of 2**n_pyramid_levels raises ValueError as pad_image_for_pyramid does; CPU tensors
raise (no CPU fallback, as everywhere in this library).

Resize: the steerable pyramid needs a size that is a multiple of 2**n_pyramid_levels, and 1080 is none of 32. ``resize=``
does what the reference's scripts do with F.interpolate(x, size=.., mode='bilinear', align_corners=False) on both pictures
before the call (metric_mask_learn.py:221-227, eff_finetune.py:116-122, prune.py:128-134), inside the kernels:

    loss = loss_fn(image, target, resize="pyramid")       # to pyramid_size(H, W, n_pyramid_levels); or resize=(height, width)

``image`` and ``target`` are the un-resized pictures and the gradient has ``image``'s shape. The samples are taken in the load
of the first pyramid level and the adjoint is a gather per source pixel: no resized picture is written, nothing is added with
atomics, the same bits on every run. The size may only grow (or stay) on each axis; a size equal to the input's is the plain
call. Because the caller's own target tensor is what the call sees, the target state below is reusable across steps for a
caller that keeps its ground truth on the GPU. ``resize=None`` is the call without it, bit for bit.

Target state: the target's pyramid statistics are kept from call to call and reused only when the target is provably the one
they were computed from -- the same tensor object (held by a weak reference), address, shape, strides and autograd _version,
the same settings (the resize size among them), colour space and device (rasterizer.py's rule for "unchanged"). Anything else recomputes them in the same
launches as the image's. There is no host synchronisation in the call.

``MetamericLoss`` (metameric_loss.py, csrc/hvs_fov.hip) is the gaze-dependent loss of the same package: its docstring says what
it supports. ``MetamerMSELoss`` (metamer_mse_loss.py, csrc/metamer.hip) is the third name of the reference's import line: it
synthesises a metamer of the target and compares against that picture; ``pyramid_roundtrip`` is its synthesis alone.
"""
import importlib
import math
import weakref

import torch

from . import _native_hvs as _hvs

__all__ = ["MetamericLossUniform", "MetamericLoss", "MetamerMSELoss", "pyramid_size", "pyramid_roundtrip"]


def pyramid_size(height, width, n_pyramid_levels):
    """-> (required_height, required_width): the next multiples of 2**n_pyramid_levels, the size the reference's scripts resize
    to before the HVS loss (metric_mask_learn.py:188-190, eff_finetune.py:66-68: math.ceil(h / 2**n) * 2**n)"""
    d = 2 ** n_pyramid_levels
    return int(math.ceil(height / d) * d), int(math.ceil(width / d) * d)


def _load_filters(n_orientations):
    try:
        mod = importlib.import_module("odak_perception.steerable_pyramid_filters")
        return mod.get_steerable_pyramid_filters(5, n_orientations, "cropped")
    except Exception as e:  # ImportError, or a module of that name without the function
        raise RuntimeError(
            "MetamericLossUniform: the steerable-pyramid filter coefficients are an input of this library and "
            f"odak_perception.steerable_pyramid_filters could not be used from this environment ({type(e).__name__}: {e}). "
            "Pass filters= (the dict get_steerable_pyramid_filters(5, n_orientations, 'cropped') returns), or put the "
            "reference's metamer/ directory on sys.path.") from e


def pack_filters(filters, n_orientations):
    """-> CPU fp32 tensor [(2 + n) * 25]: l0, h0, b_0 .. b_{n-1} (the layout fr_hvs_forward reads)"""
    if not isinstance(filters, dict) or not all(k in filters for k in ("l0", "h0", "b")):
        raise ValueError('filters must be a dict with "l0", "h0" and "b" (the layout of get_steerable_pyramid_filters)')
    bands = list(filters["b"])
    if len(bands) < n_orientations:
        raise ValueError(f"n_orientations={n_orientations} but the filter set holds {len(bands)} oriented filters")
    rows = []
    for name, f in [("l0", filters["l0"]), ("h0", filters["h0"])] + [(f"b[{i}]", b) for i, b in enumerate(bands[:n_orientations])]:
        f = torch.as_tensor(f).detach().to("cpu", torch.float32)
        if f.numel() != 25 or tuple(f.shape[-2:]) != (5, 5):
            raise ValueError(f"filter {name} has shape {tuple(f.shape)}: only the cropped 5x5 filters are supported")
        rows.append(f.reshape(25))
    return torch.cat(rows).contiguous()


class MetamericLossUniform:
    def __init__(self, device=torch.device("cpu"), pooling_size=32, n_pyramid_levels=5, n_orientations=2, loss_type="L1",
                 bilinear_downsampling=False, filters=None):
        if not bilinear_downsampling:
            raise NotImplementedError("MetamericLossUniform: bilinear_downsampling=False (the non-bilinear pyramid) is unsupported; "
                                      "the training scripts pass bilinear_downsampling=True")
        if loss_type not in ("L1", "MSE"):
            raise ValueError("loss_type must be 'L1' or 'MSE'")
        if not (isinstance(n_pyramid_levels, int) and 2 <= n_pyramid_levels <= _hvs.MAX_LEVELS):
            raise ValueError(f"n_pyramid_levels={n_pyramid_levels!r} is unsupported: 2..{_hvs.MAX_LEVELS}")
        if not (isinstance(n_orientations, int) and 1 <= n_orientations <= _hvs.MAX_ORIENTATIONS):
            raise ValueError(f"n_orientations={n_orientations!r} is unsupported: 1..{_hvs.MAX_ORIENTATIONS}")
        if not (float(pooling_size) > 0.0):
            raise ValueError(f"pooling_size={pooling_size!r} must be positive")
        self.device = torch.device(device)
        self.pooling_size = pooling_size
        self.n_pyramid_levels = n_pyramid_levels
        self.n_orientations = n_orientations
        self.loss_type = loss_type
        self.bilinear_downsampling = bilinear_downsampling
        self._filters_cpu = pack_filters(_load_filters(n_orientations) if filters is None else filters, n_orientations)
        self._filters_dev = {}
        self._target = None  # (weakref, signature, state tensor)

    def to(self, device):
        self.device = torch.device(device)
        return self

    def gen_metamer(self, image):
        raise NotImplementedError("MetamericLossUniform.gen_metamer is unsupported (out of scope of the fused loss)")

    def _filters_on(self, device):
        f = self._filters_dev.get(device)
        if f is None:
            f = self._filters_dev[device] = self._filters_cpu.to(device)
        return f

    def _settings(self, H, W, rgb):
        return _hvs.Settings(H, W, float(self.pooling_size), self.n_pyramid_levels, self.n_orientations,
                             1 if self.loss_type == "MSE" else 0, 1 if rgb else 0)

    def _target_state(self, target, tgt, st):
        """-> (state tensor, fresh): fresh = the kernels must fill it from `tgt` in this call"""
        sig = (id(target), target._version, target.data_ptr(), tuple(target.shape), target.stride(), target.dtype, target.device, st)
        ent = self._target
        if ent is not None and ent[0]() is target and ent[1] == sig:
            return ent[2], False
        state = torch.empty(_hvs.floats(st, 0), dtype=torch.float32, device=tgt.device)
        try:
            self._target = (weakref.ref(target), sig, state)
        except TypeError:
            self._target = None
        return state, True

    def _resize_size(self, resize, Hs, Ws):
        """-> (H, W) the loss runs at, or None for the plain call (no resize asked for, or to the pictures' own size)"""
        if resize is None:
            return None
        if isinstance(resize, str):
            if resize != "pyramid":
                raise ValueError(f"resize={resize!r} is malformed: None, 'pyramid' or (height, width)")
            size = pyramid_size(Hs, Ws, self.n_pyramid_levels)
        else:
            try:
                size = tuple(resize)
            except TypeError:
                size = ()
            if len(size) != 2 or not all(isinstance(v, int) and not isinstance(v, bool) and v > 0 for v in size):
                raise ValueError(f"resize={resize!r} is malformed: None, 'pyramid' or (height, width) as two positive ints")
        if size == (Hs, Ws):
            return None
        H, W = size
        if H < Hs or W < Ws:
            raise ValueError(f"resize={size}: shrinking a {Hs}x{Ws} picture is unsupported (each side may only grow or stay)")
        d = 2 ** self.n_pyramid_levels
        if H % d or W % d:
            raise ValueError(f"resize={size}: the resize size is no multiple of 2 ** n_pyramid_levels = {d} "
                             f"(pyramid_size gives {pyramid_size(Hs, Ws, self.n_pyramid_levels)})")
        return size

    def __call__(self, image, target, image_colorspace="RGB", visualise_loss=False, resize=None):
        if visualise_loss:
            raise NotImplementedError("MetamericLossUniform: visualise_loss is unsupported")
        if image_colorspace not in ("RGB", "YCrCb"):
            raise ValueError(f"image_colorspace={image_colorspace!r} is unsupported: 'RGB' or 'YCrCb'")
        if not (torch.is_tensor(image) and torch.is_tensor(target)):
            raise TypeError("image and target must be tensors")
        if image.shape != target.shape:
            raise ValueError(f"image {tuple(image.shape)} and target {tuple(target.shape)} differ")
        shape = tuple(image.shape)
        if len(shape) == 4 and shape[0] != 1:
            raise NotImplementedError(f"MetamericLossUniform: batches are unsupported (N={shape[0]}); call it per image")
        if len(shape) not in (3, 4) or shape[-3] != 3:
            raise NotImplementedError(f"MetamericLossUniform: only 3-channel [1,3,H,W] / [3,H,W] input is supported, got {shape} "
                                      "(1-channel input is unsupported)")
        H, W = shape[-2], shape[-1]
        size = self._resize_size(resize, H, W)
        d = 2 ** self.n_pyramid_levels
        if size is None and (H % d or W % d):
            raise ValueError("Please make the image size valid (Multiplies of 2 ** n_pyramid_levels) before input to HVS function.")
        if not (image.is_cuda and target.is_cuda):
            raise RuntimeError("MetamericLossUniform needs GPU tensors: there is no CPU fallback")
        if image.device != target.device:
            raise RuntimeError(f"image is on {image.device}, target on {target.device}")
        st = self._settings(H, W, image_colorspace == "RGB")
        if size is not None:  # the pictures are H x W and the loss runs at `size`
            st = st._replace(H=size[0], W=size[1], Hs=H, Ws=W)
        tgt = target.detach().reshape(3, H, W)
        if tgt.dtype != torch.float32 or not tgt.is_contiguous():
            tgt = tgt.float().contiguous()
        state_t, fresh = self._target_state(target, tgt, st)
        try:
            return _hvs.HvsLoss.apply(image, tgt if fresh else None, state_t, self._filters_on(image.device), st)
        except BaseException:
            self._target = None  # (the state may not have been filled)
            raise


from .metameric_loss import MetamericLoss  # noqa: E402  (it uses pack_filters and _resize_size from above)
from .metamer_mse_loss import MetamerMSELoss, pyramid_roundtrip  # noqa: E402
