"""Drop-in for the reference's ``from odak_perception import MetamerMSELoss`` (metamer/odak_perception/metamer_mse_loss.py): the
loss that builds ONE metamer of the target for a gaze -- a picture the gaze-dependent HVS model (MetamericLoss) cannot tell from
the target -- and then compares the image with that fixed picture by L1 / MSE. The metamer is the steerable pyramid's synthesis
from a noise pyramid whose bands were matched to the target's blended statistics, as fused HIP kernels (csrc/metamer.hip,
include/fovraster.h: fr_hvs_metamer_*).

    from fov3dgs_amd.odak_perception import MetamerMSELoss
    loss_fn = MetamerMSELoss(device="cuda", alpha=0.05, real_image_width=1.0, real_viewing_distance=0.5, n_pyramid_levels=5,
                             n_orientations=6, loss_type="L1", avg_pooling_downup=True)
    loss = loss_fn(image, target, gaze=[0.5, 0.5])     # device scalar; autograd to `image` only
    picture = loss_fn.gen_metamer(target, gaze=[0.3, 0.6])   # [1,3,H,W], RGB, not clamped (the reference's leaves [0, 1] too)

``filters=`` is MetamericLossUniform's (see the package docstring): the filter coefficients are an input.

Supported: avg_pooling_downup=True (the argument the reference hands to its pyramid as use_bilinear_downup; its default False
selects the other pyramid and raises here by name), equi=False, mode "quadratic" / "linear", loss_type "L1" / "MSE", [1,3,H,W] or
[3,H,W] GPU tensors, n_pyramid_levels 2..6, up to 8 orientations, sizes that are multiples of 2**n_pyramid_levels (others raise
ValueError as pad_image_for_pyramid does) and on which MetamericLoss runs.

Two differences from the reference, on purpose:
  * ``mode`` reaches the statistics. The reference's constructor accepts ``mode`` and never passes it on (metamer_mse_loss.py:49-52),
    so its metamer is always "quadratic"; here "linear" is linear.
  * The kept metamer. The reference regenerates the metamer only when the target is another OBJECT (:146-148), so after a gaze
    change, or after the target was written in place, it silently compares against a stale metamer. Here the metamer is kept and
    reused only while the target is provably the same one (MetamericLossUniform's rule: the same tensor object, address, shape,
    strides and autograd _version, the same device) AND the gaze and every setting are unchanged; anything else regenerates it.
"""
import weakref

import torch

from . import _native_hvs as _hvs
from . import _native_metamer as _met


def _gaze(gaze):
    try:
        xy = tuple(float(v) for v in gaze)
    except (TypeError, ValueError):
        xy = ()
    if len(xy) != 2 or not all(abs(v) < 1e6 for v in xy):
        raise ValueError(f"gaze={gaze!r} is malformed: two finite numbers (x, y) in normalised image coordinates")
    return xy


def _picture(name, who, t):
    """-> (H, W) of a [1,3,H,W] / [3,H,W] tensor"""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor")
    shape = tuple(t.shape)
    if len(shape) == 4 and shape[0] != 1:
        raise NotImplementedError(f"{who}: batches are unsupported (N={shape[0]}); call it per image")
    if len(shape) not in (3, 4) or shape[-3] != 3:
        raise NotImplementedError(f"{who}: only 3-channel [1,3,H,W] / [3,H,W] input is supported, got {shape} "
                                  "(1-channel input is unsupported)")
    return shape[-2], shape[-1]


def _need_gpu(who, *tensors):
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{who} needs GPU tensors: there is no CPU fallback")


def _check_size(H, W, levels):
    d = 2 ** levels
    if H % d or W % d:
        raise ValueError("Please make the image size valid (Multiplies of 2 ** n_pyramid_levels) before input to HVS function.")


class MetamerMSELoss:
    def __init__(self, device=torch.device("cpu"), alpha=0.2, real_image_width=0.2, real_viewing_distance=0.7, mode="quadratic",
                 n_pyramid_levels=5, n_orientations=2, equi=False, loss_type="L1", avg_pooling_downup=False, filters=None):
        from . import _load_filters, pack_filters
        if not avg_pooling_downup:
            raise NotImplementedError("MetamerMSELoss: avg_pooling_downup=False (the non-bilinear pyramid) is unsupported; pass "
                                      "avg_pooling_downup=True")
        if equi:
            raise NotImplementedError("MetamerMSELoss: equi=True (equirectangular input) is unsupported")
        if mode not in ("quadratic", "linear"):
            raise ValueError(f"mode={mode!r} is unsupported: 'quadratic' or 'linear'")
        if loss_type not in ("L1", "MSE"):
            raise ValueError("loss_type must be 'L1' or 'MSE'")
        if not (isinstance(n_pyramid_levels, int) and 2 <= n_pyramid_levels <= _hvs.MAX_LEVELS):
            raise ValueError(f"n_pyramid_levels={n_pyramid_levels!r} is unsupported: 2..{_hvs.MAX_LEVELS}")
        if not (isinstance(n_orientations, int) and 1 <= n_orientations <= _hvs.MAX_ORIENTATIONS):
            raise ValueError(f"n_orientations={n_orientations!r} is unsupported: 1..{_hvs.MAX_ORIENTATIONS}")
        if not (float(alpha) >= 0.0):
            raise ValueError(f"alpha={alpha!r} must not be negative")
        if not (float(real_image_width) > 0.0):
            raise ValueError(f"real_image_width={real_image_width!r} must be positive")
        if not (float(real_viewing_distance) > 0.0):
            raise ValueError(f"real_viewing_distance={real_viewing_distance!r} must be positive")
        self.device = torch.device(device)
        self.alpha = alpha
        self.real_image_width = real_image_width
        self.real_viewing_distance = real_viewing_distance
        self.mode = mode
        self.n_pyramid_levels = n_pyramid_levels
        self.n_orientations = n_orientations
        self.equi = equi
        self.loss_type = loss_type
        self.avg_pooling_downup = avg_pooling_downup
        self._filters_cpu = pack_filters(_load_filters(n_orientations) if filters is None else filters, n_orientations)
        self._filters_dev = {}
        self._kept = None  # (weakref to the target, signature, metamer [3,H,W])

    def to(self, device):
        self.device = torch.device(device)
        return self

    def _filters_on(self, device):
        f = self._filters_dev.get(device)
        if f is None:
            f = self._filters_dev[device] = self._filters_cpu.to(device)
        return f

    def _settings(self, H, W, gaze, rgb=True):
        return _met.Settings(H, W, float(self.alpha), float(self.real_image_width), float(self.real_viewing_distance),
                             1 if self.mode == "quadratic" else 0, float(gaze[0]), float(gaze[1]), self.n_pyramid_levels,
                             self.n_orientations, 1 if rgb else 0)

    def gen_metamer(self, image, gaze, noise=None, image_colorspace="RGB"):
        """The metamer of `image` for `gaze` -> [1,3,H,W] fp32, RGB (metamer_mse_loss.py:63-123).

        noise: the picture whose pyramid is matched to the image's statistics, of the image's shape, used as it is. With
        noise=None it is drawn as the reference draws it (:89-91): torch.manual_seed(0), then torch.rand_like on the image's
        device -- which RESEEDS the global generator, as the reference does. That draw depends on the device type and on the torch
        build: the same seed gives other numbers on the CPU, on a CUDA and on a ROCm device. A caller who needs the metamer the
        reference makes on a CPU or CUDA machine draws the noise there and passes it in.
        image_colorspace="YCrCb": the image is not converted on the way in (the result is RGB all the same)."""
        if image_colorspace not in ("RGB", "YCrCb"):
            raise ValueError(f"image_colorspace={image_colorspace!r} is unsupported: 'RGB' or 'YCrCb'")
        gaze = _gaze(gaze)
        H, W = _picture("image", "MetamerMSELoss", image)
        _check_size(H, W, self.n_pyramid_levels)
        _need_gpu("MetamerMSELoss", image)
        if noise is None:
            torch.manual_seed(0)
            noise = torch.rand_like(image.detach().reshape(1, 3, H, W), dtype=torch.float32)
        else:
            if not torch.is_tensor(noise) or noise.numel() != 3 * H * W:
                raise ValueError(f"noise must be a tensor of the image's shape {tuple(image.shape)}")
            if noise.device != image.device:
                raise RuntimeError(f"image is on {image.device}, noise on {noise.device}")
        st = self._settings(H, W, gaze, image_colorspace == "RGB")
        return _met.metamer(image, noise, self._filters_on(image.device), st).reshape(1, 3, H, W)

    def _metamer_of(self, target, gaze):
        H, W = target.shape[-2], target.shape[-1]
        sig = (id(target), target._version, target.data_ptr(), tuple(target.shape), target.stride(), target.dtype, target.device,
               self._settings(H, W, gaze), self.loss_type)
        ent = self._kept
        if ent is not None and ent[0]() is target and ent[1] == sig:
            return ent[2]
        metamer = self.gen_metamer(target, gaze).reshape(3, H, W)
        try:
            self._kept = (weakref.ref(target), sig, metamer)
        except TypeError:
            self._kept = None
        return metamer

    def __call__(self, image, target, gaze=[0.5, 0.5]):
        gaze = _gaze(gaze)
        H, W = _picture("image", "MetamerMSELoss", image)
        _picture("target", "MetamerMSELoss", target)
        if image.shape != target.shape:
            raise ValueError(f"image {tuple(image.shape)} and target {tuple(target.shape)} differ")
        _check_size(H, W, self.n_pyramid_levels)
        _need_gpu("MetamerMSELoss", image, target)
        if image.device != target.device:
            raise RuntimeError(f"image is on {image.device}, target on {target.device}")
        return _met.MetamerLoss.apply(image, self._metamer_of(target, gaze), 1 if self.loss_type == "MSE" else 0)


def pyramid_roundtrip(image, n_pyramid_levels, n_orientations, filters=None, image_colorspace="RGB"):
    """reconstruct_from_pyramid(construct_pyramid(image)) of the bilinear steerable pyramid (spatial_steerable_pyramid.py:132-223)
    -> a tensor of the image's shape, fp32: the synthesis kernels fed with the picture's own pyramid. With "RGB" the picture is
    converted to YCrCb on the way in and back on the way out, as gen_metamer does; with "YCrCb" the channels pass as they are.
    The 5x5 pyramid is not an identity: the result differs from the image by the pyramid's own reconstruction error."""
    from . import _load_filters, pack_filters
    if image_colorspace not in ("RGB", "YCrCb"):
        raise ValueError(f"image_colorspace={image_colorspace!r} is unsupported: 'RGB' or 'YCrCb'")
    if not (isinstance(n_pyramid_levels, int) and 2 <= n_pyramid_levels <= _hvs.MAX_LEVELS):
        raise ValueError(f"n_pyramid_levels={n_pyramid_levels!r} is unsupported: 2..{_hvs.MAX_LEVELS}")
    if not (isinstance(n_orientations, int) and 1 <= n_orientations <= _hvs.MAX_ORIENTATIONS):
        raise ValueError(f"n_orientations={n_orientations!r} is unsupported: 1..{_hvs.MAX_ORIENTATIONS}")
    H, W = _picture("image", "pyramid_roundtrip", image)
    _check_size(H, W, n_pyramid_levels)
    _need_gpu("pyramid_roundtrip", image)
    f = pack_filters(_load_filters(n_orientations) if filters is None else filters, n_orientations).to(image.device)
    return _met.roundtrip(image, f, H, W, n_pyramid_levels, n_orientations, image_colorspace == "RGB").reshape(image.shape)
