"""Drop-in for the reference's ``from odak_perception import MetamericLoss`` (metamer/odak_perception/metameric_loss.py), the
gaze-dependent (foveated) HVS loss that hvs_loss_calc.py:34-49 builds and hvs_metrics.py prints as "HVS FOV", as fused HIP
kernels (csrc/hvs_fov.hip, include/fovraster.h: fr_hvs_fov_*): one forward and one backward C call.

    from fov3dgs_amd.odak_perception import MetamericLoss
    loss_fn = MetamericLoss(device="cuda", alpha=0.05, real_image_width=1.0, real_viewing_distance=0.5, n_pyramid_levels=5,
                            mode="quadratic", n_orientations=6, use_l2_foveal_loss=False, loss_type="MSE", use_bilinear_downup=True)
    loss = loss_fn(image, target, gaze=[0.5, 0.5])     # device scalar; autograd to `image` only

``filters=`` and ``resize=`` are MetamericLossUniform's (see the package docstring): the filter coefficients are an input, and
``resize="pyramid"`` resizes both pictures to the pyramid's size inside the kernels.

Supported: use_bilinear_downup=True, mode "quadratic" / "linear", loss_type "L1" / "MSE", use_l2_foveal_loss=False (then any
fovea_weight is accepted and unused, as in the reference), use_radial_weight=False, use_fullres_l0=False, equi=False, [1,3,H,W]
or [3,H,W] GPU tensors, image_colorspace "RGB" / "YCrCb", n_pyramid_levels 2..6, up to 8 orientations. Anything else raises and
names what is unsupported. A size on which the reference itself raises (a pyramid level whose mip chain ends neither at 1x1 nor
at 1x2, e.g. 64x32 or 32x96) raises ValueError.

Kept from call to call, with no host synchronisation in the call:
  the LOD maps (one per pyramid level, built on the device in double) while the size, the four display parameters and the gaze
  stay the same: a gaze change costs kernels only;
  the target's state (bands and mip chains) under MetamericLossUniform's rule: the same tensor object, address, shape, strides
  and autograd _version, the same settings, colour space and device. The gaze is part of the settings.
A difference from the reference, on purpose: when only the gaze changes between two calls with an equal target, the reference
keeps the target's statistics of the PREVIOUS gaze (metameric_loss.py:239-249 compares the target's values only). That is a bug
there and is not reproduced: both pictures are always evaluated with the gaze of the call.
"""
import weakref

import torch

from . import _native_hvs as _hvs
from . import _native_hvs_fov as _fov


class MetamericLoss:
    def __init__(self, device=torch.device("cpu"), alpha=0.2, real_image_width=0.2, real_viewing_distance=0.7, n_pyramid_levels=5,
                 mode="quadratic", n_orientations=2, use_l2_foveal_loss=True, fovea_weight=20.0, use_radial_weight=False,
                 use_fullres_l0=False, equi=False, loss_type="L1", use_bilinear_downup=False, filters=None):
        from . import _load_filters, pack_filters
        if not use_bilinear_downup:
            raise NotImplementedError("MetamericLoss: use_bilinear_downup=False (the non-bilinear pyramid) is unsupported; "
                                      "hvs_loss_calc.py passes use_bilinear_downup=True")
        if use_l2_foveal_loss:
            raise NotImplementedError("MetamericLoss: use_l2_foveal_loss=True (the direct L2 term in the fovea and fovea_weight) is "
                                      "unsupported; hvs_loss_calc.py passes use_l2_foveal_loss=False")
        if use_radial_weight:
            raise NotImplementedError("MetamericLoss: use_radial_weight=True is unsupported")
        if use_fullres_l0:
            raise NotImplementedError("MetamericLoss: use_fullres_l0=True is unsupported")
        if equi:
            raise NotImplementedError("MetamericLoss: equi=True (equirectangular input) is unsupported")
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
        self.n_pyramid_levels = n_pyramid_levels
        self.n_orientations = n_orientations
        self.mode = mode
        self.use_l2_foveal_loss = use_l2_foveal_loss
        self.fovea_weight = fovea_weight
        self.use_radial_weight = use_radial_weight
        self.use_fullres_l0 = use_fullres_l0
        self.equi = equi
        self.loss_type = loss_type
        self.use_bilinear_downup = use_bilinear_downup
        self._filters_cpu = pack_filters(_load_filters(n_orientations) if filters is None else filters, n_orientations)
        self._filters_dev = {}
        self._target = None  # (weakref, signature, state tensor)
        self._lod = None     # (key, device, float64 tensor, filled)

    def to(self, device):
        self.device = torch.device(device)
        return self

    def _filters_on(self, device):
        f = self._filters_dev.get(device)
        if f is None:
            f = self._filters_dev[device] = self._filters_cpu.to(device)
        return f

    def _settings(self, H, W, rgb, gaze):
        return _fov.Settings(H, W, float(self.alpha), float(self.real_image_width), float(self.real_viewing_distance),
                             1 if self.mode == "quadratic" else 0, float(gaze[0]), float(gaze[1]), self.n_pyramid_levels,
                             self.n_orientations, 1 if self.loss_type == "MSE" else 0, 1 if rgb else 0)

    def _target_state(self, target, tgt, st):
        """-> (state tensor, fresh): fresh = the kernels must fill it from `tgt` in this call"""
        sig = (id(target), target._version, target.data_ptr(), tuple(target.shape), target.stride(), target.dtype, target.device, st)
        ent = self._target
        if ent is not None and ent[0]() is target and ent[1] == sig:
            return ent[2], False
        state = torch.empty(_fov.floats(st, 0), dtype=torch.float32, device=tgt.device)
        try:
            self._target = (weakref.ref(target), sig, state)
        except TypeError:
            self._target = None
        return state, True

    def _lod_maps(self, st, device):
        """-> (float64 device buffer of every level's LOD map, valid): valid = it was filled by an earlier call with this size,
        these parameters and this gaze. Another gaze gets a NEW buffer: a graph of an earlier call may still hold the old one."""
        key = _fov.lod_key(st)
        ent = self._lod
        if ent is not None and ent[0] == key and ent[1] == device:
            return ent[2], ent[3]
        buf = torch.empty(_fov.floats(st, 3) // 2, dtype=torch.float64, device=device)
        self._lod = (key, device, buf, False)
        return buf, False

    def lod_maps(self, height, width, gaze=[0.5, 0.5], device=None):
        """the LOD maps of a height x width call, one float64 [h,w] tensor per pyramid level, as the kernels build them (the
        reference's RadiallyVaryingBlur.lod_map of blurs[l]); for tests and tools"""
        device = torch.device(self.device if device is None else device)
        st = self._settings(height, width, True, gaze)
        buf = torch.empty(_fov.floats(st, 3) // 2, dtype=torch.float64, device=device)
        x = torch.zeros(3, height, width, device=device)
        state = torch.empty(_fov.floats(st, 0), dtype=torch.float32, device=device)
        with torch.no_grad():
            _fov.HvsFovLoss.apply(x, x, state, buf, False, self._filters_on(device), st)
        return [buf[lv["lod"]:lv["lod"] + lv["h"] * lv["w"]].reshape(lv["h"], lv["w"]) for lv in _fov.layout(st)]

    def __call__(self, image, target, gaze=[0.5, 0.5], image_colorspace="RGB", visualise_loss=False, resize=None):
        if visualise_loss:
            raise NotImplementedError("MetamericLoss: visualise_loss is unsupported")
        if image_colorspace not in ("RGB", "YCrCb"):
            raise ValueError(f"image_colorspace={image_colorspace!r} is unsupported: 'RGB' or 'YCrCb'")
        try:
            xy = tuple(float(v) for v in gaze)
        except (TypeError, ValueError):
            xy = ()
        if len(xy) != 2 or not all(abs(v) < 1e6 for v in xy):
            raise ValueError(f"gaze={gaze!r} is malformed: two finite numbers (x, y) in normalised image coordinates")
        gaze = xy
        if not (torch.is_tensor(image) and torch.is_tensor(target)):
            raise TypeError("image and target must be tensors")
        if image.shape != target.shape:
            raise ValueError(f"image {tuple(image.shape)} and target {tuple(target.shape)} differ")
        shape = tuple(image.shape)
        if len(shape) == 4 and shape[0] != 1:
            raise NotImplementedError(f"MetamericLoss: batches are unsupported (N={shape[0]}); call it per image")
        if len(shape) not in (3, 4) or shape[-3] != 3:
            raise NotImplementedError(f"MetamericLoss: only 3-channel [1,3,H,W] / [3,H,W] input is supported, got {shape} "
                                      "(1-channel input is unsupported)")
        H, W = shape[-2], shape[-1]
        size = _hvs_resize_size(self, resize, H, W)
        d = 2 ** self.n_pyramid_levels
        if size is None and (H % d or W % d):
            raise ValueError("MetamericLoss: the image size is no multiple of 2 ** n_pyramid_levels (the reference pads such a "
                             "picture; padding is unsupported: pass resize='pyramid', as hvs_loss_calc.py resizes)")
        if not (image.is_cuda and target.is_cuda):
            raise RuntimeError("MetamericLoss needs GPU tensors: there is no CPU fallback")
        if image.device != target.device:
            raise RuntimeError(f"image is on {image.device}, target on {target.device}")
        st = self._settings(H, W, image_colorspace == "RGB", gaze)
        if size is not None:  # the pictures are H x W and the loss runs at `size`
            st = st._replace(H=size[0], W=size[1], Hs=H, Ws=W)
        tgt = target.detach().reshape(3, H, W)
        if tgt.dtype != torch.float32 or not tgt.is_contiguous():
            tgt = tgt.float().contiguous()
        state_t, fresh = self._target_state(target, tgt, st)
        lod, lod_valid = self._lod_maps(st, image.device)
        try:
            out = _fov.HvsFovLoss.apply(image, tgt if fresh else None, state_t, lod, lod_valid, self._filters_on(image.device), st)
        except BaseException:
            self._target = None  # (the state may not have been filled)
            self._lod = None
            raise
        if not lod_valid:
            self._lod = self._lod[:3] + (True,)
        return out


def _hvs_resize_size(fn, resize, Hs, Ws):
    from . import MetamericLossUniform
    return MetamericLossUniform._resize_size(fn, resize, Hs, Ws)
