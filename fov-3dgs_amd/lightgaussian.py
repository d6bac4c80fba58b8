"""LightGaussian's global-significance pruning on the HIP library: how the models of the multi-model foveated baseline (MMFR)
are made (reference: LightGaussian/get_multimodel.py:64-76 -> scripts/run_prune_finetune.sh -> prune_finetune.py
--prune_type v_important_score --v_pow 0.1).

Drops in for
  gaussian_renderer.count_render          LightGaussian/gaussian_renderer/__init__.py:127-229
  prune.prune_list, calculate_v_imp_score LightGaussian/prune.py:133-157, :112-128
  GaussianModel.prune_gaussians           LightGaussian/scene/gaussian_model.py:776-782
  the prune step of prune_finetune.py     :214-242 (global_significance_prune)

  count_render            one counting render (csrc/render.hip, FR_VARIANT_COUNT): image and radii of the vanilla rasterizer plus,
                          per Gaussian, the pixels that accumulated it and that number times its opacity
  kth_value               an order statistic by radix select (csrc/prune.hip, fr_select_kth) where the reference sorts all P rows
                          to read one element -- twice per prune
  calculate_v_imp_score   volume, its 90th-percentile-largest value, (volume / that)^v_pow * score: three launches
  percentile_mask         score <= the element of rank int(percent (P - 1)); prune_gaussians cuts those rows with
                          pruning.prune_points (one plan, one gather)

One deviation from the reference, on purpose: its counting kernel (compress-diff-gaussian-rasterization, cuda_rasterizer/
forward.cu:473-474) increments gaussian_count[id] and important_score[id] with NON-atomic read-modify-writes from all 256
threads of every tile, so what it returns is not a function of its input. Here gaussians_count is exact -- the statement
executed one pixel at a time -- and important_score = float(double(count) * double(opacity)), the value the reference's fp32
running sum approximates, rounded once. Same bits on every run.

The percentile mask takes every row tied with the threshold (`<=`), and never-hit Gaussians tie at 0 by the thousand, so
the number of pruned rows is only known on the device: the compaction plan's count readback is the ONE host
synchronisation of a prune after its renders.

GPU tensors only: there is no CPU fallback. Not here: the fine-tune loop (the vanilla rasterizer, loss_utils and optim.Adam
of this package), distill_train.py. The stage after it, vectree quantisation, is fov3dgs_amd.vectree."""
import math

import torch

from . import _native, pruning
from .compress_diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
from .gaussian_renderer import _reference_model_fields
from .pruning import _check, _require_gpu, _stream, _workspace
from .rasterizer import zero_points_like

PRUNE_TYPES = ("important_score", "v_important_score", "max_v_important_score", "count", "opacity")
_DTYPES = {torch.float32: 0, torch.int32: 1}


@torch.no_grad()
def count_render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0, override_color=None):
    """The reference's count_render: -> {"render", "viewspace_points", "visibility_filter", "radii", "gaussians_count",
    "important_score"}. `pc` is anything with the GaussianModel getters; a reference-shaped model hands over its raw parameters
    and its two SH tensors as gaussian_renderer.render does. No autograd node is built (the reference's forward_count is a static
    call outside autograd): viewspace_points is a plain zero tensor."""
    xyz = pc.get_xyz
    raster_settings = GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height),
        image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5),
        tanfovy=math.tan(viewpoint_camera.FoVy * 0.5),
        bg=bg_color,
        scale_modifier=scaling_modifier,
        viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform,
        sh_degree=pc.active_sh_degree,
        campos=viewpoint_camera.camera_center,
        prefiltered=False,
        debug=bool(getattr(pipe, "debug", False)),
        f_count=True,
    )
    rasterizer = GaussianRasterizer(raster_settings=raster_settings)
    extra = {}
    scales = rotations = cov3D_precomp = None
    raw = getattr(pc, "get_raw_activation_params", None)
    act = getattr(pc, "get_activated", None) if raw is None else None
    ref_fields = _reference_model_fields(pc) if (raw is None and act is None and not hasattr(pc, "get_features_split")) else None
    if getattr(pipe, "compute_cov3D_python", False):
        cov3D_precomp = pc.get_covariance(scaling_modifier)
        opacity = pc.get_opacity
    elif raw is not None or ref_fields is not None:
        scales, rotations, opacity = raw if raw is not None else ref_fields[:3]
        extra["raw_activations"] = True
    elif act is not None:
        scales, rotations, opacity = act
    else:
        opacity, scales, rotations = pc.get_opacity, pc.get_scaling, pc.get_rotation
    shs = colors_precomp = None
    if override_color is not None:
        colors_precomp = override_color
    elif getattr(pipe, "convert_SHs_python", False):
        raise NotImplementedError("count_render: convert_SHs_python is not supported (the rasterizer evaluates the SH colours)")
    elif hasattr(pc, "get_features_split"):
        shs = pc.get_features_split
    elif ref_fields is not None:
        shs = (ref_fields[3], ref_fields[4])
    else:
        shs = pc.get_features
    out = rasterizer(means3D=xyz, means2D=None, shs=shs, colors_precomp=colors_precomp, opacities=opacity, scales=scales,
                     rotations=rotations, cov3D_precomp=cov3D_precomp, **extra)
    counts, score, image, radii = out
    visible = out.visibility_filter
    return {"render": image, "viewspace_points": zero_points_like(xyz), "visibility_filter": visible if visible is not None else radii > 0,
            "radii": radii, "gaussians_count": counts, "important_score": score}


@torch.no_grad()
def prune_list(gaussians, cameras, pipe, background):
    """The reference's prune_list: -> (gaussian_list int32 [P], imp_list float32 [P]), the per-view counts and scores of
    count_render summed over `cameras` (a list, or a scene with getTrainCameras()) by torch's `+=` in the REFERENCE'S order --
    viewpoint_stack.pop() takes the last camera first -- so that the fp32 sum of the scores has the reference's association."""
    stack = list(cameras.getTrainCameras() if hasattr(cameras, "getTrainCameras") else cameras)
    if not stack:
        raise ValueError("prune_list: no cameras")
    pkg = count_render(stack.pop(), gaussians, pipe, background)
    gaussian_list, imp_list = pkg["gaussians_count"], pkg["important_score"]
    while stack:
        pkg = count_render(stack.pop(), gaussians, pipe, background)
        gaussian_list += pkg["gaussians_count"]
        imp_list += pkg["important_score"]
    return gaussian_list, imp_list


def _values(values, what):
    _require_gpu(what, values)
    if values.dtype not in _DTYPES:
        raise ValueError(f"{what}: values must be float32 or int32, got {values.dtype}")
    P = values.shape[0] if values.dim() else 1
    v = values.detach()
    if v.dim() != 1:
        if v.numel() != P:
            raise ValueError(f"{what}: expected [P] or [P, 1], got {list(values.shape)}")
        v = v.reshape(-1)
    return v.contiguous(), P


@torch.no_grad()
def kth_value(values, k):
    """-> 0-dim device tensor: ``torch.sort(values, stable=True)[0][k]`` (ascending, NaN last, -0 == +0: a tie at zero gives
    +0.0) without the sort. values: float32 or int32 [P] or [P,1] (int32 is compared as integers). No host synchronisation."""
    v, P = _values(values, "kth_value")
    k = int(k)
    if not 0 <= k < P:
        raise ValueError(f"kth_value: k = {k} is not in 0..{P - 1}")
    out = torch.empty((), dtype=v.dtype, device=v.device)
    lib = _native.load()
    with torch.cuda.device(v.device):
        ws = _workspace(lib, P, v.device)
        rc = lib.fr_select_kth(P, v.data_ptr(), _DTYPES[v.dtype], k, out.data_ptr(), ws.data_ptr(), _stream(v.device))
    _check(rc, "select_kth")
    return out


def percentile_index(P, percent):
    """index_nth_percentile of gaussian_model.py:779, in Python floats as written"""
    return int(percent * (P - 1))


def volume_index(P):
    """prune.py:122-124 takes sorted_volume[int(len(volume) * 0.9)] of the DESCENDING order: -> that rank in ascending order"""
    return P - 1 - int(P * 0.9)


@torch.no_grad()
def percentile_mask(score, percent):
    """-> torch.bool [P]: ``score <= torch.sort(score)[0][int(percent * (P - 1))]`` (gaussian_model.py:778-781). All rows tied
    with the threshold are marked, a NaN row never is. score: float32 or int32 [P] or [P,1]. No host synchronisation."""
    v, P = _values(score, "percentile_mask")
    mask = torch.empty(P, dtype=torch.bool, device=v.device)
    if P == 0:
        return mask
    threshold = kth_value(v, percentile_index(P, percent))
    lib = _native.load()
    with torch.cuda.device(v.device):
        rc = lib.fr_mask_le(P, v.data_ptr(), _DTYPES[v.dtype], threshold.data_ptr(), mask.data_ptr(), _stream(v.device))
    _check(rc, "mask_le")
    return mask


def _scaling_of(gaussians):
    """(scaling [P,3] float32 contiguous, raw): the raw log-scales of a reference-shaped model, else get_scaling"""
    f = _reference_model_fields(gaussians)
    s, raw = (f[0], True) if f is not None else (gaussians.get_scaling, False)
    return s.detach().float().contiguous(), raw


@torch.no_grad()
def volume_of(scaling, raw=False):
    """``torch.prod(scaling, dim=1)`` of a [P,3] float32 tensor; raw=True: of exp(scaling), the exp taken in the kernel"""
    _require_gpu("volume_of", scaling)
    if scaling.dim() != 2 or scaling.shape[1] != 3 or scaling.dtype != torch.float32:
        raise ValueError(f"volume_of: expected float32 [P,3], got {scaling.dtype} {list(scaling.shape)}")
    s = scaling.detach().contiguous()
    P = s.shape[0]
    vol = torch.empty(P, dtype=torch.float32, device=s.device)
    if P:
        with torch.cuda.device(s.device):
            _check(_native.load().fr_volume(P, s.data_ptr(), int(bool(raw)), vol.data_ptr(), _stream(s.device)), "volume")
    return vol


@torch.no_grad()
def calculate_v_imp_score(gaussians, imp_list, v_pow, scaling=None, raw=False):
    """The reference's calculate_v_imp_score (prune.py:112-128): ``(volume / kth_percent_largest) ** v_pow * imp_list`` with
    volume = prod(get_scaling, dim=1) and kth_percent_largest = the element int(P * 0.9) of the descending order. scaling / raw
    (extension): the [P,3] scales to use instead of the model's (raw=True: log-scales). No host synchronisation."""
    if scaling is None:
        scaling, raw = _scaling_of(gaussians)
    imp, P = _values(imp_list, "calculate_v_imp_score")
    if imp.dtype != torch.float32:
        raise ValueError(f"calculate_v_imp_score: imp_list must be float32, got {imp.dtype}")
    vol = volume_of(scaling, raw)
    if vol.shape[0] != P:
        raise ValueError(f"calculate_v_imp_score: {vol.shape[0]} Gaussians, {P} scores")
    if P == 0:
        return vol
    kth = kth_value(vol, volume_index(P))
    with torch.cuda.device(vol.device):
        rc = _native.load().fr_v_importance(P, vol.data_ptr(), kth.data_ptr(), float(v_pow), imp.data_ptr(), vol.data_ptr(), _stream(vol.device))
    _check(rc, "v_importance")
    return vol


@torch.no_grad()
def prune_gaussians(model, percent, import_score):
    """GaussianModel.prune_gaussians (gaussian_model.py:776-782): cuts the rows whose score is <= the score of rank
    int(percent * (P - 1)). The compaction plan's count readback is the only host synchronisation. Returns the mask."""
    mask = percentile_mask(import_score, percent)
    pruning.prune_points(model, mask)
    return mask


def prune_opacity(model, percent):
    """prune_gaussians by the activated opacity (prune_finetune.py:238-242)"""
    opacity = model.get_opacity if hasattr(model, "get_opacity") else torch.sigmoid(model._opacity)
    return prune_gaussians(model, percent, opacity.detach().float())


def global_significance_prune(model, cameras, pipe, bg, percent, prune_type="v_important_score", v_pow=0.1):
    """The prune step of prune_finetune.py:214-242: prune_list over `cameras`, the score of `prune_type` -- "important_score",
    "v_important_score" (the MMFR models: v_pow 0.1), "max_v_important_score", "count" or "opacity" -- and prune_gaussians at
    `percent`. Returns the mask that was cut (bool [P], True = pruned)."""
    if prune_type not in PRUNE_TYPES:
        raise ValueError(f"unknown prune_type {prune_type!r} (expected one of {PRUNE_TYPES})")
    gaussian_list, imp_list = prune_list(model, cameras, pipe, bg)
    if prune_type == "important_score":
        score = imp_list
    elif prune_type == "v_important_score":
        score = calculate_v_imp_score(model, imp_list, v_pow)
    elif prune_type == "max_v_important_score":
        score = imp_list * torch.max(model.get_scaling.detach(), dim=1)[0]
    elif prune_type == "count":
        score = gaussian_list
    else:
        return prune_opacity(model, percent)
    return prune_gaussians(model, percent, score)
