"""Drop-in for the reference package LightGaussian/submodules/compress-diff-gaussian-rasterization/
compress_diff_gaussian_rasterization/__init__.py: the vanilla rasterizer plus the counting render of the global-significance
pruning (`f_count`).

Same public names: GaussianRasterizationSettings (the reference's twelve fields and `f_count`), GaussianRasterizer,
rasterize_gaussians. Without f_count the module IS the "original" rasterizer (diff_gaussian_rasterization): forward returns
(color, radii) with the full backward pass. With f_count forward returns (gaussians_count, important_score, color, radii)
(reference :135-136, :248-346) and builds no autograd node -- the reference's forward_count is a static call outside autograd.

gaussians_count [P] int32 and important_score [P] float32 are the exact values of the statements the reference executes
racily (include/fovraster.h, fr_forward_args.gaussians_count): hits of every Gaussian, and hits * opacity rounded once.
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from .. import _native
from ..rasterizer import _forward_begin, _make_plain, _mark_visible, _raster_output


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    f_count: bool = False


_RasterizeGaussians, _rasterize_plain, _PlainRasterizer = _make_plain(_native.VARIANT_ORIGINAL, with_counts=False, has_backward=True)


@torch.no_grad()
def _rasterize_count(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, sh_rest=None,
                     packed=None, raw_activations=False):
    """-> (gaussians_count, important_score, color, radii): one counting call on the current stream, no autograd node"""
    frame = _forward_begin(_native.VARIANT_ORIGINAL, raster_settings, means3D, sh, colors_precomp, opacities, scales, rotations,
                           cov3Ds_precomp, persistent=True, sh_rest=sh_rest, packed=packed, raw_activations=raw_activations, count=True)
    res = frame.finish()
    return res[6], res[7], res[1], res[2]


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
    if raster_settings.f_count:
        return _rasterize_count(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings)
    return _rasterize_plain(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings
        self._plain = _PlainRasterizer(raster_settings)

    def markVisible(self, positions):
        with torch.no_grad():
            return _mark_visible(positions, self.raster_settings)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None,
                packed=None, raw_activations=False):
        """packed / raw_activations / shs as the pair (features_dc, features_rest): this package's extensions, as in
        diff_gaussian_rasterization."""
        rs = self.raster_settings
        if not rs.f_count:
            return self._plain(means3D, means2D, opacities, shs=shs, colors_precomp=colors_precomp, scales=scales, rotations=rotations,
                               cov3D_precomp=cov3D_precomp, packed=packed, raw_activations=raw_activations)
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        if raw_activations and (cov3D_precomp is not None or packed is not None):
            raise Exception('raw_activations needs the scale/rotation pair and no packed model')
        shs_rest = None
        if isinstance(shs, (tuple, list)):
            shs, shs_rest = shs
            if shs_rest is not None and shs_rest.numel() == 0:
                shs_rest = None
        counts, score, color, radii = _rasterize_count(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, rs,
                                                       sh_rest=shs_rest, packed=packed, raw_activations=raw_activations)
        out = _raster_output((color, radii))
        res = _CountOutput((counts, score, color, radii))
        res.visibility_filter = out.visibility_filter
        return res


class _CountOutput(tuple):
    """(gaussians_count, important_score, color, radii) with visibility_filter beside it (rasterizer.RasterOutput)"""
    visibility_filter = None
