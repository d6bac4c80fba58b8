"""Drop-in for the reference package
fov3dgs/submodules/diff-gaussian-rasterization_fov_pcheck_obb/diff_gaussian_rasterization_fov_pcheck_obb/__init__.py
(the foveated rasterizer behind gaussian_renderer_fov.render(): inference-only as the reference's, and -- extension --
differentiable in the per-level opacities and DC colours with GaussianRasterizer.forward(..., appearance_only=True)).
"""
from ..rasterizer import FoveationSettings, GaussianRasterizationSettings, _make_fov  # noqa: F401

_RasterizeGaussians, rasterize_gaussians, GaussianRasterizer = _make_fov()
