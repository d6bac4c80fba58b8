"""The gradient side of tests/lpips_cases.py: per case, once per session, the float64 gradient of tests/lpips_ref.py's value with
respect to x (torch.autograd, the picture's own decisions), the float32 one, and both pictures' 13 post-ReLU maps in float64.
Shared by test_lpips_backward_cpu.py and test_lpips_backward_gpu.py; the tests must leave them unchanged.

Yardsticks, measured on the CPU over the six cases (test_lpips_backward_cpu.py re-measures them on every run and records them):
  GRAD_YARDSTICK     the float32 autograd gradient's largest |g - g64| / (|g64| + rms(g64)) against the float64 gradient frozen to
                     float32's decisions (lpips_cases.feature_ratio): 3.38e-5 (seams)
  GRAD_L2_YARDSTICK  its largest |g - g64|_2 / |g64|_2: 8.0e-6 (35x50)
  ACT_YARDSTICK      the float32 restatement's largest feature_ratio over all 13 post-ReLU maps (lpips_cases.FEAT_YARDSTICK covers
                     the five taps only): 3.74e-6 (seams)
The HIP path gets lpips_cases.MARGIN = 4 on each, for the reason given there: MFMA chains add in another order than torch's CPU
kernels."""
import functools

import torch

from tests import lpips_cases, lpips_grad_ref

GRAD_YARDSTICK = 3.38e-5
GRAD_L2_YARDSTICK = 8.0e-6
ACT_YARDSTICK = 3.74e-6  # measured 3.740e-6 (seams)
GRAD_RTOL = lpips_cases.MARGIN * GRAD_YARDSTICK
GRAD_L2_RTOL = lpips_cases.MARGIN * GRAD_L2_YARDSTICK
ACT_RTOL = lpips_cases.MARGIN * ACT_YARDSTICK


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(x, y, value64, grad64, maps64 (x's 13 maps), ymaps64, value32, grad32, maps32)"""
    c = lpips_cases.case(name)
    w = lpips_cases.weights()
    v64, g64, m64 = lpips_grad_ref.lpips_grad(c["x"], c["y"], w, torch.float64)
    v32, g32, m32 = lpips_grad_ref.lpips_grad(c["x"], c["y"], w, torch.float32)
    with torch.no_grad():
        ym64 = lpips_grad_ref.activations(c["y"], w["features"], torch.float64)
    return dict(x=c["x"], y=c["y"], value64=v64, grad64=g64, maps64=m64, ymaps64=ym64, value32=v32, grad32=g32, maps32=m32)


def frozen64(x, y, x_maps, name=None):
    """the float64 value and gradient with x's decisions frozen to `x_maps`; y keeps its own float64 decisions (its branch carries
    no gradient). `name`: a case whose y maps are at hand."""
    w = lpips_cases.weights()
    y_maps = case(name)["ymaps64"] if name is not None else None
    v, g, _ = lpips_grad_ref.lpips_grad(x, y, w, torch.float64, [m.cpu() for m in x_maps], y_maps)
    return v, g


def grad_ratio(got, g64):
    """the largest |got - g64| / (|g64| + rms(g64)) over the gradient: lpips_cases.feature_ratio"""
    return lpips_cases.feature_ratio(got, g64)


def grad_l2(got, g64):
    g64 = g64.double()
    return float((got.double() - g64).norm() / g64.norm())
