"""Foveation settings (include/fovraster.h: fr_foveation; rasterizer.FoveationSettings), the parts that need no GPU: the struct's
layout, what the library refuses before anything runs, the shape checks of the host layer, a library built before the settings,
and the level map's geometry against the reference's own pooling-size map for display geometries other than the default."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, ROOT
from tests import foveation_helpers as fh
from fov3dgs_amd import _native, rasterizer
from fov3dgs_amd.rasterizer import FoveationSettings


def _fov(levels=4, mps=12.0, riw=2.0, rvd=1.0, sb=0.5, bw=0.5, size=None):
    return _native.Foveation(C.sizeof(_native.Foveation) if size is None else size, levels, mps, riw, rvd, sb, bw)


def test_foveation_matches_the_c_layout(tmp_path):
    fields = [f[0] for f in _native.Foveation._fields_]
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/fovraster.h"', 'int main(){',
            'printf("%zu\\n", sizeof(fr_foveation));']
    body += [f'printf("%zu\\n", offsetof(fr_foveation, {f}));' for f in fields]
    body += ['return 0;}']
    src, exe = tmp_path / "layout_fov.c", tmp_path / "layout_fov"
    src.write_text("\n".join(body))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert nums[0] == C.sizeof(_native.Foveation) == 28
    assert fields == ["size", "levels", "max_pooling_size", "real_image_width", "real_viewing_distance", "start_blend", "blend_width"]
    for f, off in zip(fields, nums[1:]):
        assert getattr(_native.Foveation, f).offset == off, f
    lib = _native.load()
    assert lib.fr_abi_version() == _native.ABI_VERSION == 12  # (added symbols: fr_forward_args / fr_forward_ext as they were)
    assert _native.has_foveation(lib) and _native.has_forward_ext(lib)
    for name in _native.FOVEATION_EXPORTS:
        assert name in _native.EXPORTS and name in _native.OPTIONAL_EXPORTS and hasattr(lib, name), name
    # the settings record's defaults are the reference's constants
    assert FoveationSettings() == (4, 12.0, 2.0, 1.0, 0.5, 0.5)
    from fov3dgs_amd import diff_gaussian_rasterization_fov_pcheck_obb as pkg
    assert pkg.FoveationSettings is FoveationSettings is rasterizer.FoveationSettings


def _empty_args(variant=_native.VARIANT_FOV_PCHECK_OBB):
    """a hand-filled call that passes the argument checks and would only clear a 16 x 16 image (P = 0) -- at address 1: it
    must be refused before anything runs"""
    a = _native.ForwardArgs()
    a.variant, a.P, a.W, a.H, a.out_color = variant, 0, 16, 16, 1
    return a


@pytest.mark.parametrize("fov,field", [
    (dict(levels=1), b"levels"), (dict(levels=9), b"levels"), (dict(mps=1.0), b"max_pooling_size"),
    (dict(mps=float("nan")), b"max_pooling_size"), (dict(riw=float("nan")), b"real_image_width"), (dict(riw=0.0), b"real_image_width"),
    (dict(rvd=float("inf")), b"real_viewing_distance"), (dict(rvd=-1.0), b"real_viewing_distance"),
    (dict(sb=0.0), b"start_blend"), (dict(sb=1.0), b"start_blend"), (dict(sb=float("nan")), b"start_blend"),
    (dict(bw=0.0), b"blend_width"), (dict(bw=float("nan")), b"blend_width"), (dict(size=4), b"fr_foveation.size")])
def test_invalid_settings_are_refused_before_anything_runs(fov, field):
    lib = _native.load()
    f = _fov(**fov)
    a = _empty_args()
    assert lib.fr_forward_fov_call(C.byref(a), None, C.byref(f)) == -1
    err = lib.fr_last_error()
    assert field in err and b"fr_foveation" in err, err
    handle = C.c_void_p()
    assert lib.fr_forward_begin_fov(C.byref(a), None, C.byref(f), C.byref(handle)) == -1 and not handle.value
    assert field in lib.fr_last_error()


def test_settings_are_refused_with_any_other_variant():
    lib = _native.load()
    f = _fov()
    for variant in (_native.VARIANT_PCHECK_OBB_SUM, _native.VARIANT_NAIVE_FOV_PCHECK_OBB, _native.VARIANT_MMFR_PCHECK_OBB):
        a = _empty_args(variant)
        assert lib.fr_forward_fov_call(C.byref(a), None, C.byref(f)) == -1
        assert b"fr_foveation" in lib.fr_last_error() and b"variant" in lib.fr_last_error()
    # the levels-aware sizes: behind everything a call without settings keeps, and refused outside 2 .. 8
    P = 1000
    g4 = lib.fr_geometry_bytes(3, P)
    assert lib.fr_geometry_bytes_fov(3, P, 4) == g4
    assert lib.fr_geometry_bytes_fov(3, P, 8) == g4 + 64 * P                       # the rows of the levels 4 .. 7
    assert 0 <= lib.fr_geometry_bytes_fov(3, P, 3) - (g4 + 16 * P + 48 * P) < 512   # the four-wide copies of [P,3] / [P,3,3] (256-byte aligned)
    assert lib.fr_geometry_bytes_fov(3, P, 6) >= g4 + 64 * P + 32 * P + 96 * P     # ... rows and eight-wide copies (256-byte aligned)
    assert lib.fr_geometry_bytes_fov(2, P, 6) == lib.fr_geometry_bytes(2, P)        # (no other variant has level rows)
    assert lib.fr_geometry_bytes_fov(3, P, 1) == 0 and lib.fr_geometry_bytes_fov(3, P, 9) == 0
    assert lib.fr_geometry_level_colours_hi(P, 4, 4096) is None
    hi = lib.fr_geometry_level_colours_hi(P, 6, 4096)
    assert hi is not None and hi >= 4096 + g4 - 256


def test_null_settings_are_the_old_entry_points():
    """fov == NULL: fr_forward_begin_ext / fr_forward_ext_call -- the same refusals with the same words, before anything runs"""
    lib = _native.load()
    a = _native.ForwardArgs()
    a.variant = 8
    handle = C.c_void_p()
    assert lib.fr_forward_ext_call(C.byref(a), None) == -1
    want = lib.fr_last_error()
    assert b"variant" in want
    assert lib.fr_forward_fov_call(C.byref(a), None, None) == -1 and lib.fr_last_error() == want
    assert lib.fr_forward_begin_fov(C.byref(a), None, None, C.byref(handle)) == -1 and not handle.value
    # a bad variant is reported before the settings are looked at, a short fr_forward_ext too
    assert lib.fr_forward_fov_call(C.byref(a), None, C.byref(_fov(levels=9))) == -1 and lib.fr_last_error() == want
    a = _empty_args()
    ext = _native.ForwardExt(4, None)
    assert lib.fr_forward_fov_call(C.byref(a), C.byref(ext), C.byref(_fov())) == -1 and b"fr_forward_ext.size" in lib.fr_last_error()


class _Raster:
    image_height, image_width, sh_degree, tanfovx, tanfovy, scale_modifier, prefiltered, debug = 32, 32, 3, 1.0, 1.0, 1.0, False, False


def _model(P, L):
    return dict(means3D=torch.zeros(P, 3), sh=torch.zeros(P, 15, 3), opacities=torch.ones(P, L), scales=torch.ones(P, 3),
                rotations=torch.ones(P, 4), shs_dcs=torch.zeros(P, L, 3), highest_levels=torch.zeros(P, 1))


def _begin(m, monkeypatch, foveation=None, packed=None):
    """_forward_begin on CPU tensors, up to where it would need the GPU: the shape checks come first"""
    monkeypatch.setattr(rasterizer, "_require_gpu", lambda t: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type("Stream", (), {"cuda_stream": 0})())
    return rasterizer._forward_begin(_native.VARIANT_FOV_PCHECK_OBB, _Raster(), m["means3D"], m["sh"], None, m["opacities"], m["scales"],
                                     m["rotations"], None, m["shs_dcs"], m["highest_levels"], foveation=foveation, packed=packed)


def test_a_model_of_another_width_is_refused_not_misread(monkeypatch):
    with pytest.raises(RuntimeError, match=r"opacities.*\b3 level.*renders 4 levels"):
        _begin(_model(5, 3), monkeypatch)
    with pytest.raises(RuntimeError, match=r"opacities.*\b4 level.*renders 3 levels"):
        _begin(_model(5, 4), monkeypatch, FoveationSettings(levels=3))
    with pytest.raises(RuntimeError, match=r"opacities.*\b5 level.*renders 4 levels"):
        _begin(_model(5, 5), monkeypatch, FoveationSettings())
    m = _model(5, 6)
    m["shs_dcs"] = torch.zeros(5, 4, 3)
    with pytest.raises(RuntimeError, match=r"shs_dcs.*\b4 level.*renders 6 levels"):
        _begin(m, monkeypatch, FoveationSettings(levels=6))
    # a packed copy made from another number of layers
    pk = rasterizer.PackedModel(torch.zeros(5, 16), torch.zeros(5, 64), torch.zeros(5, 4), levels=4)
    with pytest.raises(RuntimeError, match=r"packed model.*4 levels.*renders 3"):
        _begin(_model(5, 3), monkeypatch, FoveationSettings(levels=3), packed=pk)
    # settings with another rasterizer
    with pytest.raises(RuntimeError, match="foveated rasterizer"):
        rasterizer._forward_begin(_native.VARIANT_PCHECK_OBB, _Raster(), torch.zeros(2, 3), torch.zeros(2, 16, 3), None, torch.ones(2, 1),
                                  torch.ones(2, 3), torch.ones(2, 4), None, foveation=FoveationSettings())
    # the settings as the reuse key and the struct see them
    assert rasterizer._foveation_key(None) is None
    assert rasterizer._foveation_key(FoveationSettings(levels=6, real_image_width=1)) == (6, 12.0, 1.0, 1.0, 0.5, 0.5)
    assert rasterizer._foveation_key((3, 9, 2, 1, 0.4, 0.6)) == (3, 9.0, 2.0, 1.0, 0.4, 0.6)
    f = rasterizer._foveation_struct(_native.load(), (6, 16.0, 1.6, 0.8, 0.5, 0.5))
    assert (f.size, f.levels) == (28, 6) and math.isclose(f.real_image_width, 1.6, rel_tol=1e-6) and math.isclose(f.max_pooling_size, 16.0)


class _OldLibrary:
    """The loaded library as one built before the foveation settings: every attribute but the new entry points."""

    def __init__(self, lib, calls=None):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        if name in _native.FOVEATION_EXPORTS:
            raise AttributeError(name)
        if name == "fr_forward_begin_ext" and self._calls is not None:
            return lambda a, ext, handle: self._calls.append(name) or -1  # (no GPU here: refused once the entry point is known)
        return getattr(self._lib, name)


def test_a_library_without_the_settings_loads_serves_none_and_refuses_the_rest(monkeypatch):
    real = _native.load()
    old = _OldLibrary(real)
    assert not _native.has_foveation(old) and _native.has_forward_ext(old)  # (the visibility output does not depend on the new names)
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native.C, "CDLL", lambda path: old)
    try:
        assert _native.load() is old
    finally:
        monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.undo()
    assert _native.load() is real
    # non-default settings: refused, never ignored; no settings and the defaults spelled out: today's entry point
    with pytest.raises(RuntimeError, match="no foveation settings"):
        rasterizer._foveation_struct(old, rasterizer._foveation_key(FoveationSettings(levels=3)))
    with pytest.raises(RuntimeError, match="no foveation settings"):
        rasterizer._foveation_struct(old, rasterizer._foveation_key(FoveationSettings(real_viewing_distance=0.8)))
    assert rasterizer._foveation_struct(old, None) is None
    assert rasterizer._foveation_struct(old, rasterizer._foveation_key(FoveationSettings())) is None
    calls = []
    old = _OldLibrary(real, calls)
    radii = torch.zeros(4, dtype=torch.int32)
    assert rasterizer._begin_call(old, _native.ForwardArgs(), 4, radii.device, radii, C.c_void_p(), None) == -1
    assert calls == ["fr_forward_begin_ext"]


def test_pack_model_refuses_more_than_four_levels(monkeypatch):
    monkeypatch.setattr(rasterizer, "_require_gpu", lambda t: None)
    with pytest.raises(RuntimeError, match="at most 4 levels.*has 6"):
        rasterizer.pack_model(torch.zeros(2, 3), torch.ones(2, 3), torch.ones(2, 4), torch.ones(2, 6), shs=torch.zeros(2, 15, 3),
                              shs_dcs=torch.zeros(2, 6, 3), highest_levels=torch.zeros(2, 1))


def test_level_map_geometry_matches_the_reference_pooling_map(monkeypatch):
    """The reference's own pooling-size map (odak make_pooling_size_map_pixels, tests/golden/make_golden_foveation.py) at 1280x720
    for three display geometries and layer counts other than the default, turned into levels with each setting's step and cap,
    against the derivation under the same constants: the figure of the existing pin at the default geometry (4e-3 of a level:
    odak samples linspace(-0.5, 0.5, W), the rasterizer (x + 8) / W)."""
    g = np.load(os.path.join(GOLDEN, "ref_pooling_geometry.npz"))
    W, H = [int(x) for x in g["size"]]
    inside = g["inside"].reshape(-1)
    assert len(g["cases"]) == 3
    for ci, (L, mps, riw, rvd, gx, gy, alpha) in enumerate(g["cases"]):
        s = FoveationSettings(int(L), float(mps), float(riw), float(rvd))
        assert s[:4] in ((6, 16.0, 1.6, 0.8), (3, 9.0, 2.4, 1.5), (8, 25.0, 1.2, 1.0))
        cam = dict(image_width=W, image_height=H, tanfovx=1.0, tanfovy=1.0, bg=np.zeros(3), viewmatrix=np.eye(4), projmatrix=np.eye(4),
                   campos=np.zeros(3), sh_degree=3, gaze=(float(gx), float(gy)), alpha=float(alpha))
        lv = fh.level_map(monkeypatch, s, cam)["tile_levels"]
        step, cap = (float(v) for v in fh.step_and_cap(s))
        ps = g[f"ps{ci}"].astype(np.float64).reshape(-1)
        want = np.minimum(np.where(ps <= 1, 0.0, (np.sqrt(np.maximum(ps, 1e-30)) - 1) / step), cap)
        np.testing.assert_allclose(lv[inside], want[inside], atol=4e-3, err_msg=f"setting {s}")
        assert sorted(np.unique(np.floor(lv[inside]).astype(int))) == list(range(s.levels)), s
