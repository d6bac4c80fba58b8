"""Depth and coverage outputs (include/fovraster.h: fr_forward_aux), the parts that need no GPU: the reference helper
(tests/depth_ref.py) pinned to the C oracle and to the numpy derivation through a depth-as-colour render, the struct's layout, what
the library refuses before anything runs, and the refusals of the Python layer."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import depth_ref as D
from tests import fov_backward_ref as R
from tests import fov_backward_scenes as fs
from tests import foveation_helpers as fh
from tests.helpers import ROOT, small_case
from fov3dgs_amd import _native, rasterizer
from fov3dgs_amd.rasterizer import FoveationSettings

# The helper against the oracle's own blend: 1e-5 on depth / zmax and on coverage. The float32-versus-float64 difference of the
# helper's arithmetic on these frames is <= 4.5e-7 (depth / zmax) and <= 8.1e-7 (coverage); the oracle's image carries the rounding of
# the colour c = SH_C0 dc + 0.5 (1e-7) besides. The bound is more than an order above that and an order below the parity bound (1e-4).
PIN = 1e-5
L6 = (FoveationSettings(6, 16.0, 1.6, 0.8, 0.5, 0.5), 0.6, (0.3, 0.4))   # the levels=6 frame: foveation_helpers.fov_case at 200 x 120
MIN_TWO_LEVEL_TILES = 8
_empty_share = {}


def _pin(tag, image, ref, depths, zmax):
    d64, c64 = D.outputs(ref, depths)
    d32, c32 = D.outputs(ref, depths, np.float32)
    err_d, err_c = np.abs(image[0] - d64 / zmax).max(), np.abs(image[1] - c64).max()
    print(tag, "two-level tiles", D.two_level_tiles(ref), "| depth/zmax: oracle vs helper", err_d, "f32 vs f64", np.abs(d32 - d64).max() / zmax,
          "| coverage: oracle vs helper", err_c, "f32 vs f64", np.abs(c32 - c64).max(), "| empty pixels", float((c64 == 0).mean()),
          "| partly covered", float(((c64 > 0.05) & (c64 < 0.95)).mean()))
    assert D.two_level_tiles(ref) >= MIN_TWO_LEVEL_TILES   # (a frame without two-level tiles would not judge the mix of the two states)
    assert (c64 > 0).mean() > 0.5 and (d64 > 0).mean() > 0.5
    assert np.all(image[2] == 0)
    assert err_d <= PIN and err_c <= PIN
    assert np.all(d64[c64 == 0] == 0)
    _empty_share[tag] = float((c64 == 0).mean())


@pytest.mark.parametrize("kw", R.PARITY, ids=lambda k: f"a{k['alpha']}-g{k['gaze'][0]}-{k['gaze'][1]}-w{k.get('width', 200)}")
def test_the_helper_is_the_oracles_blend_with_depth_as_colour(kw):
    """Zero rest SH, black background, every level's DC set so that the level colour is (z / zmax, 1, 0): lists and opacities are the
    frame's, so the decisions are; the oracle image's channel 0 times zmax is then the depth, channel 1 the sum of the weights."""
    scene, cam, fwd, ref, _ = R.case(**kw)
    zmax = D.zmax_of(fwd)
    s2, c2 = dict(scene), dict(cam)
    s2["shs"] = np.zeros_like(scene["shs"])
    s2["shs_dcs"] = np.repeat(D.dc_of_colour(D.depth_as_colour(fwd["depths"], zmax))[:, None, :], 4, axis=1)
    c2["bg"] = np.zeros(3, np.float32)
    img = orc.forward("fov_pcheck_obb", s2, c2)
    assert np.array_equal(img["point_list"], fwd["point_list"]) and np.array_equal(img["ranges"], fwd["ranges"])
    _pin(f"parity {kw}", img["color"], ref, fwd["depths"], zmax)


def test_the_helper_with_six_levels_against_the_derivation():
    settings, alpha, gaze = L6
    scene, cam = fh.fov_case(settings, alpha, gaze, width=200, height=120, bg=(0.0, 0.0, 0.0))
    fwd = fs.forward(scene, cam, settings)
    ref = fs.make_ref(fwd, scene, cam, settings)
    zmax = D.zmax_of(fwd)
    s2 = dict(scene)
    s2["shs"] = np.zeros_like(scene["shs"])
    s2["shs_dcs"] = np.repeat(D.dc_of_colour(D.depth_as_colour(fwd["depths"], zmax))[:, None, :], 6, axis=1)
    img = fs.forward(s2, cam, settings)
    assert np.array_equal(img["point_list"], fwd["point_list"]) and np.array_equal(img["ranges"], fwd["ranges"])
    assert max(st["lev"] for tl in ref.tiles for st in tl["states"] if st["acc"].any()) >= 4   # (levels the second row of level colours holds)
    _pin("L6", np.asarray(img["color"]), ref, fwd["depths"], zmax)


def test_one_of_the_frames_has_empty_pixels():
    """(after the frames above: a degenerate scene -- every pixel covered -- cannot pass the "exactly 0 where nothing lands" checks silently)"""
    if len(_empty_share) < len(R.PARITY):
        for kw in R.PARITY:
            scene, cam, fwd, ref, _ = R.case(**kw)
            _empty_share[f"parity {kw}"] = float((D.outputs(ref, fwd["depths"])[1] == 0).mean())
    assert max(_empty_share.values()) >= 0.01, _empty_share


@pytest.mark.parametrize("size", ((200, 120), (203, 131)))
def test_the_one_state_helper_is_the_oracles_pcheck_obb_blend(size):
    scene, cam = small_case("pcheck_obb", width=size[0], height=size[1])
    fwd = orc.forward("pcheck_obb", scene, cam)
    ref = D.plain_ref(fwd, scene, cam)
    zmax = D.zmax_of(fwd)
    # the helper's image is the oracle's: the restatement blends the oracle's pairs
    assert np.abs(ref.image(dtype=np.float32) - fwd["color"]).max() <= PIN
    s2, c2 = dict(scene), dict(cam)
    s2["shs"] = np.zeros_like(scene["shs"])
    s2["shs"][:, 0, :] = D.dc_of_colour(D.depth_as_colour(fwd["depths"], zmax))
    c2["bg"] = np.zeros(3, np.float32)
    img = orc.forward("pcheck_obb", s2, c2)
    assert np.array_equal(img["point_list"], fwd["point_list"])
    d64, c64 = D.outputs(ref, fwd["depths"])
    err_d, err_c = np.abs(img["color"][0] - d64 / zmax).max(), np.abs(img["color"][1] - c64).max()
    print("pcheck_obb", size, "depth/zmax", err_d, "coverage", err_c, "empty", float((c64 == 0).mean()))
    assert err_d <= PIN and err_c <= PIN and (c64 > 0).mean() > 0.5


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_forward_aux_matches_the_c_layout(tmp_path):
    fields = [f[0] for f in _native.ForwardAux._fields_]
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/fovraster.h"', 'int main(){',
            'printf("%zu\\n", sizeof(fr_forward_aux));', 'printf("%zu\\n", sizeof(fr_forward_args));', 'printf("%zu\\n", sizeof(fr_forward_ext));']
    body += [f'printf("%zu\\n", offsetof(fr_forward_aux, {f}));' for f in fields]
    body += ['return 0;}']
    src, exe = tmp_path / "layout_aux.c", tmp_path / "layout_aux"
    src.write_text("\n".join(body))
    subprocess.check_call(["cc", "-o", str(exe), str(src)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert nums[0] == C.sizeof(_native.ForwardAux) == 24
    assert nums[1] == C.sizeof(_native.ForwardArgs) == 352 and nums[2] == C.sizeof(_native.ForwardExt) == 16
    assert fields == ["size", "depth", "coverage"]
    for f, off in zip(fields, nums[3:]):
        assert getattr(_native.ForwardAux, f).offset == off, f
    lib = _native.load()
    assert lib.fr_abi_version() == _native.ABI_VERSION == 12
    assert _native.has_forward_aux(lib)
    for name in _native.FORWARD_AUX_EXPORTS:
        assert name in _native.EXPORTS and name in _native.OPTIONAL_EXPORTS and hasattr(lib, name), name


def _empty_args(variant=_native.VARIANT_FOV_PCHECK_OBB):
    """a hand-filled call that passes the argument checks and would only clear a 16 x 16 image (P = 0) -- at address 1: it must be
    refused before anything runs"""
    a = _native.ForwardArgs()
    a.variant, a.P, a.W, a.H, a.out_color = variant, 0, 16, 16, 1
    return a


def _aux(size=None, depth=1, coverage=1):
    return _native.ForwardAux(C.sizeof(_native.ForwardAux) if size is None else size, depth, coverage)


@pytest.mark.parametrize("variant,aux,words", [
    (_native.VARIANT_FOV_PCHECK_OBB, dict(size=8), (b"fr_forward_aux.size", b"8")),
    (_native.VARIANT_PCHECK_OBB, dict(size=0), (b"fr_forward_aux.size",)),
    (_native.VARIANT_FOV_PCHECK_OBB, dict(coverage=None), (b"go together", b"only depth")),
    (_native.VARIANT_PCHECK_OBB, dict(depth=None), (b"go together", b"only coverage")),
    (_native.VARIANT_ORIGINAL, dict(), (b"fr_forward_aux", b"variant 0")),
    (_native.VARIANT_PCHECK_OBB_SUM, dict(), (b"fr_forward_aux", b"variant 1")),
    (_native.VARIANT_NAIVE_FOV_PCHECK_OBB, dict(), (b"fr_forward_aux", b"variant 6")),
    (_native.VARIANT_MMFR_PCHECK_OBB, dict(), (b"fr_forward_aux", b"variant 7"))])
def test_bad_aux_structs_are_refused_before_anything_runs(variant, aux, words):
    lib = _native.load()
    a, x = _empty_args(variant), _aux(**aux)
    assert lib.fr_forward_aux_call(C.byref(a), None, None, C.byref(x)) == -1
    err = lib.fr_last_error()
    assert all(w in err for w in words), err
    handle = C.c_void_p()
    assert lib.fr_forward_begin_aux(C.byref(a), None, None, C.byref(x), C.byref(handle)) == -1 and not handle.value
    assert all(w in lib.fr_last_error() for w in words)


def test_null_aux_is_the_old_entry_points():
    """aux == NULL: fr_forward_begin_fov / fr_forward_fov_call -- the same refusals with the same words, before anything runs; and the
    old refusals come before the new struct is looked at"""
    lib = _native.load()
    a = _native.ForwardArgs()
    a.variant = 8
    handle = C.c_void_p()
    assert lib.fr_forward_fov_call(C.byref(a), None, None) == -1
    want = lib.fr_last_error()
    assert b"variant" in want
    assert lib.fr_forward_aux_call(C.byref(a), None, None, None) == -1 and lib.fr_last_error() == want
    assert lib.fr_forward_begin_aux(C.byref(a), None, None, None, C.byref(handle)) == -1 and not handle.value
    assert lib.fr_forward_aux_call(C.byref(a), None, None, C.byref(_aux(size=4))) == -1 and lib.fr_last_error() == want
    # settings with another variant and a short fr_forward_ext are refused as they were, with or without the outputs
    a = _empty_args(_native.VARIANT_PCHECK_OBB)
    fov = _native.Foveation(C.sizeof(_native.Foveation), 4, 12.0, 2.0, 1.0, 0.5, 0.5)
    assert lib.fr_forward_aux_call(C.byref(a), None, C.byref(fov), None) == -1 and b"fr_foveation" in lib.fr_last_error()
    assert lib.fr_forward_aux_call(C.byref(a), None, C.byref(fov), C.byref(_aux())) == -1 and b"fr_foveation" in lib.fr_last_error()
    ext = _native.ForwardExt(4, None)
    assert lib.fr_forward_aux_call(C.byref(_empty_args()), C.byref(ext), None, C.byref(_aux())) == -1 and b"fr_forward_ext.size" in lib.fr_last_error()
    bad = _native.Foveation(C.sizeof(_native.Foveation), 9, 12.0, 2.0, 1.0, 0.5, 0.5)
    assert lib.fr_forward_aux_call(C.byref(_empty_args()), None, C.byref(bad), C.byref(_aux())) == -1 and b"levels" in lib.fr_last_error()


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
class _Raster:
    image_height, image_width, sh_degree, tanfovx, tanfovy, scale_modifier, prefiltered, debug = 32, 32, 3, 1.0, 1.0, 1.0, False, False
    bg, viewmatrix, projmatrix, campos = torch.zeros(3), torch.eye(4), torch.eye(4), torch.zeros(3)


class _OldLibrary:
    """The loaded library as one built before the depth / coverage outputs: every attribute but the new entry points."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in _native.FORWARD_AUX_EXPORTS:
            raise AttributeError(name)
        return getattr(self._lib, name)


def test_a_library_without_the_outputs_loads_and_refuses_want_depth(monkeypatch):
    real = _native.load()
    old = _OldLibrary(real)
    assert not _native.has_forward_aux(old) and _native.has_forward_ext(old) and _native.has_foveation(old)
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native.C, "CDLL", lambda path: old)
    try:
        assert _native.load() is old   # (the two names are optional exports)
    finally:
        monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.undo()
    assert _native.load() is real
    radii = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="rebuild"):
        rasterizer._aux_planes(old, radii, 16, 16, radii.device)
    assert rasterizer.depth_of(radii) == (None, None)
    # through the call itself, up to where it would need the GPU
    monkeypatch.setattr(rasterizer, "_require_gpu", lambda t: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type("Stream", (), {"cuda_stream": 0})())
    monkeypatch.setattr(_native, "load", lambda: old)

    with pytest.raises(RuntimeError, match="rebuild"):
        rasterizer._forward_begin(_native.VARIANT_PCHECK_OBB, _Raster(), torch.zeros(2, 3), torch.zeros(2, 16, 3), None, torch.ones(2, 1),
                                  torch.ones(2, 3), torch.ones(2, 4), None, want_depth=True)


def test_want_depth_is_refused_where_it_has_no_meaning(monkeypatch):
    from fov3dgs_amd.gaussian_renderer import render
    from fov3dgs_amd.gaussian_renderer_fov import render as render_fov
    pc = type("Model", (), {"get_xyz": torch.zeros(1, 3)})()
    for kw in (dict(appearance_only=True), dict(differentiable=True)):
        with pytest.raises(ValueError, match="want_depth.*inference frame"):
            render_fov(None, pc, torch.zeros(3), alpha=0.05, gazeArray=(0.5, 0.5), want_depth=True, **kw)
    for cuda_type in ("", "original", "pcheck_obb_sum", "pcheck_obb_max", "pcheck_obb_loss_weighted_max_count"):
        with pytest.raises(ValueError, match=r'want_depth.*"pcheck_obb".*"fov_pcheck_obb"'):
            render(None, pc, None, torch.zeros(3), cuda_type=cuda_type, want_depth=True)
    # the rasterizer modules themselves
    from fov3dgs_amd import diff_gaussian_rasterization_pcheck_obb_sum as sum_pkg, diff_gaussian_rasterization_fov_pcheck_obb as fov_pkg
    z = torch.zeros(1, 3)
    with pytest.raises(ValueError, match="want_depth"):
        sum_pkg.GaussianRasterizer(None)(means3D=z, means2D=z, opacities=z[:, :1], shs=torch.zeros(1, 16, 3), scales=z, rotations=torch.zeros(1, 4),
                                         want_depth=True)
    for kw in (dict(appearance_only=True), dict(differentiable=True)):
        with pytest.raises(ValueError, match="want_depth"):
            fov_pkg.GaussianRasterizer(None)(means3D=z, means2D=z, opacities=z, shs_rest=torch.zeros(1, 15, 3), scales=z, rotations=torch.zeros(1, 4),
                                             want_depth=True, **kw)
    # the state-keeping forwards and the other variants, below the modules
    monkeypatch.setattr(rasterizer, "_require_gpu", lambda t: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type("Stream", (), {"cuda_stream": 0})())
    with pytest.raises(RuntimeError, match="depth / coverage"):
        rasterizer._forward_begin(_native.VARIANT_ORIGINAL, _Raster(), z, None, None, z, z, z, None, want_depth=True)
    with pytest.raises(RuntimeError, match="depth / coverage"):
        rasterizer._forward_begin(_native.VARIANT_FOV_PCHECK_OBB, _Raster(), z, None, None, z, z, z, None, want_depth=True, keep_state=_native.FovState())
