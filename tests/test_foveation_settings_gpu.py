"""Foveation settings on the GPU: a composed model of 2 .. 8 layers through render(..., foveation=...) / the C ABI against the
independent derivation (tests/numpy_fov_rasterizer.py) run with the same constants, list for list; the default settings spelled
out against the call without settings, bit for bit; no stale settings on the overlapped inference path; the packed layout.

Frames are 640x368 with the 3 000 Gaussians of helpers.small_cloud in L equally likely layers (the derivation takes 2-3 s a case).
Every parity case asserts, ON THE DERIVATION'S OWN VALUES, that a level flip cannot hide behind the 2e-5 the level maps may
differ by: every level holds tiles, many tiles blend, and no tile_min lies within 1e-4 of an integer or of the blend threshold."""
import numpy as np
import pytest
import torch

from tests import foveation_helpers as fh
from tests.checks import check_image
from tests.helpers import small_camera, small_case, small_cloud, syn
from fov3dgs_amd.rasterizer import FoveationSettings

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():  # only reached by an explicit -m gpu run (tests/conftest.py skips otherwise)
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _assert_condition(want, settings):
    """the case cannot hide a level flip (the level maps are compared within 2e-5): see the module docstring"""
    L = settings.levels
    tm = want["tile_min"].astype(np.float64)
    counts = np.bincount(np.clip(np.trunc(tm), 0, L - 1).astype(int), minlength=L)
    assert counts.min() >= (100 if L == 2 else 30), counts
    assert int(np.asarray(want["tile_blend"]).sum()) >= 150
    nonint = tm != np.round(tm)
    assert np.abs(tm[nonint] - np.round(tm[nonint])).min() >= 1e-4
    frac = tm[nonint] - np.trunc(tm[nonint])
    assert np.abs(frac - np.float64(np.float32(settings.start_blend))).min() >= 1e-4


@pytest.mark.parametrize("case", ("L3", "L5", "L6", "L8", "L4band", "L2"))
def test_settings_match_the_derivation_with_the_same_constants(case, monkeypatch):
    _need_gpu()
    settings, alpha, gaze = fh.CASES[case]
    L = settings.levels
    scene, cam = fh.fov_case(settings, alpha, gaze)
    assert scene["opacities"].shape == (fh.POINTS, L) and scene["shs_dcs"].shape == (fh.POINTS, L, 3)
    assert sorted(np.unique(scene["highest_levels"]).astype(int)) == list(range(L))
    want = fh.derivation(monkeypatch, settings, scene, cam)
    _assert_condition(want, settings)
    got = fh.hip_forward_fov(scene, cam, settings)
    assert got["num_rendered"] == want["num_rendered"] > 10000
    np.testing.assert_array_equal(got["radii"], want["radii"])
    np.testing.assert_array_equal(got["ranges"], want["ranges"])
    np.testing.assert_array_equal(got["point_list"], want["point_list"])
    np.testing.assert_allclose(got["tile_levels"], want["tile_levels"], atol=2e-5)
    np.testing.assert_allclose(got["tile_min"], want["tile_min"], atol=2e-5)
    np.testing.assert_array_equal(got["tile_blend"], np.asarray(want["tile_blend"]).astype(np.uint8))
    # the level rows of the levels inside every visible Gaussian's level range (the others are unwritten in the reference too)
    vis = want["radii"] > 0
    assert vis.sum() > 500
    np.testing.assert_array_equal(got["level_ranges"][vis], want["level_ranges"][vis])
    lo, hi = want["level_ranges"][:, 0], want["level_ranges"][:, 1]
    assert hi[vis].max() == L - 1 and (hi[vis] > lo[vis]).sum() > 50
    for l in range(L):
        m = vis & (lo <= l) & (l <= hi)
        assert m.any(), f"no Gaussian needs level {l}"
        np.testing.assert_array_equal(got["level_colours"][m, l, 3], scene["opacities"][m, l])
        np.testing.assert_allclose(got["level_colours"][m, l, :3], want["fov_colors"][m, l], rtol=0, atol=1e-6)
    check_image(got["color"], want["color"], name=f"foveation {case}")
    if got["visibility"] is not None:
        np.testing.assert_array_equal(got["visibility"].cpu().numpy(), want["radii"] > 0)


def _model_on(dev, P, L, seed=3):
    cloud = small_cloud(P, seed).to(dev)
    highest, shs_dcs, opac = syn.foveation_layers(cloud, seed=seed + 1, fractions=(1.0 / L,) * L)
    return cloud, dict(highest_levels=highest, shs_dcs=shs_dcs, opacities=opac)


def _lists(scene, cam, settings, **kw):
    got = fh.hip_forward_fov(scene, cam, settings, debug=False, **kw)
    return got


@pytest.mark.parametrize("size", ((200, 120), (1280, 720)))
@pytest.mark.parametrize("packed", (False, True))
def test_explicit_defaults_are_the_call_without_settings(size, packed):
    _need_gpu()
    scene, cam = small_case("fov_pcheck_obb", width=size[0], height=size[1])
    a = _lists(scene, cam, None, packed=packed)
    b = _lists(scene, cam, FoveationSettings(), packed=packed)
    assert a["num_rendered"] == b["num_rendered"] > 0
    for k in ("color", "radii", "ranges", "point_list", "tile_levels", "tile_min", "tile_gx", "tile_gy", "tile_blend", "level_ranges"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["level_colours"], b["level_colours"], equal_nan=True)
    # ... and through render(): image and radii torch.equal
    from fov3dgs_amd.gaussian_renderer_fov import render
    dev = "cuda:0"
    cloud, layers = _model_on(dev, 3000, 4)
    camera = small_camera(*size).to(dev)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    with torch.no_grad():
        for pk in (None, "auto"):
            outs = [render(camera, cloud, bg, alpha=0.05, gazeArray=(0.4, 0.55), blending=True, packed=pk, foveation=f, **layers)
                    for f in (None, None, FoveationSettings(), None, FoveationSettings())]
            for o in outs[1:]:
                assert torch.equal(o["render"], outs[0]["render"]) and torch.equal(o["radii"], outs[0]["radii"])
                assert torch.equal(o["visibility_filter"], outs[0]["visibility_filter"])


def test_successive_frames_never_see_stale_settings():
    """Nine render() calls in a row on the overlapped inference path (reused argument structs, three internal streams), alternating
    two settings on one model with no synchronisation in between: every image is the one the same call gives on its own. Then nine
    more in the order A B A A B A A B A, where every internal stream sees ONE setting three times (its argument struct is used
    again) while its neighbours carry the other."""
    _need_gpu()
    from fov3dgs_amd import rasterizer
    from fov3dgs_amd.gaussian_renderer_fov import render
    assert rasterizer.OVERLAP_SUCCESSIVE_FRAMES
    dev = "cuda:0"
    cloud, layers = _model_on(dev, 3000, 4)
    camera = small_camera(640, 368).to(dev)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    other = FoveationSettings(4, 16.0, 1.6, 0.8, 0.35, 0.65)
    seq = [None if i % 2 == 0 else other for i in range(9)] + [other if i % 3 == 1 else None for i in range(9)]
    kw = dict(alpha=0.05, gazeArray=(0.3, 0.6), blending=True, **layers)
    with torch.no_grad():
        with rasterizer.serial_frames():
            want = {f: render(camera, cloud, bg, foveation=f, **kw) for f in (None, other)}
        torch.cuda.synchronize()
        assert not torch.equal(want[None]["render"], want[other]["render"])
        got = [render(camera, cloud, bg, foveation=f, **kw) for f in seq]
        torch.cuda.synchronize()
    for f, o in zip(seq, got):
        assert torch.equal(o["render"], want[f]["render"]), f
        assert torch.equal(o["radii"], want[f]["radii"]), f


def test_packed_layout_with_settings(monkeypatch):
    _need_gpu()
    from fov3dgs_amd import rasterizer
    from fov3dgs_amd.gaussian_renderer_fov import render
    # L = 3 packed is the unpacked call bit for bit (and both match the derivation: the parity test above)
    settings, alpha, gaze = fh.CASES["L3"]
    scene, cam = fh.fov_case(settings, alpha, gaze)
    a = _lists(scene, cam, settings, packed=False)
    b = _lists(scene, cam, settings, packed=True)
    assert a["num_rendered"] == b["num_rendered"] > 10000
    for k in ("color", "radii", "ranges", "point_list", "level_ranges"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["level_colours"], b["level_colours"], equal_nan=True)
    # L = 6: pack_model refuses, packed="auto" renders from the ordinary tensors and matches
    dev = "cuda:0"
    settings, alpha, gaze = fh.CASES["L6"]
    cloud, layers = _model_on(dev, 3000, 6)
    camera = small_camera(640, 368).to(dev)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    packs = []
    real_pack = rasterizer.pack_model
    monkeypatch.setattr("fov3dgs_amd.gaussian_renderer_fov.pack_model", lambda *a_, **k_: packs.append(1) or real_pack(*a_, **k_))
    with torch.no_grad():
        plain = render(camera, cloud, bg, alpha=alpha, gazeArray=gaze, blending=True, foveation=settings, **layers)
        autos = [render(camera, cloud, bg, alpha=alpha, gazeArray=gaze, blending=True, packed="auto", foveation=settings, **layers) for _ in range(3)]
        torch.cuda.synchronize()
        assert not packs
        for o in autos:
            assert torch.equal(o["render"], plain["render"]) and torch.equal(o["radii"], plain["radii"])
        with pytest.raises(RuntimeError, match="at most 4 levels"):
            rasterizer.pack_model(cloud.get_xyz, cloud.get_scaling, cloud.get_rotation, layers["opacities"], shs=cloud.get_rest_features,
                                  shs_dcs=layers["shs_dcs"], highest_levels=layers["highest_levels"])
        # a mismatched model is refused instead of misread, through render() too
        with pytest.raises(RuntimeError, match=r"6 level.*renders 4 levels"):
            render(camera, cloud, bg, alpha=alpha, gazeArray=gaze, blending=True, **layers)


@pytest.mark.parametrize("levels", (3, 6))
def test_empty_model_and_empty_frame_with_settings(levels):
    _need_gpu()
    settings = FoveationSettings(levels=levels, real_image_width=1.6, real_viewing_distance=0.8)
    scene, cam = fh.fov_case(settings, 0.05, (0.4, 0.6), width=200, height=120, P=64)
    # a frame with no instance: every Gaussian behind the camera -- the background, no radius, no list
    behind = dict(scene, means3D=scene["means3D"].copy())
    behind["means3D"][:, 2] = -5.0
    got = fh.hip_forward_fov(behind, cam, settings)
    assert got["num_rendered"] == 0 and not got["radii"].any() and not got["ranges"].any()
    for ch in range(3):
        # (a two-level tile holds bg * w + bg * (1 - w): three roundings of half an ulp each, and one for 1 - w)
        np.testing.assert_allclose(got["color"][ch], np.float32(cam["bg"][ch]), rtol=3e-7, atol=0)
    # P = 0: the zero image (the reference returns its zero-initialised tensor), placeholders of any width
    empty = {k: v[:0] for k, v in scene.items()}
    got = fh.hip_forward_fov(empty, cam, settings)
    assert got["num_rendered"] == 0 and got["radii"].size == 0 and np.all(got["color"] == 0)
