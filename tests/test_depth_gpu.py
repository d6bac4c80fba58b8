"""Depth and coverage outputs of the two inference renderers (include/fovraster.h: fr_forward_aux; want_depth=True) on the GPU,
against tests/depth_ref.py (float64, on the oracle's / the derivation's lists and frozen decisions).

Both outputs are judged as the image is (checks.check_image at its defaults): depth / zmax and coverage are each a colour channel with
c <= 1 over the very pairs the image blends, so the image's own bound carries over -- a frame whose image passes cannot fail here
through a flipped decision alone."""
import numpy as np
import pytest
import torch

from fov3dgs_amd import _native, rasterizer
from fov3dgs_amd import synthetic as syn
from fov3dgs_amd.rasterizer import FoveationSettings, _forward_begin, _forward_native, pack_model, serial_frames
from oracle import oracle as orc
from tests import depth_ref as D
from tests import fov_backward_ref as R
from tests import fov_backward_scenes as fs
from tests import foveation_helpers as fh
from tests.checks import check_image
from tests.gpu_helpers import _t, _view, settings_from, vis_list_of
from tests.helpers import small_camera, small_case, small_cloud

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VID = _native.VARIANT_FOV_PCHECK_OBB
PIN = 1e-5   # the depth-as-colour cross-check (tests/test_depth_cpu.py: the bound of the same check against the oracle)


def _need_gpu():
    if not torch.cuda.is_available():  # only reached by an explicit -m gpu run (tests/conftest.py skips otherwise)
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _tensors(scene):
    return {k: _t(scene.get(k), DEV) for k in ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "shs_dcs", "highest_levels")}


def run_fov(scene, cam, settings=None, want_depth=True, packed=False):
    """The foveated inference frame by direct call, on the caller's stream -> dict: image, radii, depth, coverage (device tensors; the
    two planes None without want_depth) and the tile lists as Gaussian indices."""
    lib = _native.load()
    rs = settings_from(cam, DEV, debug=False)
    t = _tensors(scene)
    pk = pack_model(t["means3D"], t["scales"], t["rotations"], t["opacities"], shs=t["shs"], shs_dcs=t["shs_dcs"],
                    highest_levels=t["highest_levels"]) if packed else None
    with torch.no_grad(), serial_frames():
        res = _forward_native(VID, rs, t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, t["shs_dcs"],
                              t["highest_levels"], cam["gaze"], cam["alpha"], persistent=True, packed=pk, foveation=settings,
                              **({"want_depth": True} if want_depth else {}))
    torch.cuda.synchronize()
    n, color, radii, geom, binb, img = res[:6]
    depth, coverage = rasterizer.depth_of(radii)
    out = dict(color=color, radii=radii, depth=depth, coverage=coverage, num_rendered=n)
    W, H, P = rs.image_width, rs.image_height, t["means3D"].shape[0]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    if P == 0 or img.numel() == 0:   # (the library returns before it touches a workspace)
        out["ranges"], out["point_list"] = np.zeros((T, 2), np.uint32), np.zeros(0, np.uint32)
        return out
    out["ranges"] = _view(img, lib.fr_image_ranges(VID, W, H, img.data_ptr()), 2 * T, torch.int32).cpu().numpy().astype(np.uint32).reshape(T, 2)
    if n > 0:
        vis = vis_list_of(lib, VID, P, geom)
        out["point_list"] = vis[_view(binb, lib.fr_binning_point_list(VID, n, binb.data_ptr()), n, torch.int32).long()].cpu().numpy().astype(np.uint32)
    else:
        out["point_list"] = np.zeros(0, np.uint32)
    return out


def judge(out, ref, fwd, tag):
    """depth / zmax and coverage of `out` against depth_ref in float64, each as an image channel; shapes, finiteness, and exact zeros
    where nothing lands. -> (depth64, coverage64, zmax)"""
    assert np.array_equal(out["ranges"], fwd["ranges"]) and np.array_equal(out["point_list"], fwd["point_list"])   # the reference's tile lists
    H, W = ref.H, ref.W
    assert out["depth"].shape == (1, H, W) and out["coverage"].shape == (1, H, W)
    assert out["depth"].dtype == torch.float32 and out["coverage"].dtype == torch.float32
    assert not out["depth"].requires_grad and not out["coverage"].requires_grad
    d64, c64 = D.outputs(ref, fwd["depths"])
    zmax = D.zmax_of(fwd)
    d, c = out["depth"][0].cpu().numpy(), out["coverage"][0].cpu().numpy()
    print(tag, "depth/zmax max diff", np.abs(d / zmax - d64 / zmax).max(), "coverage max diff", np.abs(c - c64).max(), "two-level tiles",
          D.two_level_tiles(ref), "empty", float((c64 == 0).mean()))
    check_image(d / zmax, d64 / zmax, name=f"{tag} depth / zmax")
    check_image(c, c64, name=f"{tag} coverage")
    assert np.all(c >= 0) and np.all(c <= 1) and np.all(d >= 0)
    return d64, c64, zmax


# ---- 4. parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", R.PARITY, ids=lambda k: f"a{k['alpha']}-g{k['gaze'][0]}-{k['gaze'][1]}-w{k.get('width', 200)}")
def test_depth_and_coverage_match_the_reference(kw):
    _need_gpu()
    scene, cam, ofwd, ref, _ = R.case(**kw)
    out = run_fov(scene, cam)
    check_image(out["color"].cpu().numpy(), ofwd["color"], name="image")
    judge(out, ref, ofwd, "parity")
    assert D.two_level_tiles(ref) >= 8
    # the frame itself is the frame without the outputs
    plain = run_fov(scene, cam, want_depth=False)
    assert plain["depth"] is None and plain["coverage"] is None
    assert torch.equal(out["color"], plain["color"]) and torch.equal(out["radii"], plain["radii"])


# ---- 5. levels and layouts ---------------------------------------------------------------------------------------------------------
SETTINGS = {"L3": (FoveationSettings(3, 12.0, 2.0, 1.0, 0.35, 0.65), 0.6, (0.3, 0.4)),
            "L6": (FoveationSettings(6, 16.0, 1.6, 0.8, 0.5, 0.5), 0.6, (0.3, 0.4))}   # (L6: levels >= 4 read the second row of level colours)


@pytest.mark.parametrize("name", tuple(SETTINGS))
def test_other_level_counts(name, monkeypatch):
    _need_gpu()
    settings, alpha, gaze = SETTINGS[name]
    scene, cam = fh.fov_case(settings, alpha, gaze, width=200, height=120, bg=R.BG)
    deriv = fh.derivation(monkeypatch, settings, scene, cam)
    ref = fs.make_ref(deriv, scene, cam, settings)
    levels_used = sorted({st["lev"] for tl in ref.tiles for st in tl["states"] if st["acc"].any()})
    print(name, "levels with accumulated pairs", levels_used)
    assert D.two_level_tiles(ref) >= 5 and levels_used[-1] == settings.levels - 1
    out = run_fov(scene, cam, settings)
    check_image(out["color"].cpu().numpy(), np.asarray(deriv["color"]), name="image")
    judge(out, ref, deriv, name)
    plain = run_fov(scene, cam, settings, want_depth=False)
    assert torch.equal(out["color"], plain["color"]) and torch.equal(out["radii"], plain["radii"])


def test_the_packed_model_gives_the_same_bits():
    _need_gpu()
    scene, cam, ofwd, ref, _ = R.case(**R.MAIN)
    a, b = run_fov(scene, cam), run_fov(scene, cam, packed=True)
    for k in ("color", "radii", "depth", "coverage"):
        assert torch.equal(a[k], b[k]), k


def test_helper_streams_and_the_diagnostic_outputs_beside_the_planes():
    """A leased workspace set (the library's helper streams on: no_helper_streams = 0) with list_consumed and blend_pairs: the planes
    and the image are those of the inference call's settings (no_helper_streams = 1), and the two diagnostics those of the call
    without the planes."""
    _need_gpu()
    scene, cam, ofwd, ref, _ = R.case(**R.MAIN)
    want = run_fov(scene, cam)
    rs, t = settings_from(cam, DEV, debug=False), _tensors(scene)
    T = ((rs.image_width + 15) // 16) * ((rs.image_height + 15) // 16)
    got = {}
    for depth in (True, False):
        cons, pairs = torch.full((T,), -1, dtype=torch.int32, device=DEV), torch.full((T,), -1, dtype=torch.int32, device=DEV)
        with torch.no_grad():
            frame = _forward_begin(VID, rs, t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, t["shs_dcs"],
                                   t["highest_levels"], cam["gaze"], cam["alpha"], persistent=False, list_consumed=cons, blend_pairs=pairs,
                                   **({"want_depth": True} if depth else {}))
            assert int(frame.a.no_helper_streams) == 0
            res = frame.finish()
        torch.cuda.synchronize()
        got[depth] = (res[1], res[2], cons, pairs) + rasterizer.depth_of(res[2])
    assert torch.equal(got[True][0], want["color"]) and torch.equal(got[True][1], want["radii"])
    assert torch.equal(got[True][4], want["depth"]) and torch.equal(got[True][5], want["coverage"])
    assert torch.equal(got[True][2], got[False][2]) and torch.equal(got[True][3], got[False][3])
    assert int(got[True][2].min()) >= 0 and int(got[True][2].sum()) > 0 and int(got[True][3].sum()) > 0


@pytest.mark.parametrize("name", ("tiny-17x15", "tiny-8x8", "tiny-15x1"))
def test_edge_frames(name):
    """17 x 15 (two tiles: one whose tile_min is <= -1 -- level 0 -- and a two-level one), 8 x 8 (a frame smaller than its only tile,
    which is two-level) and 15 x 1 (a frame one pixel high): edge tiles and `inside` masks, on planes NaN before the call."""
    _need_gpu()
    scene, cam, settings = fs.build(name)
    fwd = fs.forward(scene, cam, settings)
    ref = fs.make_ref(fwd, scene, cam, settings)
    if name == "tiny-17x15":
        assert np.asarray(fwd["tile_min"]).min() <= -1 and D.two_level_tiles(ref) >= 1
    if name == "tiny-8x8":
        assert D.two_level_tiles(ref) == 1
    rasterizer.POISON_DEPTH_OUTPUTS = True
    try:
        out = run_fov(scene, cam)
    finally:
        rasterizer.POISON_DEPTH_OUTPUTS = False
    check_image(out["color"].cpu().numpy(), fwd["color"], name="image")
    d64, c64, _ = judge(out, ref, fwd, name)
    assert (c64 > 0).any()


# ---- 6. pcheck_obb -----------------------------------------------------------------------------------------------------------------
def run_plain(scene, cam, want_depth=True):
    rs = settings_from(cam, DEV, debug=False)
    t = _tensors(scene)
    with torch.no_grad():
        res = _forward_begin(_native.VARIANT_PCHECK_OBB, rs, t["means3D"], t["shs"], t["colors_precomp"], t["opacities"], t["scales"], t["rotations"],
                             None, persistent=True, **({"want_depth": True} if want_depth else {})).finish()
    torch.cuda.synchronize()
    lib, vid = _native.load(), _native.VARIANT_PCHECK_OBB
    n, color, radii, geom, binb, img = res[:6]
    depth, coverage = rasterizer.depth_of(radii)
    W, H, P = rs.image_width, rs.image_height, t["means3D"].shape[0]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    vis = vis_list_of(lib, vid, P, geom)
    return dict(color=color, radii=radii, depth=depth, coverage=coverage,
                ranges=_view(img, lib.fr_image_ranges(vid, W, H, img.data_ptr()), 2 * T, torch.int32).cpu().numpy().astype(np.uint32).reshape(T, 2),
                point_list=vis[_view(binb, lib.fr_binning_point_list(vid, n, binb.data_ptr()), n, torch.int32).long()].cpu().numpy().astype(np.uint32))


@pytest.mark.parametrize("size", ((200, 120), (203, 131)))
def test_pcheck_obb_matches_the_reference_and_its_own_colour_path(size):
    _need_gpu()
    scene, cam = small_case("pcheck_obb", width=size[0], height=size[1])
    ofwd = orc.forward("pcheck_obb", scene, cam)
    ref = D.plain_ref(ofwd, scene, cam)
    out = run_plain(scene, cam)
    check_image(out["color"].cpu().numpy(), ofwd["color"], name="image")
    d64, c64, zmax = judge(out, ref, ofwd, f"pcheck_obb {size}")
    plain = run_plain(scene, cam, want_depth=False)
    assert plain["depth"] is None and torch.equal(out["color"], plain["color"]) and torch.equal(out["radii"], plain["radii"])
    # depth as colour through the existing colour path: colors_precomp = (z / zmax, 1, 0), black background
    s2, c2 = dict(scene), dict(cam)
    s2["shs"], s2["colors_precomp"] = None, D.depth_as_colour(ofwd["depths"], zmax)
    c2["bg"] = np.zeros(3, np.float32)
    img = run_plain(s2, c2, want_depth=False)["color"].cpu().numpy()
    d, c = out["depth"][0].cpu().numpy(), out["coverage"][0].cpu().numpy()
    err_d, err_c = np.abs(img[0] - d / zmax).max(), np.abs(img[1] - c).max()
    print("pcheck_obb", size, "against its colour path: depth/zmax", err_d, "coverage", err_c)
    assert err_d <= PIN and err_c <= PIN and np.all(img[2] == 0)


# ---- 7. written in full, the same bits every run -----------------------------------------------------------------------------------
def test_planes_are_written_in_full_with_the_same_bits_every_run(monkeypatch):
    _need_gpu()
    kw = R.PARITY[3]
    assert kw["gaze"] == (0.9, 0.1) and kw["alpha"] == 0.6   # (the frame with empty pixels)
    scene, cam, ofwd, ref, _ = R.case(**kw)
    monkeypatch.setattr(rasterizer, "POISON_DEPTH_OUTPUTS", True)
    a = run_fov(scene, cam)
    b = run_fov(scene, cam)
    d64, c64, _ = judge(a, ref, ofwd, "poisoned")
    for out in (a, b):
        assert torch.isfinite(out["depth"]).all() and torch.isfinite(out["coverage"]).all()
    empty = c64 == 0
    assert empty.mean() >= 0.01
    assert np.all(a["depth"][0].cpu().numpy()[empty] == 0) and np.all(a["coverage"][0].cpu().numpy()[empty] == 0)
    assert torch.equal(a["depth"], b["depth"]) and torch.equal(a["coverage"], b["coverage"]) and torch.equal(a["color"], b["color"])
    # pcheck_obb likewise
    scene, cam = small_case("pcheck_obb")
    p, q = run_plain(scene, cam), run_plain(scene, cam)
    assert torch.isfinite(p["depth"]).all() and torch.isfinite(p["coverage"]).all()
    assert torch.equal(p["depth"], q["depth"]) and torch.equal(p["coverage"], q["coverage"])
    # a frame without Gaussians: both planes are zeros
    s0 = {k: (None if v is None else np.asarray(v)[:0]) for k, v in R.case(**kw)[0].items()}
    e = run_fov(s0, cam=R.case(**kw)[1])
    assert e["num_rendered"] == 0 and not e["depth"].any() and not e["coverage"].any()


# ---- 8. successive frames overlap --------------------------------------------------------------------------------------------------
class _Static:
    """a model whose getters hand over the same tensor objects on every call (what lets successive inference frames overlap)"""

    def __init__(self, cloud):
        with torch.no_grad():
            self.get_xyz, self.get_scaling, self.get_rotation = cloud.get_xyz.clone(), cloud.get_scaling.clone(), cloud.get_rotation.clone()
            self.get_opacity, self.get_rest_features = cloud.get_opacity.clone(), cloud.get_rest_features.clone()
        self.active_sh_degree = cloud.active_sh_degree


def test_nine_overlapped_frames_equal_their_serial_frames():
    """Nine successive calls at the nine bench gazes with OVERLAP_SUCCESSIVE_FRAMES on, want_depth alternating, no synchronisation
    between the calls and a dependent kernel on the caller's stream after each: every call's image / depth / coverage equals, bit for
    bit, the same call under serial_frames() (a reused argument struct or workspace set from the other kind of frame would show)."""
    _need_gpu()
    from fov3dgs_amd.gaussian_renderer_fov import render
    assert rasterizer.OVERLAP_SUCCESSIVE_FRAMES
    cloud = small_cloud(3000, 3)
    highest, dcs, opac = (x.to(DEV) for x in syn.foveation_layers(cloud, seed=4))
    pc = _Static(cloud.to(DEV))
    cam = small_camera(200, 120).to(DEV)
    bg = torch.tensor(R.BG, device=DEV)
    gazes = [(0.25 * i, 0.25 * j) for i in range(1, 4) for j in range(1, 4)]

    def frame(i, gaze):
        return render(cam, pc, bg, alpha=0.6, gazeArray=gaze, blending=True, highest_levels=highest, shs_dcs=dcs, opacities=opac,
                      **({"want_depth": True} if i % 2 == 0 else {}))
    keys = ("render", "depth", "coverage")
    with torch.no_grad():
        for i in range(3):   # (warm-up: every internal stream has had a frame of either kind)
            frame(i, gazes[i])
        torch.cuda.synchronize()
        outs, sums = [], []
        for rounds in range(2):   # (the second round meets the argument structs of the first: every slot has seen both kinds)
            for i, gaze in enumerate(gazes):
                o = frame(i + rounds, gaze)
                outs.append((i + rounds, gaze, o))
                sums.append(sum(o[k].sum() for k in keys if k in o))   # a dependent kernel on the caller's stream
        torch.cuda.synchronize()
        for i, gaze, o in outs:
            assert ("depth" in o) == (i % 2 == 0) and ("coverage" in o) == (i % 2 == 0)
            with serial_frames():
                s = frame(i, gaze)
            torch.cuda.synchronize()
            for k in keys:
                if k in o:
                    assert o[k].shape == s[k].shape and torch.equal(o[k], s[k]), (i, gaze, k)
            assert torch.equal(o["radii"], s["radii"])
        assert all(torch.isfinite(x) for x in sums)
        assert any(o["depth"].max() > 0 for _, _, o in outs if "depth" in o)
