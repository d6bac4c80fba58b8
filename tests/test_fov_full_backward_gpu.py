"""The foveated renderer's FULL backward pass on the GPU (k_render_bwd_fov_full / k_fov_full_bwd over the state of
fr_forward_begin_fov_keep_full): by direct call against tests/fov_full_backward_ref.py (autograd in float64 through a frozen-decision
restatement of the foveated forward; tests/test_fov_full_backward_cpu.py asserts the conditions relied on here), and through autograd
(gaussian_renderer_fov.render(..., differentiable=True)).

Per scene, as tests/test_fov_backward_scenes_gpu.py does for the appearance pass: lists and image are the forward's; the reference is
rebuilt on the LIBRARY's level map; the loss gradient is zero on the pixels whose kept state differs from the reference's (at most
MAX_FLIPPED of the frame); then all eight gradient tensors -- NaN before the call (tests/conftest.py) -- are held to the reference
arithmetic's own float32 noise with the clauses and constants of backward_scenes.judge / fov_backward_scenes.judge (rtol 1e-4, FACTOR
1.5, FLOOR, ABS_ROWS, TAIL_FLOOR), per tensor, and per branch on that branch's own rows. Measured shares go to the parity report."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from fov3dgs_amd import _native, rasterizer
from fov3dgs_amd import synthetic as syn
from fov3dgs_amd.rasterizer import _backward_fov_full_native, _forward_begin, _forward_native
from tests import fov_backward_ref as R
from tests import fov_backward_scenes as fs
from tests import fov_full_backward_ref as F
from tests import test_fov_backward_gpu as fb
from tests.backward_scenes import MIN_LIVE
from tests.checks import check_grad, check_image
from tests.gpu_helpers import _t, _view, settings_from, vis_list_of
from tests.helpers import small_camera, small_cloud

pytestmark = pytest.mark.gpu
DEV = fb.DEV
VID = fb.VID
MAX_FLIPPED = 1e-3   # as tests/test_fov_backward_scenes_gpu.py
FACTORS = F.FACTORS  # per-tensor exceptions to the factor 1.5, with their measurements (tests/fov_full_backward_ref.py)
NAMES = F.LEVELLED + F.GEOMETRY


def full_forward(scene, cam, settings=None, allow_empty=False):
    """The _full state-keeping forward by direct call -> dict, as test_fov_backward_gpu.keep_forward's."""
    lib = _native.load()
    rs = settings_from(cam, DEV, debug=True)
    t = fb._tensors(scene)
    state = _native.FovState()
    state.size = C.sizeof(_native.FovState)
    res = _forward_begin(VID, rs, t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, t["shs_dcs"],
                         t["highest_levels"], cam.get("gaze", (0.5, 0.5)), cam.get("alpha", 0.05), persistent=False, foveation=settings,
                         keep_state=state, keep_full=True).finish()
    torch.cuda.synchronize()
    num_rendered, color, radii, geom, binb, img = res[:6]
    W, H, P = rs.image_width, rs.image_height, t["means3D"].shape[0]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    assert (state.variant, state.P, state.W, state.H, state.num_rendered) == (VID | _native.FOV_STATE_FULL, P, W, H, num_rendered)
    assert state.levels == (4 if settings is None else settings.levels)
    assert 0 < state.num_items <= 4 * T or (allow_empty and num_rendered == 0 and 0 <= state.num_items <= 4 * T)
    assert state.geometry == geom.data_ptr() and state.image == img.data_ptr() and state.binning == binb.data_ptr()
    assert geom.numel() >= lib.fr_geometry_bytes_fov_keep_full(P, state.levels) and img.numel() >= lib.fr_image_bytes_fov_keep(W, H)
    out = dict(color=color, radii=radii, state=state, rs=rs, tensors=t, lease=res[-1], buffers=(geom, binb, img), num_rendered=num_rendered)
    out["ranges"] = _view(img, lib.fr_image_ranges(VID, W, H, img.data_ptr()), 2 * T, torch.int32).cpu().numpy().astype(np.uint32).reshape(T, 2)
    vis = vis_list_of(lib, VID, P, geom)
    if num_rendered > 0:
        items = _view(binb, lib.fr_binning_point_list(VID, num_rendered, binb.data_ptr()), num_rendered, torch.int32).long()
        out["point_list"] = vis[items].cpu().numpy().astype(np.uint32)
    else:
        out["point_list"] = np.zeros(0, np.uint32)
    out["final_T"] = _view(img, lib.fr_image_fov_state_T(W, H, img.data_ptr()), 2 * W * H, torch.float32).cpu().numpy().reshape(2, H, W)
    out["n_contrib"] = _view(img, lib.fr_image_fov_state_n(W, H, img.data_ptr()), 2 * W * H, torch.int32).cpu().numpy().reshape(2, H, W)
    tl = _view(img, lib.fr_image_tile_levels(W, H, img.data_ptr()), 5 * T, torch.float32).cpu().numpy().reshape(5, T)
    out["tile_min"], out["tile_gx"], out["tile_gy"], out["tile_blend"] = tl[1], tl[2], tl[3], (tl[4] != 0).astype(np.uint8)
    return out


def backward(fwd, dL, **kw):
    t = fwd["tensors"]
    g = _backward_fov_full_native(fwd["state"], fwd["rs"], t["means3D"], t["scales"], t["rotations"], t["shs"], _t(dL, DEV),
                                  want_colours=True, want_conic=True, debug=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in g.items() if v is not None}


def _both_passes(name, sh_degree=3):
    """Library and reference on ONE forward state (test_fov_backward_scenes_gpu._both_passes, for the full pass)
    -> (got, g32, g64, census, level census, reference dict, forward dict)"""
    r = F.reference(name, sh_degree)
    fwd = full_forward(r["scene"], r["cam"], r["settings"])
    assert fwd["num_rendered"] == r["fwd"]["num_rendered"]
    np.testing.assert_array_equal(fwd["ranges"], r["fwd"]["ranges"])
    np.testing.assert_array_equal(fwd["point_list"], r["fwd"]["point_list"])
    check_image(fwd["color"].cpu().numpy(), r["fwd"]["color"], name=f"{name} image")
    lib_map = {k: fwd[k] for k in ("tile_min", "tile_gx", "tile_gy")}
    np.testing.assert_array_equal(fwd["tile_blend"], np.asarray(r["fwd"]["tile_blend"]).astype(np.uint8))
    for k in lib_map:
        np.testing.assert_allclose(lib_map[k], r["fwd"][k], rtol=0, atol=2e-5, equal_nan=True)
    ref = fs.make_ref(dict(r["fwd"], **lib_map), r["scene"], r["cam"], r["settings"])
    fT, nc, single = ref.state_planes()
    agree = np.ones_like(single)
    for plane, mask in ((0, np.ones_like(single)), (1, ~single)):
        same = (fwd["n_contrib"][plane] == nc[plane]) & ~(np.abs(fwd["final_T"][plane] - fT[plane]) > 1e-5 * np.abs(fT[plane]) + 1e-9)
        agree &= same | ~mask
    left_out = fs.record_flipped_pixels(f"{name} (full)", agree)
    print(f"{name}: {int((~agree).sum())} of {agree.size} pixels left out of the loss")
    assert left_out <= MAX_FLIPPED
    dpix = r["dpix"] * agree[None].astype(np.float32)
    full = F.FovFullBackwardRef(ref, r["scene"], r["cam"])
    g32, g64 = full.backward(dpix, np.float32), full.backward(dpix, np.float64)
    cen, lcen = F.census(ref, r["scene"], r["cam"], g64), fs.census(ref, r["fwd"], r["scene"], g64)
    got = backward(fwd, dpix)
    for k in NAMES:
        assert got[k].shape == np.shape(g64[k]), (k, got[k].shape)
    return got, g32, g64, cen, lcen, dict(r, ref=ref), fwd


# ---- 1. gradients against the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(F.LARGE))
def test_every_tensor_and_branch_against_the_reference(name):
    """faint (two-level tiles, start-finished pixels), deep (n_contrib beyond 4000: T recovered by division thousands of times),
    faint-L2 (two levels, another blend band) and close-wide-x2.5-fov (clamped tangents of both kinds, scale_modifier): all eight
    tensors, whole, and the five per-Gaussian ones on the live rows of every branch the scene claims. Factor 1.5 throughout
    (fov_full_backward_ref.FACTORS holds no exception)."""
    fb._need_gpu()
    got, g32, g64, cen, lcen, r, _ = _both_passes(name)
    F.record_census(f"{name} (full)", cen)
    for br in F.LARGE[name]:
        assert int(cen[br].sum()) >= F.MIN_BRANCH, br
    F.judge(got, g32, g64, cen, lcen, name, r["L"], branches=F.LARGE[name], factors=FACTORS.get(name))


@pytest.mark.parametrize("name", F.TINY)
def test_tiny_frames(name):
    """17 x 15 (a ragged pair of tiles, one two-level), 8 x 8 (a frame smaller than its only, two-level, tile), 15 x 1 (a frame one
    pixel high): judged with min_rows from the frame's own census."""
    fb._need_gpu()
    got, g32, g64, cen, lcen, r, _ = _both_passes(name)
    F.record_census(f"{name} (full)", cen)
    F.judge(got, g32, g64, cen, lcen, name, 4, min_rows=min(int(cen["live"].sum()), int(lcen["live"].sum())), factors=FACTORS.get(name))


@pytest.mark.parametrize("name", F.SHORT_NAMES)
def test_short_lists_take_every_tail_of_the_nine_sum_fold(name):
    """Lists of 1, 2, 3 and 5 entries: fold18 ends with one entry pending (fold_one, its moments routed to the second row) or none.
    EVERY row of every tensor within SHORT_RTOL of the float64 reference."""
    fb._need_gpu()
    got, g32, g64, cen, lcen, r, _ = _both_passes(name)
    F.judge_short(got, g32, g64, lcen, name, 4, min_rows=int(lcen["live"].sum()))


@pytest.mark.parametrize("name", F.NOTHING)
def test_a_frame_that_renders_nothing_gives_exact_zeros(name):
    fb._need_gpu()
    r = F.reference(name)
    fwd = full_forward(r["scene"], r["cam"], allow_empty=True)
    assert fwd["num_rendered"] == 0 == r["fwd"]["num_rendered"] and not (fwd["radii"] > 0).any()
    got = backward(fwd, r["dpix"])
    for k in NAMES + ("dL_dconic",):
        assert np.isfinite(got[k]).all() and not got[k].any(), k


@pytest.mark.parametrize("deg", F.DEGREES)
def test_lower_sh_degrees_leave_the_higher_coefficients_at_exact_zero(deg):
    fb._need_gpu()
    got, g32, g64, cen, lcen, r, _ = _both_passes("faint", deg)
    n = (deg + 1) ** 2 - 1
    assert not got["dL_dshs_rest"][:, n:].any() and (deg == 0 or got["dL_dshs_rest"][:, :n].any())
    assert not np.asarray(g64["dL_dshs_rest"])[:, n:].any()
    # (degree 0: the reference's dL_dshs_rest is all zeros, asserted exactly above -- no row of it to judge by ratios)
    geometry = F.GEOMETRY if deg else tuple(k for k in F.GEOMETRY if k != "dL_dshs_rest")
    F.judge(got, g32, g64, cen, lcen, f"faint degree {deg}", 4, branches=F.LARGE["faint"], factors=FACTORS.get("faint"), geometry=geometry)


# ---- 2. the forward and the appearance path are what they were ------------------------------------------------------------------------
def test_the_full_forward_is_the_inference_frame_and_the_appearance_path_is_unchanged():
    """Image and radii of the _full forward are torch.equal to the inference frame's and to the plain keep forward's. The appearance
    pass over a plain keep state, run twice with a loss gradient confined to ONE band of ONE single-level tile (every row of sums
    then receives a single atomic add per component: no summation order to vary), is bit-identical; on the whole frame its repeat is
    reported and held to check_grad, like the full call's dL_dopacities / dL_dshs_dcs against the appearance call's (float atomics
    move the last bits)."""
    fb._need_gpu()
    r = F.reference("faint")
    full = full_forward(r["scene"], r["cam"])
    keep = fb.keep_forward(r["scene"], r["cam"])
    t = full["tensors"]
    with torch.no_grad():
        inf = _forward_native(VID, settings_from(r["cam"], DEV, debug=False), t["means3D"], t["shs"], None, t["opacities"], t["scales"],
                              t["rotations"], None, t["shs_dcs"], t["highest_levels"], r["cam"]["gaze"], r["cam"]["alpha"], persistent=True)
    torch.cuda.synchronize()
    assert torch.equal(full["color"], inf[1]) and torch.equal(full["radii"], inf[2])
    assert torch.equal(full["color"], keep["color"]) and torch.equal(full["radii"], keep["radii"])
    for k in ("ranges", "point_list", "tile_blend"):
        np.testing.assert_array_equal(full[k], keep[k])
    # the kept planes: plane 0 everywhere; plane 1 is WRITTEN in two-level tiles only (fovraster.h), elsewhere it is whatever the
    # workspace held, which the two calls' workspaces need not share
    H, W = full["final_T"].shape[1:]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    two = np.kron(keep["tile_blend"].reshape(gy, gx).astype(bool), np.ones((16, 16), bool))[:H, :W]
    assert two.any() and not two.all()
    for k in ("final_T", "n_contrib"):
        np.testing.assert_array_equal(full[k][0], keep[k][0])
        np.testing.assert_array_equal(full[k][1][two], keep[k][1][two])
    # one band (eight pixel rows) of one single-level tile with a long list
    ranges = keep["ranges"].astype(np.int64)
    single = [tix for tix in np.argsort(ranges[:, 0] - ranges[:, 1]) if not keep["tile_blend"][tix]]
    tix, gx = int(single[0]), (200 + 15) // 16
    band = np.zeros_like(r["dpix"])
    y0, x0 = (tix // gx) * 16, (tix % gx) * 16
    band[:, y0:y0 + 8, x0:x0 + 16] = r["dpix"][:, y0:y0 + 8, x0:x0 + 16]
    a1, a2 = fb.backward(keep, band), fb.backward(keep, band)
    assert (a1["dL_dopacities"] != 0).sum() >= 20
    for k in a1:
        assert np.array_equal(a1[k], a2[k]), f"appearance pass, one band, repeat: {k} differs"
    b1, b2 = fb.backward(keep, r["dpix"]), fb.backward(keep, r["dpix"])
    got = backward(full, r["dpix"])
    for k in ("dL_dopacities", "dL_dshs_dcs", "dL_dlevel_colours"):
        print(f"appearance repeat, whole frame: {k}: {int((b1[k] != b2[k]).sum())} of {b1[k].size} entries differ in their last bits")
        check_grad(R.rows(b2[k], 4), R.rows(b1[k], 4), f"appearance repeat {k}", min_rows=MIN_LIVE)
        check_grad(R.rows(got[k], 4), R.rows(b1[k], 4), f"full vs appearance {k}", min_rows=MIN_LIVE)


def test_a_second_backward_over_the_same_state_repeats_the_first():
    fb._need_gpu()
    r = F.reference("faint")
    fwd = full_forward(r["scene"], r["cam"])
    first = backward(fwd, r["dpix"])
    t = fwd["tensors"]
    with torch.no_grad():  # an inference render in between does not disturb the kept state
        _forward_native(VID, fwd["rs"], t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, t["shs_dcs"],
                        t["highest_levels"], (0.7, 0.7), 0.05, persistent=True)
    torch.cuda.synchronize()
    second = backward(fwd, r["dpix"])
    for k in NAMES:
        rows = lambda x: R.rows(x, 4) if k in F.LEVELLED else x.reshape(len(x), -1)
        check_grad(rows(second[k]), rows(first[k]), f"repeat {k}", min_rows=MIN_LIVE)


# ---- 3. autograd ---------------------------------------------------------------------------------------------------------------------
class _Leaves:
    """A model whose getters ARE its leaves (activated values), so that autograd's gradients are the direct call's"""

    def __init__(self, scene, sh_degree=3):
        P = np.asarray(scene["means3D"]).shape[0]
        leaf = lambda k, shape: _t(np.asarray(scene[k], np.float32).reshape(shape), DEV).requires_grad_(True)
        self.get_xyz, self.get_scaling, self.get_rotation = leaf("means3D", (P, 3)), leaf("scales", (P, 3)), leaf("rotations", (P, 4))
        self.get_rest_features = leaf("shs", (P, -1, 3))
        self.opacities, self.shs_dcs = leaf("opacities", (P, -1)), leaf("shs_dcs", (P, -1, 3))
        self.highest_levels = _t(scene["highest_levels"], DEV)
        self.get_opacity = self.opacities[:, :1]
        self.active_sh_degree = sh_degree

    def leaves(self):
        return dict(dL_dmeans3D=self.get_xyz, dL_dscales=self.get_scaling, dL_drotations=self.get_rotation, dL_dshs_rest=self.get_rest_features,
                    dL_dopacities=self.opacities, dL_dshs_dcs=self.shs_dcs)


def _camera(cam):
    c = small_camera(int(cam["image_width"]), int(cam["image_height"])).to(DEV)
    np.testing.assert_allclose(c.full_proj_transform.cpu().numpy().reshape(-1), np.asarray(cam["projmatrix"], np.float32).reshape(-1), rtol=1e-6, atol=1e-7)
    return c


def _render(model, cam_obj, cam, **extra):
    from fov3dgs_amd.gaussian_renderer_fov import render
    return render(cam_obj, model, torch.tensor(R.BG, device=DEV), alpha=cam["alpha"], gazeArray=cam["gaze"], blending=True,
                  highest_levels=model.highest_levels, shs_dcs=model.shs_dcs, opacities=model.opacities, **extra)


def _graph(r, gaze=None, **extra):
    cam = dict(r["cam"], gaze=gaze) if gaze is not None else r["cam"]
    model = _Leaves(r["scene"])
    return _render(model, _camera(cam), cam, differentiable=True, **extra), model


def _finish(graph, dL):
    out, model = graph
    (out["render"] * dL).sum().backward()
    torch.cuda.synchronize()
    g = {k: v.grad.cpu().numpy() for k, v in model.leaves().items()}
    g["dL_dmeans2D"] = out["viewspace_points"].grad.cpu().numpy()
    return g


MIN_ALONE = 300   # rows with a gradient that every tensor of a graph run alone must have (gaze B sees fewer Gaussians than gaze A)


def _same(got, want, tag):
    """check_grad per tensor against the same graph run alone; min_rows: MIN_LIVE, or nine tenths of the rows that carry a gradient in
    the run alone where that is fewer (never fewer than MIN_ALONE)."""
    for k in got:
        assert got[k].shape == want[k].shape and np.isfinite(got[k]).all(), k
        rows = (lambda x: R.rows(x, 4)) if k in F.LEVELLED else (lambda x: x.reshape(len(x), -1))
        have = int((rows(want[k]).reshape(len(rows(want[k])), -1) != 0).any(axis=1).sum())
        assert have >= MIN_ALONE, (tag, k, have)
        check_grad(rows(got[k]), rows(want[k]), f"{tag} {k}", min_rows=min(MIN_LIVE, (9 * have) // 10))


_alone_cache = {}
GAZE_B = (0.2, 0.35)


def _alone(which):
    if which not in _alone_cache:
        r = F.reference("faint")
        _alone_cache[which] = _finish(_graph(r, None if which == "A" else GAZE_B), _t(r["dpix"], DEV))
    return _alone_cache[which]


def test_autograd_gives_the_direct_calls_gradients_and_fills_the_viewspace_points():
    fb._need_gpu()
    r = F.reference("faint")
    direct = backward(full_forward(r["scene"], r["cam"]), r["dpix"])
    got = _alone("A")
    _same(got, direct, "autograd vs direct")
    assert (np.abs(got["dL_dmeans2D"][:, :2]).sum(axis=1) != 0).sum() >= MIN_LIVE and not got["dL_dmeans2D"][:, 2].any()
    # under no_grad no node is built and the image is the inference image; without the flag nothing gets a gradient
    model, cam = _Leaves(r["scene"]), r["cam"]
    out = _render(model, _camera(cam), cam, differentiable=True)
    with torch.no_grad():
        plain = _render(model, _camera(cam), cam, differentiable=True)
    assert plain["render"].grad_fn is None and torch.equal(plain["render"], out["render"].detach())
    out = _render(model, _camera(cam), cam)
    (out["render"] * _t(r["dpix"], DEV)).sum().backward()
    assert all(v.grad is None for v in model.leaves().values())


def test_scaling_modifier_is_honoured_through_autograd():
    fb._need_gpu()
    r = F.reference("close-wide-x2.5-fov")
    direct = backward(full_forward(r["scene"], r["cam"]), r["dpix"])
    from tests import backward_scenes as bs
    cam_obj = bs.camera((0.4, -0.3, 2.5), 50.0, 200, 120).to(DEV)
    model = _Leaves(r["scene"])
    out = _render(model, cam_obj, r["cam"], differentiable=True, scaling_modifier=2.5)
    got = _finish((out, model), _t(r["dpix"], DEV))
    for k in got:
        rows = (lambda x: R.rows(x, 4)) if k in F.LEVELLED else (lambda x: x.reshape(len(x), -1))
        check_grad(rows(got[k]), rows(direct[k]), f"x2.5 autograd vs direct {k}", min_rows=F.MIN_BRANCH)


def test_two_graphs_alive_at_once_keep_their_own_state():
    fb._need_gpu()
    r = F.reference("faint")
    dL = _t(r["dpix"], DEV)
    a, b = _graph(r), _graph(r, GAZE_B)
    ws = lambda g: {t.data_ptr() for t in g[0]["render"].grad_fn.saved_tensors[:3]}
    assert not (ws(a) & ws(b)), "two live graphs share a workspace buffer"
    got_b = _finish(b, dL)
    got_a = _finish(a, dL)
    _same(got_b, _alone("B"), "B beside A")
    _same(got_a, _alone("A"), "A after B")
    assert not np.array_equal(got_a["dL_dmeans3D"], got_b["dL_dmeans3D"])


def test_a_graph_dropped_without_backward_leaves_the_next_one_intact():
    fb._need_gpu()
    r = F.reference("faint")
    dL = _t(r["dpix"], DEV)
    dropped = _graph(r)
    del dropped
    gc.collect()
    _same(_finish(_graph(r, GAZE_B), dL), _alone("B"), "after a dropped graph")


def test_forward_and_backward_on_a_non_default_stream():
    fb._need_gpu()
    want = _alone("A")
    r = F.reference("faint")
    dL = _t(r["dpix"], DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        graph = _graph(r)
        (graph[0]["render"] * dL).sum().backward()
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    got = {k: v.grad.cpu().numpy() for k, v in graph[1].leaves().items()}
    got["dL_dmeans2D"] = graph[0]["viewspace_points"].grad.cpu().numpy()
    _same(got, want, "side stream")


def test_a_non_contiguous_upstream_gradient():
    fb._need_gpu()
    r = F.reference("faint")
    dL = _t(r["dpix"], DEV)
    strided = dL.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    assert not strided.is_contiguous() and torch.equal(strided, dL)
    out, model = _graph(r)
    out["render"].backward(gradient=strided)
    torch.cuda.synchronize()
    got = {k: v.grad.cpu().numpy() for k, v in model.leaves().items()}
    got["dL_dmeans2D"] = out["viewspace_points"].grad.cpu().numpy()
    _same(got, _alone("A"), "strided upstream gradient")


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """five levels, a packed model, appearance_only together with differentiable, highest_levels that requires grad, a NULL required
    pointer (on a real state: nothing is enqueued, the state stays usable)."""
    fb._need_gpu()
    from fov3dgs_amd.rasterizer import FoveationSettings
    r = F.reference("faint")
    model, cam = _Leaves(r["scene"]), r["cam"]
    cam_obj = _camera(cam)
    with pytest.raises(ValueError, match="4 levels"):
        _render(model, cam_obj, cam, differentiable=True, foveation=FoveationSettings(5, 12.0, 2.0, 1.0, 0.5, 0.5))
    with pytest.raises(ValueError, match="appearance_only"):
        _render(model, cam_obj, cam, differentiable=True, appearance_only=True)
    packed = rasterizer.pack_model(model.get_xyz.detach(), model.get_scaling.detach(), model.get_rotation.detach(), model.opacities.detach(),
                                   shs=model.get_rest_features.detach(), shs_dcs=model.shs_dcs.detach(), highest_levels=model.highest_levels)
    with pytest.raises(ValueError, match="packed"):
        _render(model, cam_obj, cam, differentiable=True, packed=packed)
    model.highest_levels = model.highest_levels.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="highest_levels"):
        _render(model, cam_obj, cam, differentiable=True)
    fwd = full_forward(r["scene"], r["cam"])
    t = dict(fwd["tensors"])
    with pytest.raises(RuntimeError, match="scales is null"):
        _backward_fov_full_native(fwd["state"], fwd["rs"], t["means3D"], torch.empty(0, device=DEV), t["rotations"], t["shs"], _t(r["dpix"], DEV))
    got = backward(fwd, r["dpix"])   # the refused call enqueued nothing and cleared nothing
    assert np.isfinite(got["dL_dmeans3D"]).all() and (np.abs(got["dL_dmeans3D"]).sum(axis=1) != 0).sum() >= MIN_LIVE


# ---- 5. the use the pass is for ------------------------------------------------------------------------------------------------------
def test_fine_tuning_positions_and_scales_through_the_foveated_renderer():
    """Thirty Adam steps on the faint scene: means3D and the raw scales start perturbed and are fitted, L1, to the frame of the
    unperturbed model, whose loss is zero -- the loss falls below half its start, the bound of
    test_fine_tuning_the_opacities_through_the_foveated_renderer (Adam's first steps move a coordinate by its learning rate per step,
    2e-3 against a perturbation of 2e-2 in the positions: thirty steps reach every offset; a wrong sign or an unrelated direction
    RAISES the loss of a model this close to the optimum). Every step's loss is printed."""
    fb._need_gpu()
    from fov3dgs_amd.gaussian_renderer_fov import render
    from tests.fov_backward_scenes import OPACITY_FACTOR
    cloud = small_cloud(3000, 3)
    highest, dcs, opac = syn.foveation_layers(cloud, seed=4)
    cloud, cam, bg = cloud.to(DEV), small_camera().to(DEV), torch.tensor(R.BG, device=DEV)
    highest, dcs, opac = highest.to(DEV), dcs.to(DEV), (opac * OPACITY_FACTOR).to(DEV)
    kw = dict(alpha=0.6, gazeArray=(0.4, 0.55), blending=True, highest_levels=highest, shs_dcs=dcs, opacities=opac)
    with torch.no_grad():
        target = render(cam, cloud, bg, **kw)["render"]
        gen = torch.Generator(device="cpu").manual_seed(5)
        cloud._xyz += (0.02 * torch.randn(cloud._xyz.shape, generator=gen)).to(DEV)
        cloud._scaling += (0.2 * torch.randn(cloud._scaling.shape, generator=gen)).to(DEV)
    cloud._xyz.requires_grad_(True)
    cloud._scaling.requires_grad_(True)
    opt = torch.optim.Adam([dict(params=[cloud._xyz], lr=2e-3), dict(params=[cloud._scaling], lr=2e-2)])
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        loss = (render(cam, cloud, bg, differentiable=True, **kw)["render"] - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float((render(cam, cloud, bg, **kw)["render"] - target).abs().mean()))
    print("L1 loss per step", [f"{v:.5f}" for v in losses])
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0]
