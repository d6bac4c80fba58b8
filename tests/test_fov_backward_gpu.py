"""The foveated renderer's appearance backward pass on the GPU: fr_forward_begin_fov_keep / fr_backward_fov_appearance by direct call
against tests/fov_backward_ref.py (validated on its own in tests/test_fov_backward_cpu.py), and through autograd
(GaussianRasterizer.forward(..., appearance_only=True), gaussian_renderer_fov.render(..., appearance_only=True)).

Comparisons are one row per (Gaussian, level) -- [P L, ...] -- with checks.check_grad's defaults, whose budgets absorb the few
threshold flips between v_exp_f32 and the oracle's expf; min_rows comes from the conditions the CPU file asserts on the reference."""
import ctypes as C

import numpy as np
import pytest
import torch

from fov3dgs_amd import _native, rasterizer
from fov3dgs_amd import synthetic as syn
from fov3dgs_amd.rasterizer import FoveationSettings, _backward_fov_native, _forward_begin, _forward_native
from tests import checks
from tests import fov_backward_ref as R
from tests import foveation_helpers as fh
from tests.checks import check_grad, check_image
from tests.gpu_helpers import _t, _view, settings_from, vis_list_of
from tests.helpers import small_camera, small_cloud

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VID = _native.VARIANT_FOV_PCHECK_OBB
MAIN_ROWS = 4 * R.MIN_ROWS_PER_LEVEL
# share of the pixels whose kept n_contrib may differ from the reference's: the budget the gradient rows get for the threshold flips
# (a flipped pair at the END of a pixel's contributors moves its n_contrib; its final_T moves by less than the image tolerance)
N_CONTRIB_FLIPS = checks.GRAD_OUTLIERS


def _need_gpu():
    if not torch.cuda.is_available():  # only reached by an explicit -m gpu run (tests/conftest.py skips otherwise)
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _tensors(scene):
    return {k: _t(scene.get(k), DEV) for k in ("means3D", "shs", "opacities", "scales", "rotations", "shs_dcs", "highest_levels")}


def keep_forward(scene, cam, settings=None, allow_empty=False):
    """The state-keeping forward by direct call -> dict: image and radii (device tensors), the tile lists as Gaussian indices, the
    kept per-state planes, and the state for backward(). The dict holds the workspace lease.
    allow_empty: the frame may render no instance at all (then it has no work items and an empty point list)."""
    lib = _native.load()
    rs = settings_from(cam, DEV, debug=True)
    t = _tensors(scene)
    state = _native.FovState()
    state.size = C.sizeof(_native.FovState)
    res = _forward_begin(VID, rs, t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, t["shs_dcs"],
                         t["highest_levels"], cam.get("gaze", (0.5, 0.5)), cam.get("alpha", 0.05), persistent=False, foveation=settings,
                         keep_state=state).finish()
    torch.cuda.synchronize()
    num_rendered, color, radii, geom, binb, img = res[:6]
    W, H, P = rs.image_width, rs.image_height, t["means3D"].shape[0]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    assert (state.variant, state.P, state.W, state.H, state.num_rendered) == (VID, P, W, H, num_rendered)
    assert state.levels == (4 if settings is None else settings.levels)
    assert 0 < state.num_items <= 4 * T or (allow_empty and num_rendered == 0 and 0 <= state.num_items <= 4 * T)
    assert state.geometry == geom.data_ptr() and state.image == img.data_ptr() and state.binning == binb.data_ptr()
    assert geom.numel() >= lib.fr_geometry_bytes_fov_keep(P, state.levels) and img.numel() >= lib.fr_image_bytes_fov_keep(W, H)
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
    tl = _view(img, lib.fr_image_tile_levels(W, H, img.data_ptr()), 5 * T, torch.float32).cpu().numpy().reshape(5, T)   # the library's level map
    out["tile_min"], out["tile_gx"], out["tile_gy"], out["tile_blend"] = tl[1], tl[2], tl[3], (tl[4] != 0).astype(np.uint8)
    lv = _view(geom, lib.fr_geometry_level_colours(P, geom.data_ptr()), 16 * P, torch.float32).view(P, 4, 4).cpu().numpy()
    rows = np.full((P, 4, 4), np.nan, np.float32)
    rows[vis.cpu().numpy()] = lv[:len(vis)]
    out["level_colours"] = rows
    return out


def backward(fwd, dL, want_colours=True):
    g = _backward_fov_native(fwd["state"], fwd["rs"].bg, _t(dL, DEV), want_colours=want_colours, debug=True)
    torch.cuda.synchronize()
    return dict(zip(("dL_dopacities", "dL_dshs_dcs", "dL_dlevel_colours"), (None if x is None else x.cpu().numpy() for x in g)))


def compare(got, want, L, name, min_rows):
    for k in ("dL_dopacities", "dL_dlevel_colours", "dL_dshs_dcs"):
        assert got[k].shape == want[k].shape and np.isfinite(got[k]).all(), k   # (the harness poisons the outputs with NaN)
        check_grad(R.rows(got[k], L), R.rows(want[k], L), f"{name} {k}", min_rows=min_rows)
    # rows and levels no tile used are EXACT zeros
    unused = want["dL_dopacities"] == 0
    stray = int((got["dL_dopacities"][unused] != 0).sum())
    assert stray <= max(3, checks.GRAD_OUTLIERS * (~unused).sum()), f"{name}: {stray} (Gaussian, level) rows the reference leaves at zero carry a gradient"


# ---- 1. oracle parity by direct call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", R.PARITY, ids=lambda k: f"a{k['alpha']}-g{k['gaze'][0]}-{k['gaze'][1]}-w{k.get('width', 200)}")
def test_gradients_match_the_reference(kw):
    _need_gpu()
    scene, cam, ofwd, ref, dL = R.case(**kw)
    fwd = keep_forward(scene, cam)
    assert np.array_equal(fwd["ranges"], ofwd["ranges"]) and np.array_equal(fwd["point_list"], ofwd["point_list"])  # the oracle's tile lists
    check_image(fwd["color"].cpu().numpy(), ofwd["color"], name="image")
    got, want = backward(fwd, dL), ref.backward(dL)
    assert np.abs(got["dL_dopacities"]).max() > 0 and np.abs(got["dL_dshs_dcs"]).max() > 0
    compare(got, want, 4, "parity", MAIN_ROWS if kw is R.MAIN else R.MIN_ROWS_OTHER)


# ---- 2. the state-keeping forward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", (R.MAIN, R.PARITY[-1]), ids=("main", "ragged"))
def test_state_keeping_forward_is_the_inference_frame_plus_state(kw):
    _need_gpu()
    scene, cam, ofwd, ref, dL = R.case(**kw)
    fwd = keep_forward(scene, cam)
    t = fwd["tensors"]
    with torch.no_grad():
        inf = _forward_native(VID, fwd["rs"], t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, t["shs_dcs"],
                              t["highest_levels"], cam["gaze"], cam["alpha"], persistent=True)
    torch.cuda.synchronize()
    assert torch.equal(fwd["color"], inf[1]) and torch.equal(fwd["radii"], inf[2])
    fT, nc, single = ref.state_planes()
    blend = ~single
    # single-level tiles: plane 0; two-level tiles: both planes (state 1 of a pixel that starts finished keeps T = 1, n = 0)
    for plane, mask in ((0, np.ones_like(single)), (1, blend)):
        check_image(np.where(mask, fwd["final_T"][plane], 0), np.where(mask, fT[plane], 0), name=f"final_T plane {plane}")
        differ = int(((fwd["n_contrib"][plane] != nc[plane]) & mask).sum())
        print("n_contrib plane", plane, "differs on", differ, "of", int(mask.sum()), "pixels")
        assert differ <= max(3, N_CONTRIB_FLIPS * mask.sum())
    start_finished = blend & (nc[0] == 0) & (fT[0] == 1)
    assert start_finished.sum() > 0 and np.all(fwd["final_T"][0][start_finished] == 1.0)
    assert int((fwd["n_contrib"][0][start_finished] != 0).sum()) <= max(3, N_CONTRIB_FLIPS * start_finished.sum())


# ---- 3. settings -----------------------------------------------------------------------------------------------------------------
SETTINGS = {"L2": (FoveationSettings(2, 12.0, 2.0, 1.0, 0.6, 0.4), 0.6, (0.3, 0.4)),
            "L3": (FoveationSettings(3, 12.0, 2.0, 1.0, 0.35, 0.65), 0.6, (0.3, 0.4))}


@pytest.mark.parametrize("name", tuple(SETTINGS))
def test_levels_two_and_three_with_other_blend_bands(name, monkeypatch):
    _need_gpu()
    settings, alpha, gaze = SETTINGS[name]
    L = settings.levels
    scene, cam = fh.fov_case(settings, alpha, gaze, width=200, height=120, bg=R.BG)
    deriv = fh.derivation(monkeypatch, settings, scene, cam)
    ref = R.FovBackwardRef(deriv, scene, cam, levels=L, start_blend=settings.start_blend, blend_width=settings.blend_width)
    dL = R.dL_for(cam, seed=13)
    want = ref.backward(dL)
    blend_tiles = sum(1 for t in ref.tiles if t["blend"])
    rows_with = int((want["dL_dopacities"] != 0).sum())
    print(name, "two-level tiles", blend_tiles, "rows", rows_with, "per level", [(int((want["dL_dopacities"][:, lv] != 0).sum())) for lv in range(L)])
    assert blend_tiles >= 5 and rows_with >= R.MIN_ROWS_OTHER and all((want["dL_dopacities"][:, lv] != 0).any() for lv in range(L))
    fwd = keep_forward(scene, cam, settings)
    assert np.array_equal(fwd["ranges"], deriv["ranges"]) and np.array_equal(fwd["point_list"], deriv["point_list"])
    got = backward(fwd, dL)
    assert got["dL_dopacities"].shape == (ref.P, L) and got["dL_dshs_dcs"].shape == (ref.P, L, 3) and got["dL_dlevel_colours"].shape == (ref.P, L, 3)
    compare(got, want, L, name, R.MIN_ROWS_OTHER)


def test_five_levels_are_refused():
    _need_gpu()
    settings = FoveationSettings(5, 12.0, 2.0, 1.0, 0.5, 0.5)
    scene, cam = fh.fov_case(settings, 0.3, (0.4, 0.5), width=200, height=120)
    with pytest.raises(RuntimeError, match="levels"):
        keep_forward(scene, cam, settings)


# ---- 4. clamp ---------------------------------------------------------------------------------------------------------------------
def test_clamped_channels_pass_no_gradient_to_their_level():
    """DCs shifted by -1.5 as test_clamped_channels_pass_no_gradient does: roughly four channels in ten clamp. A channel the forward
    pass clamped at a level gets a DC gradient of exactly 0 there while its colour gradient is not."""
    _need_gpu()
    scene, cam, ofwd, ref, dL = R.case(**R.MAIN, mutate="clamp")
    fwd = keep_forward(scene, cam)
    got, want = backward(fwd, dL), ref.backward(dL)
    used = (ref.used_single | ref.used_blend)[..., None]
    clamped = (fwd["level_colours"][..., :3] == 0) & used                                     # what the forward pass clamped
    agree = (clamped == ((np.nan_to_num(ref.colours, nan=1.0) == 0) & used)).mean()
    assert clamped.sum() >= 300 and (used & ~clamped).sum() >= 300 and agree > 0.999
    assert np.all(got["dL_dshs_dcs"][clamped] == 0.0)
    assert np.mean(got["dL_dlevel_colours"][clamped] != 0) > 0.99
    compare(got, want, 4, "clamp", MAIN_ROWS)


# ---- 5. existence skip ------------------------------------------------------------------------------------------------------------
def test_gaussians_that_exist_at_level_zero_only_get_no_gradient_above():
    _need_gpu()
    scene, cam, ofwd, ref, dL = R.case(**R.MAIN, mutate="hl0")
    fwd = keep_forward(scene, cam)
    got, want = backward(fwd, dL), ref.backward(dL)
    for k in ("dL_dopacities", "dL_dshs_dcs", "dL_dlevel_colours"):
        assert np.all(got[k][:, 1:] == 0.0), k
    assert (got["dL_dopacities"][:, 0] != 0).sum() >= 20 and (np.abs(got["dL_dshs_dcs"][:, 0]).max(axis=1) > 0).sum() >= 20
    compare(got, want, 4, "hl0", 20)


# ---- 6. saturation convention -----------------------------------------------------------------------------------------------------
def test_saturated_alphas_follow_the_undifferentiated_min():
    _need_gpu()
    scene, cam, ofwd, ref, dL = R.case(**R.MAIN, mutate="sat")
    fwd = keep_forward(scene, cam)
    got, want = backward(fwd, dL), ref.backward(dL)
    sat = (ref.opac == 1.0) & (want["dL_dopacities"] != 0)
    assert sat.sum() >= 20 and (got["dL_dopacities"][sat] != 0).mean() > 0.9
    compare(got, want, 4, "sat", MAIN_ROWS)
    check_grad(got["dL_dopacities"][sat].reshape(-1, 1), want["dL_dopacities"][sat].reshape(-1, 1), "saturated rows", min_rows=20)


# ---- 7. - 9. autograd ------------------------------------------------------------------------------------------------------------
def _model(kw=R.MAIN):
    """the scene of R.case(**kw) as render() takes it: (cloud, camera, bg, highest_levels, shs_dcs, opacities) on the GPU"""
    cloud = small_cloud(3000, 3)
    highest, dcs, opac = syn.foveation_layers(cloud, seed=4)
    cam = small_camera(kw.get("width", 200), kw.get("height", 120)).to(DEV)
    return cloud.to(DEV), cam, torch.tensor(R.BG, device=DEV), highest.to(DEV), dcs.to(DEV), opac.to(DEV)


def _render(cloud, cam, bg, highest, dcs, opac, kw=R.MAIN, **extra):
    from fov3dgs_amd.gaussian_renderer_fov import render
    return render(cam, cloud, bg, alpha=kw["alpha"], gazeArray=kw["gaze"], blending=True, highest_levels=highest, shs_dcs=dcs, opacities=opac, **extra)


def test_autograd_gives_the_direct_calls_gradients():
    _need_gpu()
    scene, cam_d, ofwd, ref, dL = R.case(**R.MAIN)
    direct = backward(keep_forward(scene, cam_d), dL, want_colours=False)
    cloud, cam, bg, highest, dcs, opac = _model()
    opac.requires_grad_(True)
    dcs.requires_grad_(True)
    out = _render(cloud, cam, bg, highest, dcs, opac, appearance_only=True)
    (out["render"] * torch.tensor(dL, device=DEV)).sum().backward()
    torch.cuda.synchronize()
    assert opac.grad.shape == opac.shape and dcs.grad.shape == dcs.shape
    check_grad(R.rows(opac.grad.cpu().numpy(), 4), R.rows(direct["dL_dopacities"], 4), "autograd opacities", min_rows=MAIN_ROWS)
    check_grad(R.rows(dcs.grad.cpu().numpy(), 4), R.rows(direct["dL_dshs_dcs"], 4), "autograd shs_dcs", min_rows=MAIN_ROWS)
    # the image is the inference image, and under no_grad no node is built
    with torch.no_grad():
        plain = _render(cloud, cam, bg, highest, dcs, opac, appearance_only=True)
    assert plain["render"].grad_fn is None and torch.equal(plain["render"], out["render"].detach())
    # without the flag: today's behaviour -- a graph whose backward hands None to everything
    opac.grad = dcs.grad = None
    out = _render(cloud, cam, bg, highest, dcs, opac)
    (out["render"] * torch.tensor(dL, device=DEV)).sum().backward()
    assert opac.grad is None and dcs.grad is None
    # refusals
    from fov3dgs_amd.diff_gaussian_rasterization_fov_pcheck_obb import GaussianRasterizer
    r = GaussianRasterizer(settings_from(cam_d, DEV, debug=False))
    args = dict(means3D=cloud.get_xyz.detach(), means2D=torch.zeros_like(cloud.get_xyz), opacities=opac, shs_rest=cloud.get_rest_features.detach(),
                scales=cloud.get_scaling.detach(), rotations=cloud.get_rotation.detach(), shs_dcs=dcs, highest_levels=highest,
                gazeArray=R.MAIN["gaze"], alpha=R.MAIN["alpha"])
    with pytest.raises(ValueError, match="appearance_only: scales requires grad"):
        r(**dict(args, scales=cloud.get_scaling.detach().requires_grad_(True)), appearance_only=True)
    packed = rasterizer.pack_model(args["means3D"], args["scales"], args["rotations"], opac.detach(), shs=args["shs_rest"], shs_dcs=dcs.detach(),
                                   highest_levels=highest)
    with pytest.raises(ValueError, match="packed"):
        r(**args, packed=packed, appearance_only=True)
    with pytest.raises(ValueError, match="packed"):
        _render(cloud, cam, bg, highest, dcs, opac, appearance_only=True, packed=packed)


def test_a_second_backward_over_the_same_state_gives_the_same_gradients():
    _need_gpu()
    scene, cam, ofwd, ref, dL = R.case(**R.MAIN)
    fwd = keep_forward(scene, cam)
    first = backward(fwd, dL)
    t = fwd["tensors"]
    with torch.no_grad():  # a plain inference render in between does not disturb the kept state
        inf = _forward_native(VID, fwd["rs"], t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, t["shs_dcs"],
                              t["highest_levels"], (0.7, 0.7), 0.05, persistent=True)
    torch.cuda.synchronize()
    second = backward(fwd, dL)
    for k in first:
        check_grad(R.rows(second[k], 4), R.rows(first[k], 4), f"repeat {k}", min_rows=MAIN_ROWS)
    compare(second, ref.backward(dL), 4, "second call", MAIN_ROWS)


def test_outputs_that_are_not_16_byte_aligned_are_written_in_full_and_nothing_beside_them():
    """The fill's fallback for a tensor its 16-byte stores cannot take (hipMemsetAsync): every output is the [1:-1] view of a NaN-filled
    buffer two floats longer, so each pointer is 4 bytes off alignment. The call succeeds, every element of the views is written, the
    guard element on either side of each is untouched, and the gradients are those of the aligned call over the same state."""
    _need_gpu()
    scene, cam, ofwd, ref, dL = R.case(**R.MAIN)
    fwd = keep_forward(scene, cam)
    first = backward(fwd, dL)
    st, rs = fwd["state"], fwd["rs"]
    P, L = int(st.P), int(st.levels)
    bufs = {k: torch.full((n + 2,), float("nan"), dtype=torch.float32, device=DEV)
            for k, n in (("dL_dopacities", P * L), ("dL_dshs_dcs", 3 * P * L), ("dL_dlevel_colours", 3 * P * L))}
    views = {k: b[1:-1] for k, b in bufs.items()}
    a = _native.BackwardFovArgs()
    a.size, a.debug, a.state = C.sizeof(_native.BackwardFovArgs), 1, C.pointer(st)
    bg, dpix = rs.bg.to(DEV).float().contiguous(), _t(dL, DEV).float().contiguous()
    a.background, a.dL_dpix = bg.data_ptr(), dpix.data_ptr()
    for k, v in views.items():
        assert v.data_ptr() % 16 == 4, k
        setattr(a, k, v.data_ptr())
    a.stream = torch.cuda.current_stream(DEV).cuda_stream
    rc = _native.load().fr_backward_fov_appearance(C.byref(a))
    torch.cuda.synchronize()
    assert rc == 0, _native.last_error()
    for k, b in bufs.items():
        assert bool(torch.isfinite(views[k]).all()), k
        assert bool(torch.isnan(b[0])) and bool(torch.isnan(b[-1])), f"{k}: a guard element was written"
    second = {k: v.cpu().numpy().reshape(first[k].shape) for k, v in views.items()}
    for k in first:
        check_grad(R.rows(second[k], 4), R.rows(first[k], 4), f"unaligned {k}", min_rows=MAIN_ROWS)


def test_fine_tuning_the_opacities_through_the_foveated_renderer():
    """The use the pass is for: Adam on the per-level opacities against an image rendered from other opacities, L1 loss, twenty steps:
    the loss falls below half its start; and one step against the foveated metameric loss (HVSLoss's defaults) at the frame's gaze
    gives finite, non-zero gradients."""
    _need_gpu()
    from fov3dgs_amd.hvs_loss_calc import HVSLoss
    from tests import hvs_cases as hc
    cloud, cam, bg, highest, dcs, opac0 = _model()
    with torch.no_grad():
        target = _render(cloud, cam, bg, highest, dcs, (opac0 * 0.6).contiguous())["render"]
    opac = opac0.clone().requires_grad_(True)
    opt = torch.optim.Adam([opac], lr=0.03)
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        img = _render(cloud, cam, bg, highest, dcs, opac, appearance_only=True)["render"]
        loss = (img - target).abs().mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            opac.clamp_(0.0, 1.0)
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float((_render(cloud, cam, bg, highest, dcs, opac)["render"] - target).abs().mean()))
    print("L1 loss per step", [f"{v:.4f}" for v in losses])
    assert losses[-1] < 0.5 * losses[0]
    hvs = HVSLoss(device=DEV, filters=hc.filters(6))
    opac = opac0.clone().requires_grad_(True)
    dcs.requires_grad_(True)
    img = _render(cloud, cam, bg, highest, dcs, opac, appearance_only=True)["render"]
    hvs.calc_fov_loss(img, target, gaze=list(R.MAIN["gaze"])).backward()
    torch.cuda.synchronize()
    for g in (opac.grad, dcs.grad):
        assert torch.isfinite(g).all() and (g != 0).sum() >= MAIN_ROWS


# ---- 10. - 14. the host side of the autograd path, on the faint scene ------------------------------------------------------------
# tests/fov_backward_scenes.py's `faint` (opacities x 0.1: 3034 live rows at gaze (0.4, 0.55), 1305 at (0.2, 0.35)) through
# gaussian_renderer_fov.render(..., appearance_only=True). Gradients of one graph are compared with those of the same graph run alone
# by check_grad (float atomics move the last bits from run to run) with min_rows = the scenes' MIN_LIVE.
FAINT_A, FAINT_B = dict(alpha=0.6, gaze=(0.4, 0.55)), dict(alpha=0.6, gaze=(0.2, 0.35))
from tests.backward_scenes import MIN_LIVE  # noqa: E402  (the scenes' condition: live rows of every large scene)
_alone_cache = {}


def _faint_model(settings=None):
    from tests.fov_backward_scenes import OPACITY_FACTOR
    cloud = small_cloud(3000, 3)
    L = 4 if settings is None else int(settings.levels)
    highest, dcs, opac = syn.foveation_layers(cloud, seed=4, **({} if settings is None else {"fractions": (1.0 / L,) * L}))
    return cloud.to(DEV), small_camera().to(DEV), torch.tensor(R.BG, device=DEV), highest.to(DEV), dcs.to(DEV), (opac * OPACITY_FACTOR).to(DEV)


def _faint_dL():
    return torch.tensor(R.dL_for(dict(image_height=120, image_width=200)), device=DEV)


def _graph(model, kw, **extra):
    """forward of one autograd graph -> (render dict, opacities leaf, shs_dcs leaf)"""
    cloud, cam, bg, highest, dcs, opac = model
    o, d = opac.clone().requires_grad_(True), dcs.clone().requires_grad_(True)
    return _render(cloud, cam, bg, highest, d, o, kw, appearance_only=True, **extra), o, d


def _finish(graph, dL):
    out, o, d = graph
    (out["render"] * dL).sum().backward()
    torch.cuda.synchronize()
    assert o.grad.shape == o.shape and d.grad.shape == d.shape
    return o.grad.cpu().numpy(), d.grad.cpu().numpy()


def _alone(which):
    """the gradients of graph A / B of the faint scene run alone (once per session)"""
    if which not in _alone_cache:
        _alone_cache[which] = _finish(_graph(_faint_model(), FAINT_A if which == "A" else FAINT_B), _faint_dL())
    return _alone_cache[which]


def _same(got, want, tag, L=4):
    for g, w, k in zip(got, want, ("opacities", "shs_dcs")):
        assert np.isfinite(g).all()
        check_grad(R.rows(g, L), R.rows(w, L), f"{tag} {k}", min_rows=MIN_LIVE)


def _workspaces(out):
    """addresses of the workspace buffers the graph of a render holds for its backward pass"""
    saved = out["render"].grad_fn.saved_tensors
    assert len(saved) == 3
    return {t.data_ptr() for t in saved}


def test_two_graphs_alive_at_once_keep_their_own_state():
    """forward A (gaze (0.4, 0.55)), forward B (gaze (0.2, 0.35)), backward B, backward A: each graph's gradients are those of the same
    graph run alone, and the two graphs held different workspace sets (a set shared between them would hand A's backward B's lists,
    level table and state planes)."""
    _need_gpu()
    model, dL = _faint_model(), _faint_dL()
    a = _graph(model, FAINT_A)
    b = _graph(model, FAINT_B)
    assert not (_workspaces(a[0]) & _workspaces(b[0])), "two live graphs share a workspace buffer"
    got_b = _finish(b, dL)
    got_a = _finish(a, dL)
    _same(got_b, _alone("B"), "B beside A")
    _same(got_a, _alone("A"), "A after B")
    assert not np.array_equal(got_a[0], got_b[0])


def test_a_graph_dropped_without_backward_leaves_the_next_one_intact():
    _need_gpu()
    import gc
    model, dL = _faint_model(), _faint_dL()
    dropped = _graph(model, FAINT_A)
    del dropped
    gc.collect()
    _same(_finish(_graph(model, FAINT_B), dL), _alone("B"), "after a dropped graph")
    kept = _graph(model, FAINT_A)   # ... and one dropped while another is alive
    dropped = _graph(model, FAINT_B)
    del dropped
    gc.collect()
    _same(_finish(kept, dL), _alone("A"), "beside a dropped graph")


def test_forward_and_backward_on_a_non_default_stream():
    _need_gpu()
    want = _alone("A")
    model, dL = _faint_model(), _faint_dL()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        graph = _graph(model, FAINT_A)
        (graph[0]["render"] * dL).sum().backward()
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    _same((graph[1].grad.cpu().numpy(), graph[2].grad.cpu().numpy()), want, "side stream")
    with torch.no_grad():   # the image on that stream is the default stream's
        cloud, cam, bg, highest, dcs, opac = model
        plain = _render(cloud, cam, bg, highest, dcs, opac, FAINT_A)["render"]
    torch.cuda.synchronize()
    assert torch.equal(plain, graph[0]["render"].detach())


@pytest.mark.parametrize("name", tuple(SETTINGS))
def test_two_and_three_levels_through_autograd(name):
    """render(..., foveation=settings, appearance_only=True) on fov_backward_scenes' faint-L2 / faint-L3: the gradients have the
    model's shapes [P,L] / [P,L,3] and equal the direct call's."""
    _need_gpu()
    from tests import fov_backward_scenes as fs
    settings, alpha, gaze = SETTINGS[name]
    L = settings.levels
    r = fs.reference(f"faint-{name}")
    dL = R.dL_for(r["cam"])
    direct = backward(keep_forward(r["scene"], r["cam"], settings), dL, want_colours=False)
    model = _faint_model(settings)
    np.testing.assert_allclose(model[5].cpu().numpy(), r["scene"]["opacities"], rtol=1e-6)   # (the scene of the direct call)
    got = _finish(_graph(model, dict(alpha=alpha, gaze=gaze), foveation=settings), torch.tensor(dL, device=DEV))
    assert got[0].shape == (3000, L) and got[1].shape == (3000, L, 3)
    _same(got, (direct["dL_dopacities"], direct["dL_dshs_dcs"]), f"{name} autograd vs direct", L)


def test_a_non_contiguous_upstream_gradient():
    """dL/dimage handed to backward as a [W,H,3] tensor permuted to [3,H,W] gives the contiguous tensor's gradients."""
    _need_gpu()
    model, dL = _faint_model(), _faint_dL()
    strided = dL.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    assert strided.shape == dL.shape and not strided.is_contiguous() and torch.equal(strided, dL)
    out, o, d = _graph(model, FAINT_A)
    out["render"].backward(gradient=strided)
    torch.cuda.synchronize()
    _same((o.grad.cpu().numpy(), d.grad.cpu().numpy()), _alone("A"), "strided dL")
