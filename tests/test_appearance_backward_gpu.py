"""The appearance-only backward pass (fr_backward_appearance; render(..., masking=True, appearance_only=True)): the gradients of the
opacity and of the DC colour -- all the mask-learning step differentiates (metric_mask_learn.py:213,
gaussian_renderer/__init__.py:71-82) -- from a tile pass that sums four values per (band, entry) pair instead of nine and a
per-Gaussian pass without SH rows or chain rule. Against the CPU oracle, against the full pass, and against itself (dense / row-sparse,
repeated and mixed calls over one forward state). Tolerances: tests/checks.py check_grad's defaults throughout -- the lean sums are
the full pass's terms in another fold order. Every gradient tensor starts as NaN (tests/conftest.py)."""
import ctypes as C
import math
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.checks import check_grad
from tests.helpers import cam_dict, scene_dict, small_camera, small_case, small_cloud, syn
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ARGS = SimpleNamespace(position_lr_init=0.00016, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


class Pipe:
    debug = False


def _need_gpu():
    if not torch.cuda.is_available():  # only reached by an explicit -m gpu run (tests/conftest.py skips otherwise)
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _native_backward(variant, fwd, dpix, lean, **kw):
    """fr_backward_appearance (lean) or fr_backward over the forward state `fwd` (tests/gpu_helpers.hip_forward) -> dict of numpy."""
    from fov3dgs_amd.rasterizer import _backward_native
    from tests.gpu_helpers import VARIANT_IDS, _t
    t, rs = fwd["_tensors"], fwd["_rs"]
    geom, binb, img = fwd["_buffers"]
    e = torch.Tensor([])
    opt = lambda k: t[k] if t[k] is not None else e
    if lean:
        kw["appearance_only"] = True
    g = _backward_native(VARIANT_IDS[variant], rs, t["means3D"], fwd["_radii_t"], opt("colors_precomp"), t["opacities"], opt("scales"),
                         opt("rotations"), opt("cov3D_precomp"), _t(dpix, DEV), opt("shs"), geom, fwd["num_rendered"], binb, img,
                         want_color_grad=True, **kw)
    torch.cuda.synchronize()
    names = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot")
    return {n: (None if v is None else v.cpu().numpy()) for n, v in zip(names, g)}


def _check_lean_against_oracle(got, want, tag, sh=True):
    for k in ("dL_dmean2D", "dL_dmean3D", "dL_dcov3D", "dL_dscale", "dL_drot"):
        assert got[k] is None, k  # (not computed, not allocated)
    check_grad(got["dL_dopacity"], want["dL_dopacity"], f"dL_dopacity {tag}")
    check_grad(got["dL_dcolor"], want["dL_dcolor"], f"dL_dcolor {tag}")
    if sh:
        assert got["dL_dsh"].shape == (len(want["dL_dsh"]), 1, 3)  # always the DC part, also for concatenated shs
        check_grad(got["dL_dsh"][:, 0], want["dL_dsh"][:, 0], f"dL_dsh DC {tag}")
    else:
        assert got["dL_dsh"] is None


def _oracle_pair(variant, scene, cam, seed):
    from tests.gpu_helpers import hip_forward
    want_f = orc.forward(variant, scene, cam)
    dpix = np.random.default_rng(seed).normal(size=want_f["color"].shape).astype(np.float32)
    want = orc.backward(variant, scene, cam, want_f, dpix)
    got_f = hip_forward(variant, scene, cam)
    np.testing.assert_array_equal(got_f["point_list"], want_f["point_list"])
    return want_f, want, got_f, dpix


# ---- 1. oracle parity, direct call -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ("original", "pcheck_obb_sum"))
def test_matches_the_oracle(variant):
    _need_gpu()
    scene, cam = small_case(variant)
    _, want, got_f, dpix = _oracle_pair(variant, scene, cam, 5)
    got = _native_backward(variant, got_f, dpix, lean=True)
    _check_lean_against_oracle(got, want, variant)
    assert np.abs(got["dL_dopacity"]).max() > 0 and np.abs(got["dL_dsh"]).max() > 0


@pytest.mark.parametrize("variant", ("original", "pcheck_obb_sum"))
def test_matches_the_oracle_on_an_open_scene(variant):
    """small_case hides most of its cloud behind a few large splats (some seventy rows carry a gradient); here all 1000 do."""
    _need_gpu()
    scene, cam = scene_dict(syn.scene_1k(P=1000, seed=2), variant), cam_dict(syn.camera_1k(200, 136), bg=(0.3, 0.2, 0.1))
    _, want, got_f, dpix = _oracle_pair(variant, scene, cam, 6)
    assert (np.abs(want["dL_dopacity"]) > 0).sum() >= 900
    got = _native_backward(variant, got_f, dpix, lean=True)
    _check_lean_against_oracle(got, want, variant + " (open scene)")


@pytest.mark.parametrize("variant", ("original", "pcheck_obb_sum"))
def test_matches_the_oracle_with_precomputed_colours_and_covariances(variant):
    """colors_precomp + cov3D_precomp: no SH, so no dL_dsh; dL_dcolor is the input's gradient."""
    _need_gpu()
    scene, cam = small_case(variant)
    w0 = orc.forward(variant, scene, cam)
    pre = dict(scene)
    pre["colors_precomp"] = np.random.default_rng(3).random((scene["means3D"].shape[0], 3)).astype(np.float32)
    pre["cov3D_precomp"] = w0["cov3D"]
    for k in ("shs", "scales", "rotations"):
        pre.pop(k)
    _, want, got_f, dpix = _oracle_pair(variant, pre, cam, 8)
    got = _native_backward(variant, got_f, dpix, lean=True)
    _check_lean_against_oracle(got, want, variant + " (precomputed inputs)", sh=False)


def test_matches_the_oracle_at_sh_degree_0():
    _need_gpu()
    scene, cam = small_case("pcheck_obb_sum")
    cam = dict(cam, sh_degree=0)
    _, want, got_f, dpix = _oracle_pair("pcheck_obb_sum", scene, cam, 17)
    got = _native_backward("pcheck_obb_sum", got_f, dpix, lean=True)
    _check_lean_against_oracle(got, want, "degree 0")


# ---- 2. clamped colours ----------------------------------------------------------------------------------------------------------
def test_clamped_channels_pass_no_gradient():
    """A channel the forward pass clamped at zero passes no gradient to its DC coefficient (backward.cu:20-139): exactly 0."""
    _need_gpu()
    cloud = syn.scene_1k(P=1000, seed=9)  # (nothing hides anything here: every Gaussian's colour gets a gradient)
    cloud._features_dc -= 1.5  # colour = SH_C0 dc + 0.5 + ...: about four channels in ten fall below zero
    variant = "pcheck_obb_sum"
    scene, cam = scene_dict(cloud, variant), cam_dict(syn.camera_1k(200, 120), bg=(0.1, 0.2, 0.3))
    want_f, want, got_f, dpix = _oracle_pair(variant, scene, cam, 21)
    clamped = want_f["clamped"].astype(bool)
    visible = want_f["radii"] > 0
    live = np.abs(want["dL_dcolor"]).max(axis=1) > 0
    assert (clamped.any(axis=1) & visible & live).sum() >= 50 and ((~clamped).any(axis=1) & visible & live).sum() >= 50
    got = _native_backward(variant, got_f, dpix, lean=True)
    dc = got["dL_dsh"][:, 0]
    assert np.all(dc[clamped] == 0.0)
    assert np.mean(got["dL_dcolor"][clamped & live[:, None]] != 0) > 0.99  # (the colour's own gradient is not clamped)
    _check_lean_against_oracle(got, want, "clamped")


# ---- 3. fold tails ---------------------------------------------------------------------------------------------------------------
def _big_splats(P, opacity, seed, spread=0.6, scale=0.9):
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([rng.uniform(-spread, spread, (P, 2)), rng.uniform(3.6, 4.4, (P, 1))], axis=1).astype(np.float32)
    scales = (scale * rng.uniform(0.7, 1.3, (P, 3))).astype(np.float32)
    rot = rng.normal(size=(P, 4)).astype(np.float32)
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    shs = np.concatenate([rng.normal(size=(P, 1, 3)), 0.1 * rng.normal(size=(P, 15, 3))], axis=1).astype(np.float32)
    return dict(means3D=xyz, scales=scales, rotations=rot, opacities=np.full((P, 1), opacity, np.float32), shs=shs)


@pytest.mark.parametrize("variant", ("original", "pcheck_obb_sum"))
@pytest.mark.parametrize("P", (1, 2, 3, 5))
def test_short_lists_take_every_tail_of_the_fold(P, variant):
    """The lean tile pass folds the sums of two entries together: lists of 1, 2, 3 and 5 entries (large splats over several tiles)
    end with one entry pending or none, after zero, one or two full folds."""
    _need_gpu()
    scene = _big_splats(P, 0.6, seed=40 + P)
    cam = cam_dict(syn.camera_1k(200, 120), bg=(0.2, 0.1, 0.0))
    want_f, want, got_f, dpix = _oracle_pair(variant, scene, cam, 50 + P)
    n = want_f["ranges"][:, 1].astype(int) - want_f["ranges"][:, 0].astype(int)
    assert n.max() == P and (n == P).sum() >= 4  # several tiles hold all P splats
    got = _native_backward(variant, got_f, dpix, lean=True)
    _check_lean_against_oracle(got, want, f"P={P} {variant}")
    # (check_grad's outlier share means nothing for a handful of rows: its whole-tensor bounds -- cosine, relative L2 -- decide,
    # and a fold that dropped or doubled an entry is off by the entry)
    assert np.all(got["dL_dopacity"][want_f["radii"] > 0] != 0)


def test_translucent_wall_consumes_its_lists():
    """Several hundred faint splats per tile: every list is walked to its end, in batches of 64, with odd and even numbers of
    entries reaching a band."""
    _need_gpu()
    variant = "pcheck_obb_sum"
    scene = _big_splats(601, 0.03, seed=7, spread=1.6, scale=0.45)
    cam = cam_dict(syn.camera_1k(200, 120), bg=(0.0, 0.1, 0.2))
    want_f, want, got_f, dpix = _oracle_pair(variant, scene, cam, 71)
    n = want_f["ranges"][:, 1].astype(int) - want_f["ranges"][:, 0].astype(int)
    assert n.max() >= 300 and len(set(n.tolist())) > 20
    # consumed to the end: the deepest contributor of nearly every pixel is (nearly) the last entry of its list
    assert np.median(want_f["n_contrib"]) >= 200 and want_f["final_T"].min() > 1e-4
    got = _native_backward(variant, got_f, dpix, lean=True)
    _check_lean_against_oracle(got, want, "translucent wall")


# ---- 4. every element written ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (20037, 64, 33))
def test_every_element_is_written_with_clustered_visibility(P):
    """The pattern of test_narrow_gradient_tensors_with_clustered_visibility: runs behind the camera, a single visible row every
    701, a cut-off last group. The dense lean outputs (one fill, then the visible rows) are finite, zero where radii == 0 and
    equal to the row-sparse lean call (every compact row stored, nothing filled) densified."""
    _need_gpu()
    from fov3dgs_amd.gaussian_renderer import render
    cam = syn.camera_1k(200, 136).to(DEV)
    bg = torch.tensor([0.1, 0.0, 0.2], device=DEV)
    hidden = np.zeros(P, bool)
    if P > 1000:
        hidden[:3000] = True
        hidden[5000:5032] = True
        hidden[5056:5088] = True
        hidden[9000:17000] = True
        hidden[9000:17000:701] = False
        hidden[P - 50:P - 3] = True
    else:
        hidden[P // 2:] = True
    w, res = None, []
    for sparse in (False, True):
        cloud = small_cloud(P=P, seed=31)
        with torch.no_grad():
            cloud._xyz[torch.from_numpy(hidden), 2] = -6.0  # behind the camera
        cloud = cloud.to(DEV).requires_grad_(True)
        cloud.fuse_activations = True
        cloud.row_sparse_grads = sparse
        out = render(cam, cloud, Pipe(), bg, masking=True, cuda_type="pcheck_obb_sum", appearance_only=True)
        if w is None:
            w = torch.randn_like(out["render"])
        (out["render"] * w).sum().backward()
        assert cloud._opacity.grad.is_sparse == sparse and cloud._features_dc.grad.is_sparse == sparse
        grads = dict(opacity=cloud._opacity.grad, f_dc=cloud._features_dc.grad)
        res.append(({k: (g.to_dense() if g.is_sparse else g).cpu().numpy() for k, g in grads.items()}, out["radii"].cpu().numpy()))
    (dense, radii), (sp, radii2) = res
    np.testing.assert_array_equal(radii, radii2)
    assert not (radii[hidden] > 0).any() and (radii[~hidden] > 0).sum() > (~hidden).sum() // 8
    for k in dense:
        assert np.isfinite(dense[k]).all(), k
        check_grad(dense[k], sp[k], "clustered visibility, dense vs row-sparse lean " + k)
        assert not np.abs(dense[k].reshape(P, -1))[radii == 0].any(), k
        assert np.abs(dense[k]).max() > 0, k


# ---- 5. lean equals full through render() ----------------------------------------------------------------------------------------
def _camera(kind):
    return (syn.camera_1k(200, 120) if kind.endswith("-open") else small_camera()).to(DEV)


def _model(kind, seed=3, P=3000):
    """small_cloud hides most of itself behind a few large splats (some seventy rows carry a gradient); the -open kinds render
    scene_1k, where every Gaussian is seen."""
    if kind.endswith("-open"):
        cloud, kind = syn.scene_1k(P=1000, seed=seed).to(DEV).requires_grad_(True), kind[:-5]
    else:
        cloud = small_cloud(P, seed).to(DEV).requires_grad_(True)
    if kind == "cloud-fused":
        cloud.fuse_activations = True
        return cloud, cloud
    if kind == "cloud":
        return cloud, cloud
    if kind == "reference-shaped":
        return cloud, syn.ReferenceShapedModel(cloud)
    raise ValueError(kind)


def _render_step(kind, lean, w=None, extra=None):
    from fov3dgs_amd.gaussian_renderer import render
    cloud, model = _model(kind)
    cam = _camera(kind)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    kw = dict(appearance_only=True) if lean else {}
    out = render(cam, model, Pipe(), bg, masking=True, cuda_type="pcheck_obb_sum", **kw)
    if w is None:
        w = torch.randn(out["render"].shape, device=DEV, generator=torch.Generator(DEV).manual_seed(11))
    (out["render"] * w).sum().backward()
    return cloud, out, w


@pytest.mark.parametrize("kind", ("cloud-fused", "cloud", "reference-shaped", "cloud-fused-open", "reference-shaped-open"))
def test_lean_equals_full_through_render(kind):
    _need_gpu()
    full, out_f, w = _render_step(kind, lean=False)
    lean, out_l, _ = _render_step(kind, lean=True, w=w)
    assert torch.equal(out_f["radii"], out_l["radii"])
    if kind.startswith("reference-shaped"):
        # With appearance_only the reference model is rendered from its RAW parameters again (the kernels' own exp / sigmoid), the
        # plain masking call from its getters (torch's): the two forward passes differ in the activations' last bit, as
        # INTEGRATION.md documents for FAST_REFERENCE_MODEL -- bit-identity is asked of the call that takes the same forward path
        # (the same model without masking), and the getter path's image must agree within the image tolerance.
        from fov3dgs_amd.gaussian_renderer import render
        from tests.checks import check_image
        with torch.no_grad():
            same_path = render(_camera(kind), _model(kind)[1], Pipe(), torch.tensor([0.1, 0.2, 0.3], device=DEV), cuda_type="pcheck_obb_sum")
        assert torch.equal(same_path["render"], out_l["render"])
        check_image(out_l["render"].detach().cpu().numpy(), out_f["render"].detach().cpu().numpy(), name="raw parameters vs getters")
    else:
        assert torch.equal(out_f["render"], out_l["render"])
    assert out_l["viewspace_points"].requires_grad is False and not out_l["viewspace_points"].any()
    if kind.endswith("-open"):
        assert int((full._opacity.grad != 0).sum()) >= 900
    for name in ("_opacity", "_features_dc"):
        g, want = getattr(lean, name).grad, getattr(full, name).grad
        assert g is not None and g.shape == getattr(lean, name).shape and float(want.abs().max()) > 0
        check_grad(g.cpu().numpy(), want.cpu().numpy(), f"{kind} {name}.grad lean vs full")
    for name in ("_xyz", "_features_rest"):
        assert getattr(lean, name).grad is None and getattr(full, name).grad is None, name
    for name in ("_scaling", "_rotation"):
        for which, m in (("lean", lean), ("full", full)):
            g = getattr(m, name).grad
            # GaussianCloud.get_activated is ONE autograd function over (scaling, rotation, opacity) (activations.activate): asked for
            # the opacity's gradient it hands zeros to its two other inputs, with or without appearance_only. The raw-parameter path
            # and the reference model's getters give them nothing.
            if kind == "cloud" or (kind.startswith("cloud-fused") and which == "full"):
                assert g is None or not g.any(), (name, which)
            else:
                assert g is None, (name, which)


# ---- 6. raw against activated ----------------------------------------------------------------------------------------------------
def test_raw_opacity_gradient_is_the_activated_one_through_the_sigmoid():
    _need_gpu()
    from fov3dgs_amd.gaussian_wrapper import get_gs_rasterizer
    from fov3dgs_amd.rasterizer import GaussianRasterizationSettings
    cam = small_camera().to(DEV)
    rs = GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        bg=torch.tensor([0.1, 0.2, 0.3], device=DEV), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=3, campos=cam.camera_center, prefiltered=False, debug=False)
    rast = get_gs_rasterizer("pcheck_obb_sum", rs)
    grads, w = [], None
    for raw in (True, False):
        c = small_cloud(3000, 3).to(DEV)
        c._opacity.requires_grad_(True)
        m2 = torch.zeros_like(c._xyz)
        shs = (c._features_dc, c._features_rest)
        if raw:
            out = rast(means3D=c._xyz, means2D=m2, shs=shs, opacities=c._opacity, scales=c._scaling, rotations=c._rotation,
                       raw_activations=True, appearance_only=True)
        else:
            out = rast(means3D=c._xyz, means2D=m2, shs=shs, opacities=torch.sigmoid(c._opacity), scales=torch.exp(c._scaling),
                       rotations=torch.nn.functional.normalize(c._rotation), appearance_only=True)
        if w is None:
            w = torch.randn_like(out[0])
        (out[0] * w).sum().backward()
        grads.append(c._opacity.grad.cpu().numpy())
    assert np.abs(grads[1]).max() > 0
    check_grad(grads[0], grads[1], "raw _opacity.grad: kernel's o (1 - o) vs torch.sigmoid's backward")


# ---- 7. getter override ----------------------------------------------------------------------------------------------------------
def test_a_model_that_overrides_a_getter_keeps_its_getters():
    """synthetic.MaskedOpacityModel: opacity times a learned mask. render() must go through its getter also with appearance_only
    (the gradient reaches _mask through torch); it offers no split SH, so the full backward pass runs, with one warning."""
    _need_gpu()
    from fov3dgs_amd import gaussian_renderer as gr
    res, w = [], None
    for lean in (False, True):
        cloud = small_cloud(3000, 3).to(DEV).requires_grad_(True)
        mask = torch.full((3000, 1), 0.7, device=DEV).requires_grad_(True)
        model = syn.MaskedOpacityModel(cloud, mask)
        cam, bg = small_camera().to(DEV), torch.tensor([0.1, 0.2, 0.3], device=DEV)
        if lean:
            gr._warned_no_split = False
            with pytest.warns(UserWarning, match="no split SH"):
                out = gr.render(cam, model, Pipe(), bg, masking=True, cuda_type="pcheck_obb_sum", appearance_only=True)
            with warnings.catch_warnings(record=True) as again:  # ... once
                warnings.simplefilter("always")
                gr.render(cam, model, Pipe(), bg, masking=True, cuda_type="pcheck_obb_sum", appearance_only=True)
            assert not [x for x in again if "no split SH" in str(x.message)]
            assert out["viewspace_points"].requires_grad is False
        else:
            out = gr.render(cam, model, Pipe(), bg, masking=True, cuda_type="pcheck_obb_sum")
        if w is None:
            w = torch.randn_like(out["render"])
        (out["render"] * w).sum().backward()
        res.append((mask.grad.cpu().numpy(), cloud._opacity.grad.cpu().numpy(), cloud._features_dc.grad.cpu().numpy(), cloud))
    assert np.abs(res[1][0]).max() > 0
    for i, name in enumerate(("_mask", "_opacity", "_features_dc")):
        check_grad(res[1][i], res[0][i], f"masked-opacity model {name}.grad, appearance_only vs full")
    assert res[1][3]._xyz.grad is None and res[1][3]._features_rest.grad is None


# ---- 8. idempotence and mixing over one forward state ----------------------------------------------------------------------------
def test_repeated_and_mixed_calls_over_one_forward_state():
    """The gradient sums in the geometry workspace are cleared by whoever read them: lean after lean, full after lean and lean after
    full over ONE forward state each give what a fresh single call gives."""
    _need_gpu()
    from tests.gpu_helpers import hip_forward
    variant = "pcheck_obb_sum"
    scene, cam = small_case(variant)
    dpix = np.random.default_rng(12).normal(size=(3, cam["image_height"], cam["image_width"])).astype(np.float32)
    ref_full = _native_backward(variant, hip_forward(variant, scene, cam), dpix, lean=False)  # fresh single calls
    fwd = hip_forward(variant, scene, cam)
    ref_lean = _native_backward(variant, fwd, dpix, lean=True)

    def same(got, want, tag, keys):
        for k in keys:
            check_grad(got[k], want[k].reshape(got[k].shape), f"{k} {tag}")
    lean_keys = ("dL_dopacity", "dL_dcolor", "dL_dsh")
    full_keys = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dsh", "dL_dscale", "dL_drot")
    same(_native_backward(variant, fwd, dpix, lean=True), ref_lean, "lean after lean", lean_keys)
    same(_native_backward(variant, fwd, dpix, lean=False), ref_full, "full after lean", full_keys)
    same(_native_backward(variant, fwd, dpix, lean=True), ref_lean, "lean after full", lean_keys)
    same(_native_backward(variant, fwd, dpix, lean=False), ref_full, "full after lean after full", full_keys)
    check_grad(ref_lean["dL_dsh"][:, 0], ref_full["dL_dsh"][:, 0], "fresh lean vs fresh full DC")


def test_backward_twice_over_one_graph():
    _need_gpu()
    from fov3dgs_amd.gaussian_renderer import render
    cloud, model = _model("reference-shaped")
    out = render(small_camera().to(DEV), model, Pipe(), torch.zeros(3, device=DEV), masking=True, cuda_type="pcheck_obb_sum", appearance_only=True)
    loss = (out["render"] * torch.randn_like(out["render"])).sum()
    got = []
    for _ in range(2):
        cloud._opacity.grad = cloud._features_dc.grad = None
        loss.backward(retain_graph=True)
        got.append((cloud._opacity.grad.cpu().numpy(), cloud._features_dc.grad.cpu().numpy()))
    assert np.abs(got[0][0]).max() > 0
    check_grad(got[1][0], got[0][0], "_opacity.grad, second backward over the graph")
    check_grad(got[1][1], got[0][1], "_features_dc.grad, second backward over the graph")


# ---- 9. row-sparse ---------------------------------------------------------------------------------------------------------------
def test_row_sparse_gradients():
    _need_gpu()
    from fov3dgs_amd import optim
    from fov3dgs_amd.gaussian_renderer import render
    cam, bg = small_camera().to(DEV), torch.tensor([0.1, 0.2, 0.3], device=DEV)
    res, w = {}, None
    for sparse in (False, True):
        cloud = small_cloud(3000, 3).to(DEV).requires_grad_(True)
        cloud.fuse_activations, cloud.row_sparse_grads = True, sparse
        out = render(cam, cloud, Pipe(), bg, masking=True, cuda_type="pcheck_obb_sum", appearance_only=True)
        if w is None:
            w = torch.randn_like(out["render"])
        (out["render"] * w).sum().backward()
        res[sparse] = (cloud, out)
    dense, (cloud, out) = res[False][0], res[True]
    for name in ("_opacity", "_features_dc"):
        g = getattr(cloud, name).grad
        assert g.layout == torch.sparse_coo and g.is_coalesced() and g.sparse_dim() == 1, name
        rows = g._indices()[0]
        assert bool((rows[1:] > rows[:-1]).all()) and rows.numel() >= int((out["radii"] > 0).sum())
        assert g._values().shape[1:] == getattr(cloud, name).shape[1:]
        check_grad(g.to_dense().cpu().numpy(), getattr(dense, name).grad.cpu().numpy(), f"{name}.grad row-sparse vs dense lean")
    for name in ("_xyz", "_features_rest", "_scaling", "_rotation"):
        assert getattr(cloud, name).grad is None, name
    before = {n: getattr(cloud, n).detach().clone() for n in PARAMS}
    opt = optim.Adam(optim.reference_param_groups(cloud, ARGS), lr=0.0, eps=1e-15, sparse="exact")
    opt.step()
    torch.cuda.synchronize()
    touched = (cloud._opacity.grad.to_dense() != 0).squeeze(1)
    assert bool((cloud._opacity.detach() != before["_opacity"]).squeeze(1)[touched].all())
    assert torch.equal(cloud._opacity.detach()[~touched], before["_opacity"][~touched])
    for name in ("_xyz", "_features_rest", "_scaling", "_rotation"):
        assert torch.equal(getattr(cloud, name).detach(), before[name]), name


# ---- 10. one mask step end to end ------------------------------------------------------------------------------------------------
def test_one_mask_step_end_to_end():
    """render -> fused L1 + SSIM -> backward -> optim.Adam.step() with the reference's six parameter groups: opacity and DC move as
    in the full-path step, everything else stays bit for bit and gets no optimizer state."""
    _need_gpu()
    from fov3dgs_amd import optim
    from fov3dgs_amd.gaussian_renderer import render
    from fov3dgs_amd.loss_utils import l1_ssim_loss
    cam, bg = syn.camera_1k(200, 120).to(DEV), torch.tensor([0.1, 0.2, 0.3], device=DEV)
    target = torch.rand(3, cam.image_height, cam.image_width, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    after, start = {}, None
    for lean in (False, True):
        cloud = syn.scene_1k(P=1000, seed=5).to(DEV).requires_grad_(True)  # (an open scene: small_cloud hides most of itself)
        model = syn.ReferenceShapedModel(cloud)
        start = {n: getattr(cloud, n).detach().clone() for n in PARAMS}
        opt = optim.Adam(optim.reference_param_groups(cloud, ARGS), lr=0.0, eps=1e-15)
        kw = dict(appearance_only=True) if lean else {}
        out = render(cam, model, Pipe(), bg, masking=True, cuda_type="pcheck_obb_sum", **kw)
        l1_ssim_loss(out["render"], target, 0.2).backward()
        print("lean" if lean else "full", "rows with a gradient:", {n: int((getattr(cloud, n).grad.reshape(len(cloud._xyz), -1) != 0).any(dim=1).sum())
                                                                     for n in ("_opacity", "_features_dc")},
              "largest:", {n: float(getattr(cloud, n).grad.abs().max()) for n in ("_opacity", "_features_dc")})
        opt.step()
        torch.cuda.synchronize()
        after[lean] = {n: getattr(cloud, n).detach().clone() for n in PARAMS}
        print("lean" if lean else "full", "rows moved:", {n: int((after[lean][n] != start[n]).reshape(len(start[n]), -1).any(dim=1).sum())
                                                           for n in ("_opacity", "_features_dc")})
        for n in ("_xyz", "_features_rest", "_scaling", "_rotation"):
            assert torch.equal(after[lean][n], start[n]), n
            assert len(opt.state[getattr(cloud, n)]) == 0, n  # no Adam state was created for it
        for n in ("_opacity", "_features_dc"):
            assert float(opt.state[getattr(cloud, n)]["step"]) == 1.0
    for n in ("_opacity", "_features_dc"):
        moved = (after[True][n] != start[n]).reshape(len(start[n]), -1).any(dim=1)
        assert int(moved.sum()) >= 900, n  # (every Gaussian of this cloud is seen)
        print(n, "max |lean - full| after the step:", float((after[True][n] - after[False][n]).abs().max()))
        np.testing.assert_allclose(after[True][n].cpu().numpy(), after[False][n].cpu().numpy(), rtol=1e-4, atol=0)


# ---- 11. diagnostics and contract ------------------------------------------------------------------------------------------------
def test_blend_pairs_and_range_done():
    _need_gpu()
    from fov3dgs_amd import rasterizer
    from tests.gpu_helpers import hip_forward
    variant = "pcheck_obb_sum"
    scene, cam = small_case(variant)
    P = scene["means3D"].shape[0]
    T = ((cam["image_width"] + 15) // 16) * ((cam["image_height"] + 15) // 16)
    dpix = np.random.default_rng(4).normal(size=(3, cam["image_height"], cam["image_width"])).astype(np.float32)
    fwd = hip_forward(variant, scene, cam)
    pairs = {}
    calls = []
    for lean in (True, False):
        pairs[lean] = torch.full((T,), -1, dtype=torch.int32, device=DEV)
        rasterizer.GRADIENT_RANGE_HOOK = (lambda k, lo, hi, grads: calls.append((k, lo, hi, sorted(n for n, g in grads.items() if g is not None)))) if lean else None
        try:
            _native_backward(variant, fwd, dpix, lean=lean, blend_pairs=pairs[lean])
        finally:
            rasterizer.GRADIENT_RANGE_HOOK = None
    assert int(pairs[False].sum()) > 0
    assert torch.equal(pairs[True], pairs[False])
    assert calls == [(0, 0, P, ["opacities", "sh"])]
    # row-sparse: the rows are not Gaussian indices, nobody is told
    rasterizer.GRADIENT_RANGE_HOOK = lambda *a: calls.append(a)
    try:
        from tests.gpu_helpers import vis_list_of, VARIANT_IDS
        from fov3dgs_amd import _native
        C_rows = len(vis_list_of(_native.load(), VARIANT_IDS[variant], P, fwd["_buffers"][0]))
        sp = _native_backward(variant, fwd, dpix, lean=True, row_sparse=True, num_candidates=C_rows)
    finally:
        rasterizer.GRADIENT_RANGE_HOOK = None
    assert len(calls) == 1 and sp["dL_dopacity"].shape == (C_rows, 1) and sp["dL_dsh"].shape == (C_rows, 1, 3)


def test_a_forbidden_pointer_is_refused():
    _need_gpu()
    from fov3dgs_amd import _native
    lib = _native.load()
    buf = torch.zeros(64, device=DEV)
    for field in ("dL_dmean3D", "dL_dscale", "dL_dsh_rest"):
        a = _native.BackwardArgs()
        a.variant, a.P = 1, 16
        a.dL_dopacity = buf.data_ptr()
        setattr(a, field, buf.data_ptr())
        assert lib.fr_backward_appearance(C.byref(a)) == -1
        assert field in _native.last_error()
    assert not buf.any()


def test_value_errors():
    _need_gpu()
    from fov3dgs_amd.gaussian_renderer import render
    cam, bg = small_camera().to(DEV), torch.zeros(3, device=DEV)
    cloud = small_cloud(200, 3).to(DEV).requires_grad_(True)
    with pytest.raises(ValueError, match="masking=True"):
        render(cam, cloud, Pipe(), bg, cuda_type="pcheck_obb_sum", appearance_only=True)
    from fov3dgs_amd.gaussian_wrapper import get_gs_rasterizer
    from fov3dgs_amd.rasterizer import GaussianRasterizationSettings
    rs = GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=3,
        campos=cam.camera_center, prefiltered=False, debug=False)
    rast = get_gs_rasterizer("pcheck_obb_sum", rs)
    m2 = torch.zeros_like(cloud._xyz)
    common = dict(means2D=m2, opacities=cloud.get_opacity, scales=cloud.get_scaling.detach(), rotations=cloud.get_rotation.detach())
    with pytest.raises(ValueError, match="means3D"):
        rast(means3D=cloud._xyz, shs=cloud.get_features_split_detach_rest, appearance_only=True, **common)
    with pytest.raises(ValueError, match="split form"):
        rast(means3D=cloud._xyz.detach(), shs=cloud.get_features_detach_rest, appearance_only=True, **common)
    with pytest.raises(ValueError, match="rest SH"):
        rast(means3D=cloud._xyz.detach(), shs=cloud.get_features_split, appearance_only=True, **common)
    # ... and the same inputs detached are fine
    out = rast(means3D=cloud._xyz.detach(), shs=cloud.get_features_split_detach_rest, appearance_only=True, **common)
    out[0].sum().backward()
    assert cloud._opacity.grad is not None and cloud._features_dc.grad is not None and cloud._xyz.grad is None
