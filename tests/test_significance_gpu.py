"""LightGaussian's global-significance pruning on the MI355X: the counting render against the per-pixel numpy replay of the oracle
(tests/significance_ref.py), the order statistic against torch.sort(stable=True), the percentile mask and the volume-weighted score
against the reference's torch expressions, and the whole prune against boolean indexing.

The counts are compared with the fp32 replay under two conditions that come from the arithmetic, not from what the kernel gives: at
most 2e-3 of the rows may differ (the project's figure for the _max flavour's per-pixel count, tests/test_gpu_parity.py) and no row
by more than 2 -- a (pixel, Gaussian) pair whose alpha >= 1/255 or T (1 - alpha) >= 1e-4 decision lies inside the rounding of
v_exp_f32 / the ln(255 o) threshold moves one hit, and the fp32, fp64 and contracted replays agree in every row of these scenes."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native, lightgaussian, optim
from fov3dgs_amd import compress_diff_gaussian_rasterization as cdgr
from fov3dgs_amd import synthetic as syn
from fov3dgs_amd.activations import activate
from fov3dgs_amd.rasterizer import _forward_begin, pack_model
from tests import parity_report, prune_ref
from tests import significance_ref as sref
from tests.adam_ref import ATTRS, NAMES
from tests.gpu_helpers import _t, _view, settings_from
from tests.helpers import GOLDEN, cam_dict, scene_dict, small_camera, small_cloud

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BG = (0.1, 0.2, 0.3)
ROWS_FRAC, ROW_MAX = 2e-3, 2


class Pipe:
    debug = False
    compute_cov3D_python = False
    convert_SHs_python = False


def _need_gpu():
    assert torch.cuda.is_available(), "this test needs the MI355X"


# ---- the counting render ---------------------------------------------------------------------------------------------
def _cloud(name):
    with torch.no_grad():
        if name == "A":
            cloud = small_cloud(3000, 3, big_fraction=0.01)
            cloud._opacity -= 1.0
            return cloud, small_camera(200, 120)
        if name == "B":
            return small_cloud(3000, 5, 0.02), small_camera(200, 120)
        cloud = small_cloud(1500, 7, 0.0)
        cloud._opacity += 1.0
        return cloud, small_camera(104, 72)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(cloud, scene, cam, fp32 replay) of scene A, B or C: computed once, shared, left unchanged"""
    cloud, camera = _cloud(name)
    scene, cam = scene_dict(cloud, "original"), cam_dict(camera, bg=BG)
    return cloud, scene, cam, sref.validated(scene, cam, np.float32)


def count_forward(scene, cam, count=True, packed=False, raw=False, debug=False):
    """One ORIGINAL call on oracle-style inputs -> dict(color, radii, final_T, n_contrib[, counts, score]) of device tensors"""
    lib = _native.load()
    rs = settings_from(cam, DEV, debug)
    tens = {k: _t(scene.get(k), DEV) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    pk = pack_model(tens["means3D"], tens["scales"], tens["rotations"], tens["opacities"], shs=tens["shs"]) if packed else None
    res = _forward_begin(0, rs, tens["means3D"], tens["shs"], None, tens["opacities"], tens["scales"], tens["rotations"], None,
                         packed=pk, raw_activations=raw, count=count).finish()
    torch.cuda.synchronize()
    W, H, img = rs.image_width, rs.image_height, res[5]
    out = dict(color=res[1], radii=res[2], num_rendered=res[0], _lease=res[-1])
    if tens["means3D"].shape[0] > 0:
        out["final_T"] = _view(img, lib.fr_image_final_T(0, W, H, img.data_ptr()), W * H, torch.float32).clone()
        out["n_contrib"] = _view(img, lib.fr_image_n_contrib(0, W, H, img.data_ptr()), W * H, torch.int32).clone()
    if count:
        out["counts"], out["score"] = res[6], res[7]
    return out


def _same_frame(a, b, what):
    for k in ("color", "radii", "final_T", "n_contrib"):
        if k in a or k in b:
            assert torch.equal(a[k], b[k]), f"{what}: {k} differs between the counting and the plain call"


def _product_score(counts, opacity):
    return (counts.double() * opacity.reshape(-1).double()).float()


@pytest.mark.parametrize("name", ("A", "B", "C"))
def test_counting_render_against_the_replay(name):
    _need_gpu()
    cloud, scene, cam, rep = _case(name)
    P = scene["means3D"].shape[0]
    op = _t(scene["opacities"], DEV)
    got = count_forward(scene, cam)
    assert got["counts"].dtype == torch.int32 and got["counts"].shape == (P,) and got["score"].dtype == torch.float32
    # the frame is the plain call's, bit for bit -- also with the packed layout
    _same_frame(got, count_forward(scene, cam, count=False), f"scene {name}")
    pk = count_forward(scene, cam, packed=True)
    _same_frame(pk, count_forward(scene, cam, count=False, packed=True), f"scene {name}, packed")
    assert torch.equal(pk["score"], _product_score(pk["counts"], op))
    # the same bits on every run (the second one with a synchronisation after every kernel and the fills on the launch stream)
    again = count_forward(scene, cam, debug=True)
    assert torch.equal(again["counts"], got["counts"]) and torch.equal(again["score"], got["score"])
    # the score is the product definition of the call's own counts, with the opacity the blend used
    assert torch.equal(got["score"], _product_score(got["counts"], op))
    raw_scene = dict(scene, scales=cloud._scaling.numpy(), rotations=cloud._rotation.numpy(), opacities=cloud._opacity.numpy())
    rw = count_forward(raw_scene, cam, raw=True)
    _same_frame(rw, count_forward(raw_scene, cam, count=False, raw=True), f"scene {name}, raw")
    dev_op = activate(cloud._scaling.to(DEV), cloud._rotation.to(DEV), cloud._opacity.to(DEV))[2]
    assert torch.equal(rw["score"], _product_score(rw["counts"], dev_op))
    # the counts against the fp32 replay
    hits = torch.from_numpy(rep["hits"]).to(DEV)
    d = (got["counts"].long() - hits).abs()
    rows, worst, total = int((d > 0).sum()), int(d.max()), int(d.sum())
    # (for information: the product definition against a serial fp32 running sum of the opacity, the reference's rounding)
    serial = sref.serial_fp32_score(rep["hits"], scene["opacities"])
    prod = _product_score(hits, op).cpu().numpy()
    nz = serial > 0
    serial_rel = float(np.abs(prod[nz] - serial[nz]).max() / np.abs(serial[nz]).max()) if nz.any() else 0.0
    serial_rel_row = float((np.abs(prod[nz] - serial[nz]) / serial[nz]).max()) if nz.any() else 0.0
    parity_report.record("significance", f"counting render, scene {name}", P=P, rows_hit=int((hits > 0).sum()), hits=int(hits.sum()),
                         gpu_hits=int(got["counts"].long().sum()), rows_differing=rows, max_abs_diff=worst, sum_abs_diff=total,
                         replay_final_T_err=rep["final_T_err"], product_vs_serial_fp32_rel=serial_rel, product_vs_serial_fp32_rel_row=serial_rel_row)
    print(f"scene {name}: rows hit {int((hits > 0).sum())}, hits {int(hits.sum())} (GPU {int(got['counts'].long().sum())}), rows differing {rows}, "
          f"max |d| {worst}, sum |d| {total}, product vs serial fp32 {serial_rel_row:.3g}")
    assert rows <= ROWS_FRAC * P, f"scene {name}: {rows} of {P} rows differ from the fp32 replay"
    assert worst <= ROW_MAX, f"scene {name}: a row differs from the fp32 replay by {worst}"


def _exact_case(scene, cam, what):
    rep = sref.agreed_hits(scene, cam)  # fp32 and fp64 replays agree in every row: nothing sits on a rounding boundary
    got = count_forward(scene, cam)
    _same_frame(got, count_forward(scene, cam, count=False), what)
    hits = torch.from_numpy(rep["hits"]).to(DEV)
    assert torch.equal(got["counts"].long(), hits), f"{what}: {(got['counts'].long() - hits).abs().max()} off the replay"
    assert torch.equal(got["score"], _product_score(got["counts"], _t(scene["opacities"], DEV)))
    assert torch.equal(got["n_contrib"].cpu().reshape(rep["n_contrib"].shape), torch.from_numpy(rep["n_contrib"].astype(np.int32)))
    return rep, got


def _identical(n, xyz, scale, opacity):
    g = np.random.default_rng(1)
    shs = np.zeros((n, 16, 3), np.float32)
    shs[:, 0, :] = g.random((1, 3)).astype(np.float32)
    rot = np.zeros((n, 4), np.float32)
    rot[:, 0] = 1.0
    return dict(means3D=np.tile(np.asarray(xyz, np.float32), (n, 1)), scales=np.full((n, 3), scale, np.float32), rotations=rot,
                opacities=np.full((n, 1), opacity, np.float32), shs=shs)


def test_counting_render_empty_cloud():
    _need_gpu()
    _, scene, cam, _ = _case("C")
    empty = {k: v[:0] for k, v in scene.items()}
    got = count_forward(empty, cam)
    assert got["counts"].shape == (0,) and got["score"].shape == (0,) and got["radii"].shape == (0,) and got["num_rendered"] == 0
    # the image of the plain call with no Gaussians, bit for bit: the reference returns its zero-initialised tensor when P == 0
    # (rasterize_points.cu:165, :181), and so does fr_forward for every variant -- not the background
    plain = count_forward(empty, cam, count=False)
    assert torch.equal(got["color"], plain["color"]) and not got["color"].any()


def test_counting_render_five_full_batches_in_one_tile():
    """300 identical faint Gaussians over one tile of a 32 x 32 image: five 64-entry batches (the last one partial) in which every entry
    hits every lane of both bands, and nothing saturates (0.98^300 = 2e-3)."""
    _need_gpu()
    camera = syn.camera_1k(32, 32, 60.0)
    fx = 16.0 / np.tan(np.radians(30.0))
    z = 4.0
    xyz = ((7.5 - 15.5) * z / fx, (7.5 - 15.5) * z / fx, z)  # projects to the middle of tile (0, 0)
    scene, cam = _identical(300, xyz, 1.0, 0.02), cam_dict(camera, bg=BG)
    rep, got = _exact_case(scene, cam, "300 identical Gaussians")
    hits = rep["hits"]
    assert rep["longest"] == 300 and (hits == hits[0]).all() and hits[0] >= 256 and rep["saturated"] == 0
    first_tile = rep["n_contrib"][:16, :16]
    assert (first_tile == 300).all()  # every pixel of the tile accumulated the whole list


def test_counting_render_one_splat_over_every_tile():
    """One splat larger than an 80 x 48 image: its count is summed across 15 tiles and both bands of each."""
    _need_gpu()
    camera = syn.camera_1k(80, 48, 60.0)
    scene, cam = _identical(1, (0.0, 0.0, 4.0), 3.0, 0.8), cam_dict(camera, bg=BG)
    rep, got = _exact_case(scene, cam, "one giant splat")
    assert got["num_rendered"] == 15 and int(rep["hits"][0]) == 80 * 48


# ---- select, mask, score -----------------------------------------------------------------------------------------------
SELECT_SIZES = (1, 2, 255, 256, 257, 4097, 100_003)


def _ranks(P):
    return sorted({0, P // 3, P - 1})


def _same_value(a, b):
    return bool(torch.equal(a, b) or (torch.isnan(a).all() and torch.isnan(b).all()))


def _float_inputs(P):
    g = torch.Generator().manual_seed(P)
    rnd = torch.randn(P, generator=g)
    tie = torch.where(torch.rand(P, generator=g) < 0.9, torch.zeros(()), torch.rand(P, generator=g))  # 90 % zeros: the ranks fall inside the tie
    zeros = torch.where(torch.rand(P, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    zeros = torch.where(torch.rand(P, generator=g) < 0.2, torch.randn(P, generator=g), zeros)
    inf = torch.where(torch.rand(P, generator=g) < 0.3, torch.tensor(float("inf")), rnd)
    inf = torch.where(torch.rand(P, generator=g) < 0.2, torch.tensor(float("-inf")), inf)
    nan = torch.where(torch.rand(P, generator=g) < 0.4, torch.tensor(float("nan")), rnd)
    return {"random": rnd, "tie at zero": tie, "signed zeros": zeros, "inf": inf, "nan": nan, "all nan": torch.full((P,), float("nan"))}


@pytest.mark.parametrize("P", SELECT_SIZES)
def test_kth_value_is_the_sorted_element(P):
    _need_gpu()
    for what, v in _float_inputs(P).items():
        v = v.to(DEV)
        want = torch.sort(v, stable=True)[0]
        for k in _ranks(P):
            got = lightgaussian.kth_value(v, k)
            assert got.dtype == torch.float32 and got.dim() == 0
            assert _same_value(got, want[k]), f"{what}, P={P}, k={k}: {got.item()} != {want[k].item()}"
        assert _same_value(lightgaussian.kth_value(v.reshape(P, 1), P // 3), want[P // 3])
    # a view whose data is not 16-byte aligned
    base = torch.randn(P + 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    for off in (1, 3):
        view = base[off:off + P]
        assert view.data_ptr() % 16 != 0
        want = torch.sort(view, stable=True)[0]
        for k in _ranks(P):
            assert torch.equal(lightgaussian.kth_value(view, k), want[k])
    # int32 compared as integers: values above 2^24 that a detour through float would merge, and negative ones
    g = torch.Generator().manual_seed(2 * P)
    iv = ((1 << 24) + torch.randint(0, 64, (P,), generator=g, dtype=torch.int32)).to(DEV)
    mixed = torch.randint(-(1 << 31), (1 << 31) - 1, (P,), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)
    for v in (iv, mixed):
        want = torch.sort(v, stable=True)[0]
        for k in _ranks(P):
            got = lightgaussian.kth_value(v, k)
            assert got.dtype == torch.int32 and torch.equal(got, want[k])
    with pytest.raises(ValueError):
        lightgaussian.kth_value(iv, P)


@pytest.mark.parametrize("P", SELECT_SIZES)
def test_percentile_mask_is_the_reference_expression(P):
    _need_gpu()
    inputs = dict(_float_inputs(P))
    inputs["counts"] = torch.randint(0, 5, (P,), generator=torch.Generator().manual_seed(P), dtype=torch.int32) * (1 << 25)
    for what, v in inputs.items():
        v = v.to(DEV)
        for percent in (0, 0.3, 0.66, 1):
            mask = lightgaussian.percentile_mask(v, percent)
            assert mask.dtype == torch.bool and mask.shape == (P,)
            index = int(percent * (P - 1))
            assert torch.equal(mask, v <= lightgaussian.kth_value(v, index)), (what, percent)
            # gaussian_model.py:778-781 (the reference's sort need not be stable: only the value at the index is read)
            sorted_tensor, _ = torch.sort(v, dim=0)
            value_nth_percentile = sorted_tensor[int(percent * (sorted_tensor.shape[0] - 1))]
            # (.squeeze() drops the column of a [P,1] score; at P = 1 it would drop the row as well)
            assert torch.equal(mask, (v <= value_nth_percentile).squeeze().reshape(-1)), (what, percent)
            if what in ("random", "tie at zero", "counts"):
                assert int(mask.sum()) >= index + 1  # every row tied with the threshold goes
    score = torch.rand(P, 1, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert torch.equal(lightgaussian.percentile_mask(score, 0.5), lightgaussian.percentile_mask(score.reshape(-1), 0.5))


@pytest.mark.parametrize("raw", (False, True), ids=("activated", "raw"))
@pytest.mark.parametrize("v_pow", (0.1, 1.0))
@pytest.mark.parametrize("P", (1, 10, 257, 100_003))
def test_v_imp_score_is_the_formula(P, v_pow, raw):
    """Against prune.py:120-127 evaluated in float64 from the same fp32 scales and scores, rtol 1e-6: five fp32 roundings of at most
    2^-24 each (two products, the division, the pow's input as an fp32 value, the last product), the three before the pow damped by
    v_pow <= 1, plus powf's couple of ulp: below 6e-7."""
    _need_gpu()
    g = torch.Generator().manual_seed(P + int(raw))
    log_s = (np.log(0.05) + 0.5 * torch.randn(P, 3, generator=g)).to(DEV)
    imp = (torch.rand(P, generator=g) * 100).to(DEV)
    imp[::7] = 0
    # (raw: the kernel applies the device expression of fr_activate_forward; the formula starts from those same fp32 scales)
    scaling = activate(log_s, torch.randn(P, 4, generator=g).to(DEV), torch.zeros(P, 1, device=DEV))[0] if raw else torch.exp(log_s)
    got = lightgaussian.calculate_v_imp_score(None, imp, v_pow, scaling=log_s if raw else scaling, raw=raw)
    assert got.dtype == torch.float32 and got.shape == (P,)
    assert torch.equal(lightgaussian.volume_of(scaling), (scaling[:, 0] * scaling[:, 1]) * scaling[:, 2])
    volume = torch.prod(scaling.double(), dim=1)
    index = int(len(volume) * 0.9)
    sorted_volume, _ = torch.sort(volume, descending=True)
    kth_percent_largest = sorted_volume[index]
    want = torch.pow(volume / kth_percent_largest, v_pow) * imp.double()
    err = ((got.double() - want).abs() / want.abs().clamp_min(1e-300)).max().item()
    print(f"P={P} v_pow={v_pow} raw={raw}: max rel err {err:.3g}")
    torch.testing.assert_close(got.double(), want, rtol=1e-6, atol=0)
    # through a model, with the model's own scales
    cloud = syn.GaussianCloud(torch.zeros(P, 3, device=DEV), None, None, log_s, None, None)
    model_scaling = torch.exp(log_s)
    via = lightgaussian.calculate_v_imp_score(cloud, imp, v_pow)
    assert torch.equal(via, lightgaussian.calculate_v_imp_score(None, imp, v_pow, scaling=model_scaling))


# ---- prune_list and the whole prune ------------------------------------------------------------------------------------
class RingCam:
    """Camera `i` of tests/golden/ref_camera_ring.npz (the reference's getWorld2View2 / getProjectionMatrix) at a small image size"""

    def __init__(self, g, i, width=160, height=90):
        self.image_width, self.image_height = width, height
        self.FoVx, self.FoVy = (float(x) for x in g[f"fov{i}"])
        self.world_view_transform = torch.tensor(g[f"wvt{i}"], dtype=torch.float32, device=DEV)
        self.full_proj_transform = torch.tensor(g[f"full{i}"], dtype=torch.float32, device=DEV)
        self.camera_center = torch.tensor(g[f"center{i}"], dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def ring_cameras():
    g = np.load(os.path.join(GOLDEN, "ref_camera_ring.npz"))
    return tuple(RingCam(g, i) for i in (0, 2, 5, 7))


def ring_cloud(P=3000):
    """scene_1k moved to the middle of the camera ring"""
    cloud = syn.scene_1k(P=P, seed=11)
    with torch.no_grad():
        cloud._xyz[:, 2] -= 4.0
        cloud._scaling += 0.7
    return cloud


def test_count_render_and_prune_list():
    _need_gpu()
    cams = ring_cameras()
    cloud = ring_cloud().to(DEV)
    bg = torch.tensor(BG, device=DEV)
    views = [lightgaussian.count_render(c, cloud, Pipe(), bg) for c in cams]
    for c, v in zip(cams, views):
        assert set(v) == {"render", "viewspace_points", "visibility_filter", "radii", "gaussians_count", "important_score"}
        assert v["render"].shape == (3, c.image_height, c.image_width) and v["gaussians_count"].dtype == torch.int32
        assert torch.equal(v["visibility_filter"], v["radii"] > 0) and not v["render"].requires_grad
        assert v["viewspace_points"].shape == cloud.get_xyz.shape and not v["viewspace_points"].any()
        assert not v["gaussians_count"][~v["visibility_filter"]].any() and int(v["gaussians_count"].sum()) > 0
        # the frame of the vanilla rasterizer through the same shim, and of the reference-shaped settings without f_count
        rs = cdgr.GaussianRasterizationSettings(c.image_height, c.image_width, np.tan(c.FoVx * 0.5), np.tan(c.FoVy * 0.5), bg, 1.0,
                                                c.world_view_transform, c.full_proj_transform, 3, c.camera_center, False, False, False)
        s, q, o = cloud.get_activated
        with torch.no_grad():
            out = cdgr.GaussianRasterizer(rs)(means3D=cloud.get_xyz, means2D=None, opacities=o, shs=cloud.get_features_split, scales=s, rotations=q)
        assert len(out) == 2 and torch.equal(out[0], v["render"]) and torch.equal(out[1], v["radii"])
        assert torch.equal(v["important_score"], _product_score(v["gaussians_count"], o))
    # a model that offers only the reference's attributes and getters hands over its raw parameters: the score uses the kernel's sigmoid
    ref_model = syn.ReferenceShapedModel(cloud)
    rv = lightgaussian.count_render(cams[0], ref_model, Pipe(), bg)
    assert torch.equal(rv["important_score"], _product_score(rv["gaussians_count"], cloud.get_activated[2]))
    assert rv["gaussians_count"].shape == views[0]["gaussians_count"].shape and int(rv["gaussians_count"].sum()) > 0
    # prune_list: torch's += over the views in pop() order (the last camera first)
    want_c, want_s = views[-1]["gaussians_count"].clone(), views[-1]["important_score"].clone()
    for v in reversed(views[:-1]):
        want_c += v["gaussians_count"]
        want_s += v["important_score"]

    class Scene:
        def getTrainCameras(self):
            return list(cams)
    for arg in (list(cams), Scene()):
        got_c, got_s = lightgaussian.prune_list(cloud, arg, Pipe(), bg)
        assert got_c.dtype == torch.int32 and torch.equal(got_c, want_c) and torch.equal(got_s, want_s)
    assert len(cams) == 4  # (prune_list took a copy)


def _model_with_adam_state():
    torch.manual_seed(0)
    model = prune_ref.Model(ring_cloud(), optim.Adam, device=DEV)
    for seed in (5, 6):
        g = torch.Generator().manual_seed(seed)
        for n in NAMES:
            p = getattr(model, ATTRS[n])
            p.grad = (1e-3 * torch.randn(p.shape, generator=g)).to(DEV)
        model.optimizer.step()
        model.optimizer.zero_grad(set_to_none=True)
    return model


def _reference_mask(model, gaussian_list, imp_list, percent, prune_type, v_pow):
    """prune_finetune.py:219-242 with gaussian_model.py:778-781, in torch's own operations"""
    if prune_type == "important_score":
        score = imp_list
    elif prune_type == "v_important_score":
        score = lightgaussian.calculate_v_imp_score(model, imp_list, v_pow)  # (checked against the formula above)
    elif prune_type == "max_v_important_score":
        score = imp_list * torch.max(model.get_scaling, dim=1)[0]
    elif prune_type == "count":
        score = gaussian_list
    else:
        score = model.get_opacity.detach()
    sorted_tensor, _ = torch.sort(score, dim=0)
    value_nth_percentile = sorted_tensor[int(percent * (sorted_tensor.shape[0] - 1))]
    return (score <= value_nth_percentile).squeeze()


@pytest.mark.parametrize("prune_type", lightgaussian.PRUNE_TYPES)
def test_global_significance_prune_is_boolean_indexing(prune_type):
    _need_gpu()
    cams, bg, percent = list(ring_cameras()), torch.tensor(BG, device=DEV), 0.66
    model = _model_with_adam_state()
    ref = prune_ref.clone_model(model)
    P = len(model)
    with torch.no_grad():
        gaussian_list, imp_list = lightgaussian.prune_list(ref, cams, Pipe(), bg)
        want = _reference_mask(ref, gaussian_list, imp_list, percent, prune_type, 0.1)
    before = {k: v.clone() for k, v in prune_ref.state_tensors(model).items()}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            mask = lightgaussian.global_significance_prune(model, cams, Pipe(), bg, percent, prune_type=prune_type, v_pow=0.1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchroniz" in str(w.message)]
    assert len(syncs) == 1, [str(w.message) for w in syncs]  # the compaction plan's count readback, nothing else
    assert mask.dtype == torch.bool and torch.equal(mask, want)
    n_keep = int((~mask).sum())
    assert 0 < n_keep < P and int(mask.sum()) >= int(percent * (P - 1)) + 1 and len(model) == n_keep
    prune_ref.prune_points(ref, mask)
    prune_ref.assert_same_state(model, ref, prune_type)
    after = prune_ref.state_tensors(model)
    keep = ~mask
    for k, old in before.items():
        if old.dim() and old.shape[0] == P:
            assert after[k].shape[0] == n_keep and prune_ref.same_bits(after[k], old[keep]), k


def test_unknown_prune_type():
    with pytest.raises(ValueError):
        lightgaussian.global_significance_prune(None, [], Pipe(), None, 0.5, prune_type="two_step")
