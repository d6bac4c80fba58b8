"""GPU parity at BASELINE's full size: the S-6M cloud (6 000 000 Gaussians) at 1920x1080 against the CPU oracle.

The oracle preprocesses, culls and walks ALL 6 M Gaussians (so `radii`, which the OBB / foveal cull resets, is
compared bit for bit over the whole cloud -- this is what proves that the cull pass's conservative frame test and the
clipped walks never drop a Gaussian the reference keeps). On a host with >= 64 cores (the MI355X box has 256) it also
bins / sorts / blends ALL 8160 tiles: instance lists of every tile bit for bit, every pixel, the training variant's
per-Gaussian statistics and a backward pass with a gradient on every pixel. On a small host the oracle only does a
window of tiles (`orc_in.win`): lists / pixels inside it, backward with dL_dpix zero outside it (so that every
per-Gaussian gradient sum only has terms the oracle also sums).

BASELINE configs covered: 2 (non-foveated forward, pcheck_obb), 3 (4-layer foveated, centred + moving gaze, packed
and ordinary model layout), 4 (training step: pcheck_obb_sum forward statistics + backward gradients).
Reference: RF rasterizer_impl.cu:264-383 (filter), RF forward.cu:262-609 (blend), RS forward.cu:298-430, R0 backward.cu.
"""
import math
import os

import numpy as np
import pytest
import torch

from tests.checks import FULL_FRAME_GRAD_BUDGETS, FULL_FRAME_GRAD_GROSS, FULL_FRAME_GRAD_REL_L2, check_against_noise, check_grad, check_image
from tests.helpers import cam_dict, scene_dict, syn
from tests import parity_report
from tests.envelope import differences
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

W, H = 1920, 1080
GX, GY = 120, 68
T = GX * GY
FULL_WIN = (0, 0, GX, GY)
# Whole-frame comparisons need the oracle to bin / sort / blend all 8160 tiles of the S-6M frame (6-17 M instances): a second
# or two per frame on the MI355X box's 256 host cores, minutes on a small host -- there the oracle only does a window of
# tiles (and the per-Gaussian statistics / whole-image backward, which have no windowed form, are skipped).
# FOVRASTER_WHOLE_FRAME=0/1 overrides the core-count rule.
WHOLE = os.environ.get("FOVRASTER_WHOLE_FRAME", "1" if (os.cpu_count() or 1) >= 64 else "0") == "1"


def gaussian_lists(lib, vid, P, D, geom, binb):
    """The per-tile sorted lists as GAUSSIAN indices (the reference's point_list): the library's lists hold positions in its
    index-ordered list of cull survivors."""
    from tests.gpu_helpers import vis_list_of
    vis = vis_list_of(lib, vid, P, geom)
    ptr = lib.fr_binning_point_list(vid, D, binb.data_ptr())
    off = ptr - binb.data_ptr()
    return vis[binb[off:off + 4 * D].view(torch.int32).long()].to(torch.int32)


class S6M:
    """The bench scene, built once per session: CPU cloud (oracle inputs) + device tensors (rasterizer inputs).
    opacity_logit: synthetic.OPACITY_LOGIT_S6M (the headline cloud) or OPACITY_LOGIT_S6MT (S-6M-T: same geometry and
    seeds, opacities drawn so that the blend consumes its lists -- 0.9 of a foveated frame's instances, 0.7 of the training
    frame's, lists walked 20 rounds deep, > 1 M Gaussians with a gradient; bench.py extra.translucent)."""

    def __init__(self, opacity_logit=syn.OPACITY_LOGIT_S6M, name="S-6M"):
        assert torch.cuda.is_available(), "no GPU visible: -m gpu tests must run on the MI355X box"
        from fov3dgs_amd import _native, rasterizer as rz
        self.rz, self.native, self.lib = rz, _native, _native.load()
        self.dev = torch.device("cuda", 0)
        self.name = name
        orc.set_threads(os.cpu_count() or 1)
        self.cloud = syn.scene_bicycle_scale(P=6_000_000, seed=1, opacity_logit=opacity_logit)
        self.fov = syn.foveation_layers(self.cloud, seed=2)
        self.scene_plain = scene_dict(self.cloud, "pcheck_obb")
        self.scene_fov = scene_dict(self.cloud, "fov_pcheck_obb", self.fov)
        # the rasterizer gets the very arrays the oracle gets (activations evaluated once, on the CPU: torch's GPU exp /
        # sigmoid / normalize differ from the CPU's in the last bit for a fifth of the elements, and the covariance's
        # eigenvalues amplify that to hundreds of ulps)
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(self.dev)
        sp, sf = self.scene_plain, self.scene_fov
        self.xyz, self.sc, self.rot = up(sp["means3D"]), up(sp["scales"]), up(sp["rotations"])
        self.opac, self.sh, self.rest = up(sp["opacities"]), up(sp["shs"]), up(sf["shs"])
        self.highest, self.shs_dcs, self.opac4 = up(sf["highest_levels"]), up(sf["shs_dcs"]), up(sf["opacities"])
        self.bg = (0.05, 0.1, 0.15)
        self.packed_fov = self.packed_plain = None
        self.view = 0
        self._set_camera(0)

    def _set_camera(self, view):
        rz = self.rz
        self.view = view
        self.cam = syn.camera_ring(view, 8, W, H)
        self.cam_dev = c = syn.camera_ring(view, 8, W, H).to(self.dev)
        self.rs = rz.GaussianRasterizationSettings(H, W, math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5),
                                                   torch.tensor(self.bg, device=self.dev), 1.0, c.world_view_transform,
                                                   c.full_proj_transform, 3, c.camera_center, False, False)

    def at_view(self, view):
        """The same resident scene seen from ring camera `view` (BASELINE config 5: rank r of the 8-GPU job renders camera r):
        a shallow copy that shares the cloud, the device tensors and the packed model."""
        import copy
        other = copy.copy(self)
        other._set_camera(view)
        other.name = self.name  # budgets are per workload
        return other

    def cam_dict(self, gaze=(0.5, 0.5), window=None):
        cd = cam_dict(self.cam, bg=self.bg, gaze=gaze, alpha=0.05)
        cd["tile_window"] = window
        cd["capacity_hint"] = 20_000_000 if window is None or window == FULL_WIN else 12_000_000
        return cd

    def hip(self, variant, gaze=(0.5, 0.5), packed=False):
        """-> dict of numpy / tensors from one native forward call of `variant` on the resident scene."""
        rz, vid, E = self.rz, self.native.VARIANT_IDS[variant], torch.Tensor([])
        pk = None
        cons = torch.zeros(T, dtype=torch.int32, device=self.dev)
        with torch.no_grad():
            if variant == "fov_pcheck_obb":
                if packed:
                    if self.packed_fov is None:
                        self.packed_fov = rz.pack_model(self.xyz, self.sc, self.rot, self.opac4, shs=self.rest, shs_dcs=self.shs_dcs,
                                                        highest_levels=self.highest)
                    pk = self.packed_fov
                res = rz._forward_native(vid, self.rs, self.xyz, self.rest, E, self.opac4, self.sc, self.rot, E, self.shs_dcs,
                                         self.highest, gaze, 0.05, packed=pk, list_consumed=cons)
            else:
                if packed:
                    if self.packed_plain is None:
                        self.packed_plain = rz.pack_model(self.xyz, self.sc, self.rot, self.opac, shs=self.sh)
                    pk = self.packed_plain
                res = rz._forward_native(vid, self.rs, self.xyz, self.sh, E, self.opac, self.sc, self.rot, E, packed=pk, list_consumed=cons)
            torch.cuda.synchronize()
        D, color, radii, geom, binb, img = res[:6]

        def view(buf, ptr, count, dtype):
            off = ptr - buf.data_ptr()
            return buf[off:off + 4 * count].view(dtype)
        out = dict(num_rendered=D, color=color, radii=radii, buffers=(geom, binb, img), lease=res[-1], res=res, consumed=cons)
        out["ranges"] = view(img, self.lib.fr_image_ranges(vid, W, H, img.data_ptr()), 2 * T, torch.int32).view(T, 2).long()
        out["point_list"] = gaussian_lists(self.lib, vid, self.xyz.shape[0], D, geom, binb)
        if variant == "pcheck_obb_sum":
            out["final_T"] = view(img, self.lib.fr_image_final_T(vid, W, H, img.data_ptr()), W * H, torch.float32).view(H, W)
            out["n_contrib"] = view(img, self.lib.fr_image_n_contrib(vid, W, H, img.data_ptr()), W * H, torch.int32).view(H, W)
            out["gaussians_count"], out["contributions"] = res[6], res[7]
        return out


@pytest.fixture(scope="module")
def s6m():
    return S6M()


@pytest.fixture(scope="module")
def s6mt():
    return S6M(syn.OPACITY_LOGIT_S6MT, "S-6M-T")


def consumed_stats(got):
    """What the blend consumed of the frame's lists (fr_forward_args.list_consumed: per tile, entries fetched, in batches of 64)."""
    cons = got["consumed"].cpu().numpy().astype(np.int64)
    lens = (got["ranges"][:, 1] - got["ranges"][:, 0]).cpu().numpy()
    assert (cons <= lens).all() and ((cons % 64 == 0) | (cons == lens)).all()
    return dict(list_consumed_frac=float(cons.sum() / max(lens.sum(), 1)), deepest_list_position=int(cons.max()),
                rounds_of_256_deepest=int((cons.max() + 255) // 256))


def window_tiles(win):
    x0, y0, x1, y1 = win
    ty, tx = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), indexing="ij")
    return (ty * GX + tx).reshape(-1)


def compare_lists(got, want, win, tag):
    """Instance lists of every tile of the window, bit for bit (order included)."""
    tiles = window_tiles(win)
    g_rng = got["ranges"].cpu().numpy()
    w_rng = want["ranges"].astype(np.int64)
    g_len = g_rng[tiles, 1] - g_rng[tiles, 0]
    w_len = w_rng[tiles, 1] - w_rng[tiles, 0]
    np.testing.assert_array_equal(g_len, w_len, err_msg=tag + ": per-tile instance counts")
    assert int(w_len.sum()) == want["num_rendered"] and int(w_len.sum()) > 100_000, tag
    # gather both sides in (window tile, position) order
    rep = np.repeat(np.arange(len(tiles)), w_len)
    pos = np.arange(int(w_len.sum())) - np.repeat(np.cumsum(w_len) - w_len, w_len)
    gi = torch.as_tensor(g_rng[tiles, 0][rep] + pos, device=got["point_list"].device)
    g_ids = got["point_list"][gi].cpu().numpy().astype(np.uint32)
    w_ids = want["point_list"][w_rng[tiles, 0][rep] + pos]
    np.testing.assert_array_equal(g_ids, w_ids, err_msg=tag + ": sorted instance lists")
    return int(w_len.sum()), int(w_len.max())


def crop(img, win):
    x0, y0, x1, y1 = win
    return img[..., y0 * 16:min(y1 * 16, H), x0 * 16:min(x1 * 16, W)]


CENTRE_WIN = (44, 18, 76, 50)  # 32 x 32 tiles around the image centre (small hosts)


def gaze_window(gaze, rows=9):
    """A full-width strip of `rows` tile rows through the gaze point: it crosses all four eccentricity levels and
    ~200 two-level tiles (a square window around the gaze only holds levels 0 and 1)."""
    cy = int(gaze[1] * GY)
    y0 = min(max(cy - rows // 2, 0), GY - rows)
    return (0, y0, GX, y0 + rows)


def pick(win):
    """-> (window the comparisons cover, window handed to the oracle): the whole frame on a host with the cores for it."""
    return (FULL_WIN, None) if WHOLE else (win, win)


def scope(win):
    return "whole frame" if win == FULL_WIN else f"window {win}"


def against_the_contracted_flavour(s6m, variant, scene, cd, got, want, tag):
    """the same whole frame by the oracle's CONTRACTED flavour (f32_fma: multiply-adds fused where gcc's
    -ffp-contract=fast fuses them, standing in for nvcc's default -fmad=true) -- how far the two readings of the reference's source are
    apart on this frame (radii, instances, order, pixels), and the HIP image against the contracted reading. The HIP lists equal the
    uncontracted oracle's bit for bit (asserted by the caller), so their distance to the contracted lists IS the envelope."""
    if not (WHOLE and orc.has_fma_flavour()):
        return
    fma = orc.forward(variant, scene, cd, fma=True)
    env = differences(want, fma)
    hip = differences(got, fma)
    parity_report.record("fma_envelope", tag + ": oracle f32 vs f32_fma", **env)
    parity_report.record("fma_envelope", tag + ": HIP vs oracle f32_fma", **hip)
    # the contracted reading is the same frame up to a few dozen flips, and the HIP path is no further from it than the uncontracted
    # oracle is (+ its own flip budget against that oracle)
    assert env["radii_differ"] <= 20 and env["instances_in_one_only"] <= 200 and env["values_gt_1e4"] <= 600, env
    assert hip["radii_differ"] == env["radii_differ"] and hip["instances_in_one_only"] == env["instances_in_one_only"], (hip, env)
    assert hip["values_gt_1e4"] <= env["values_gt_1e4"] + 3 * FRAME_COUNT_BUDGETS[s6m.name], (hip, env)
    assert hip["max_abs"] <= 2.5e-2, hip


def test_plain_forward_full_size(s6m):
    """Config 2: pcheck_obb over the whole S-6M cloud -- radii of all 6 M Gaussians, lists + pixels of every tile."""
    _plain_forward(s6m)


def test_plain_forward_full_size_translucent(s6mt):
    """Config 2 on S-6M-T: the same lists (the opacities do not enter the binning), blended 0.7 of the way down instead of 0.1."""
    _plain_forward(s6mt)


def view_tag(s6m):
    return "" if s6m.view == 0 else f" ring view {s6m.view}"


def _plain_forward(s6m, layouts=(False, True), fma=True):
    win, owin = pick(CENTRE_WIN)
    want = orc.forward("pcheck_obb", s6m.scene_plain, s6m.cam_dict(window=owin))
    for packed in layouts:
        got = s6m.hip("pcheck_obb", packed=packed)
        tag = f"pcheck_obb {s6m.name}{view_tag(s6m)} {scope(win)} packed={packed}"
        np.testing.assert_array_equal(got["radii"].cpu().numpy(), want["radii"], err_msg=tag + ": radii over all Gaussians")
        if WHOLE:
            assert got["num_rendered"] == want["num_rendered"], tag
        n, longest = compare_lists(got, want, win, tag)
        check_image(crop(got["color"], win).cpu().numpy(), crop(want["color"], win), name=tag, count=FRAME_COUNT_BUDGETS[s6m.name] if WHOLE else None)
        parity_report.record("lists", tag, gaussians=int(s6m.xyz.shape[0]), visible=int((want["radii"] > 0).sum()),
                             compared_instances=n, longest_compared_list=longest, frame_instances=int(got["num_rendered"]),
                             tiles_compared=int(len(window_tiles(win))), **consumed_stats(got))
        if fma and not packed:
            against_the_contracted_flavour(s6m, "pcheck_obb", s6m.scene_plain, s6m.cam_dict(window=owin), got, want, tag)
    s6m.plain_radii = want["radii"]


BENCH_GAZES = [(0.25 * i, 0.25 * j) for i in range(1, 4) for j in range(1, 4)]  # bench.py GAZES (render_compose_gazes_fps.py:26)
# values of a whole 1080p frame (6.2 M) allowed beyond 1e-4 -- flipped (pixel, Gaussian) pairs at a blend threshold, three channels each:
# S-6M: measured <= 9 over the twelve gazes; S-6M-T blends five to seven times as many pairs per frame, most of them faint (median
# alpha 0.03: far more pairs sit near alpha = 1/255), measured <= 29 (largest 2.2e-3). Budgets = measured worst x 1.25.
# Ring views 2 / 5 / 7 of S-6M (round 6): 4 / 10 / 14 values on the training frame -- the count moves with the view like it moves with the
# gaze; the S-6M budget is the worst of all of them x 1.25.
FRAME_COUNT_BUDGETS = {"S-6M": 18, "S-6M-T": 36}
# training frame: share of the pixels whose final_T lies outside 1e-4 relative although n_contrib agrees (a flipped pair in the middle
# of a list moves T by its alpha >= 1/255 without moving n_contrib): measured 1.4e-6 (S-6M, 3 pixels) / 1.06e-5 (S-6M-T, 22 pixels)
FINAL_T_OUTLIERS = {"S-6M": 1e-5, "S-6M-T": 2e-5}


@pytest.mark.parametrize("gaze_id", ("centre", "lissajous10", "lissajous47") + tuple(f"bench{i}" for i in range(9) if i != 4))
def test_foveated_forward_full_size(s6m, gaze_id):
    """Config 3: fov_pcheck_obb, centred gaze and two gazes of the bench's Lissajous path, ordinary and packed model; and the
    other eight of the bench's nine fixed gazes (bench4 is the centre), ordinary model -- every frame the headline times is
    compared whole (on a host with the cores for it)."""
    _foveated_forward(s6m, gaze_id)


@pytest.mark.parametrize("gaze_id", ("centre", "bench2", "lissajous47"))
def test_foveated_forward_full_size_translucent(s6mt, gaze_id):
    """Config 3 on S-6M-T (RF forward.cu:322-475 run to the end of most lists: two-level tiles whose upper state runs long, single-
    level tiles thousands of entries deep): whole frames at the centre, one off-centre bench gaze and one gaze of the moving path."""
    _foveated_forward(s6mt, gaze_id)
    assert s6mt.last_consumed["list_consumed_frac"] >= 0.5, s6mt.last_consumed


FMA_GAZES = ("centre", "bench2")  # the frames also compared with the contracted oracle flavour


def _foveated_forward(s6m, gaze_id, layouts=None):
    if gaze_id.startswith("bench"):
        if not WHOLE:
            pytest.skip("the eight off-centre bench gazes are whole-frame comparisons (host with >= 64 cores)")
        gaze = BENCH_GAZES[int(gaze_id[5:])]
    else:
        gaze = (0.5, 0.5) if gaze_id == "centre" else syn.lissajous_gaze(int(gaze_id[9:]), 90)
    win, owin = pick(gaze_window(gaze))
    want = orc.forward("fov_pcheck_obb", s6m.scene_fov, s6m.cam_dict(gaze=gaze, window=owin))
    tiles = window_tiles(win)
    assert want["tile_blend"][tiles].sum() > 100 and len(np.unique(want["tile_min"][tiles].astype(int))) == 4, \
        "the window should cross all four levels and hold two-level tiles"
    for packed in (layouts or ((False,) if gaze_id.startswith("bench") else (False, True))):
        got = s6m.hip("fov_pcheck_obb", gaze=gaze, packed=packed)
        tag = f"fov_pcheck_obb {s6m.name}{view_tag(s6m)} {scope(win)} gaze={gaze_id} packed={packed}"
        np.testing.assert_array_equal(got["radii"].cpu().numpy(), want["radii"], err_msg=tag + ": radii over all Gaussians")
        if WHOLE:
            assert got["num_rendered"] == want["num_rendered"], tag
        n, longest = compare_lists(got, want, win, tag)
        check_image(crop(got["color"], win).cpu().numpy(), crop(want["color"], win), name=tag, count=FRAME_COUNT_BUDGETS[s6m.name] if WHOLE else None)
        parity_report.record("lists", tag, visible=int((want["radii"] > 0).sum()), compared_instances=n, longest_compared_list=longest,
                             frame_instances=int(got["num_rendered"]), two_level_tiles_compared=int(want["tile_blend"][tiles].sum()),
                             tiles_compared=int(len(tiles)), **consumed_stats(got))
        s6m.last_consumed = consumed_stats(got)
        if gaze_id in FMA_GAZES and not packed and s6m.view == 0:
            against_the_contracted_flavour(s6m, "fov_pcheck_obb", s6m.scene_fov, s6m.cam_dict(gaze=gaze, window=owin), got, want, tag)


def _native_lists(s6m, vid, res):
    D, color, radii, geom, binb, img = res[:6]
    view = lambda buf, ptr, count, dtype: buf[ptr - buf.data_ptr():ptr - buf.data_ptr() + 4 * count].view(dtype)
    return dict(num_rendered=D, color=color, radii=radii,
                ranges=view(img, s6m.lib.fr_image_ranges(vid, W, H, img.data_ptr()), 2 * T, torch.int32).view(T, 2).long(),
                point_list=gaussian_lists(s6m.lib, vid, s6m.xyz.shape[0], D, geom, binb))


def test_shared_model_baseline_full_size(s6m):
    """SURVEY 8f rank 4 at full size: the SMFR baseline on the S-6M cloud (plain model + the foveated model's highest levels)."""
    gaze = syn.lissajous_gaze(10, 90)
    win, owin = pick(gaze_window(gaze))
    scene = dict(s6m.scene_plain, highest_levels=s6m.scene_fov["highest_levels"])
    want = orc.forward("naive_pcheck_obb", scene, s6m.cam_dict(gaze=gaze, window=owin))
    rz, E = s6m.rz, torch.Tensor([])
    vid = s6m.native.VARIANT_IDS["naive_pcheck_obb"]
    with torch.no_grad():
        res = rz._forward_native(vid, s6m.rs, s6m.xyz, s6m.sh, E, s6m.opac, s6m.sc, s6m.rot, E, None, s6m.highest, gaze, 0.05)
        torch.cuda.synchronize()
    got = _native_lists(s6m, vid, res)
    tag = f"naive_pcheck_obb (SMFR) S-6M {scope(win)}"
    np.testing.assert_array_equal(got["radii"].cpu().numpy(), want["radii"], err_msg=tag + ": radii over all Gaussians")
    n, longest = compare_lists(got, want, win, tag)
    check_image(crop(got["color"], win).cpu().numpy(), crop(want["color"], win), name=tag)
    parity_report.record("lists", tag, compared_instances=n, longest_compared_list=longest, tiles_compared=int(len(window_tiles(win))))


@pytest.mark.parametrize("level", (1,))
def test_multi_model_baseline_full_size(s6m, level):
    """SURVEY 8f rank 4 at full size: one level of the MMFR baseline (the S-6M cloud standing in for that level's model):
    the level band's tiles binned / blended, every other tile left zero."""
    gaze = (0.5, 0.5)
    win, owin = pick(gaze_window(gaze))
    scene = dict(s6m.scene_plain, highest_levels=np.zeros((s6m.xyz.shape[0], 1), np.float32))
    cd = dict(s6m.cam_dict(gaze=gaze, window=owin), cur_level=float(level))
    want = orc.forward("mmfr_pcheck_obb", scene, cd)
    rz, E = s6m.rz, torch.Tensor([])
    vid = s6m.native.VARIANT_IDS["mmfr_pcheck_obb"]
    with torch.no_grad():
        res = rz._forward_native(vid, s6m.rs, s6m.xyz, s6m.sh, E, s6m.opac, s6m.sc, s6m.rot, E, None, torch.zeros_like(s6m.highest), gaze, 0.05,
                                 cur_level=float(level))
        torch.cuda.synchronize()
    got = _native_lists(s6m, vid, res)
    tag = f"mmfr_pcheck_obb level {level} S-6M {scope(win)}"
    np.testing.assert_array_equal(got["radii"].cpu().numpy(), want["radii"], err_msg=tag + ": radii over all Gaussians")
    n, longest = compare_lists(got, want, win, tag)
    check_image(crop(got["color"], win).cpu().numpy(), crop(want["color"], win), name=tag)
    parity_report.record("lists", tag, compared_instances=n, longest_compared_list=longest, tiles_compared=int(len(window_tiles(win))))


RING_VIEWS = (2, 5, 7)  # of the eight ring cameras (BASELINE config 5: rank r renders camera r); view 0 is every other test's


@pytest.mark.parametrize("view", RING_VIEWS)
def test_plain_forward_ring_views(s6m, view):
    """Config 5's per-rank work, forward: pcheck_obb over the whole S-6M cloud from ring camera `view` -- radii of all 6 M Gaussians,
    lists and pixels of every tile (ordinary layout)."""
    _plain_forward(s6m.at_view(view), layouts=(False,), fma=False)


@pytest.mark.parametrize("view", RING_VIEWS)
def test_foveated_forward_ring_views(s6m, view):
    """The foveated frame from ring camera `view` at one off-centre bench gaze (whole frame on a host with the cores for it)."""
    _foveated_forward(s6m.at_view(view), "bench2" if WHOLE else "centre", layouts=(False,))


@pytest.mark.parametrize("view", RING_VIEWS)
def test_training_step_ring_views(s6m, view):
    """Config 5's per-rank work, training: pcheck_obb_sum forward statistics + backward gradients from ring camera `view`, same
    checks and budgets as view 0 (tests/checks.py FULL_FRAME_GRAD_BUDGETS)."""
    _training_step(s6m.at_view(view), min_rows=60_000)


BWD_WIN = (30, 20, 90, 48)  # 60 x 28 tiles (small hosts)


def compare_statistics(got, want, tag, exact_contrib=False):
    """gaussians_count / contributions over all P Gaussians (whole-frame oracle only: they are sums over every tile)."""
    gc, wc = got["gaussians_count"].cpu().numpy(), want["gaussians_count"]
    differ = float(np.mean(gc != wc))
    parity_report.record("count", tag + " gaussians_count", frac_differ=differ, n=int(gc.size), total=int(wc.sum()),
                         max_abs_diff=int(np.abs(gc.astype(np.int64) - wc).max()))
    return differ


def test_training_step_full_size(s6m):
    """Config 4: pcheck_obb_sum forward statistics and the backward pass on the S-6M cloud. On a host with the cores for
    the whole-frame oracle: lists / pixels / final_T / n_contrib of all 8160 tiles, gaussians_count and contributions
    of all 6 M Gaussians (the round-claiming scheme of k_render on 40-round lists, RS forward.cu:349-361,400), and the
    backward pass with dL_dpix non-zero everywhere (all 1.9 M visible Gaussians)."""
    _training_step(s6m, min_rows=100_000)


def test_training_step_full_size_translucent(s6mt):
    """Config 4 on S-6M-T: the blend walks 0.7 of the frame's 16.9 M instances (lists consumed 20 rounds of 256 deep: the
    round-claiming counts of RS forward.cu:349-361 far beyond the first rounds), the backward pass recovers T by division down
    thousands of entries (R0 backward.cu:503-507) and > 1 M Gaussians receive a gradient (S-6M: 131 k)."""
    _training_step(s6mt, min_rows=1_000_000)
    if WHOLE:
        assert s6mt.last_consumed["list_consumed_frac"] >= 0.5 and s6mt.last_consumed["rounds_of_256_deepest"] >= 20, s6mt.last_consumed


def budget_kw(s6m, tensor):
    """check_grad's outlier budget of a whole-frame tensor (tests/checks.py FULL_FRAME_GRAD_BUDGETS); the default budget on a window."""
    b = FULL_FRAME_GRAD_BUDGETS.get(s6m.name + (" ring" if s6m.view else ""), {}).get(tensor) if WHOLE else None
    if os.environ.get("FOVRASTER_MEASURE_BUDGETS") == "1":
        return dict(outlier_frac=1.0, gross_frac=1.0, rel_l2=1.0, cosine=1.0)  # calibration run: record, do not judge
    return {} if b is None else dict(outlier_frac=b, rel_l2=FULL_FRAME_GRAD_REL_L2, gross_frac=FULL_FRAME_GRAD_GROSS)


def _training_step(s6m, min_rows):
    from fov3dgs_amd.rasterizer import _backward_native
    win, owin = pick(BWD_WIN)
    want = orc.forward("pcheck_obb_sum", s6m.scene_plain, s6m.cam_dict(window=owin))
    got = s6m.hip("pcheck_obb_sum")
    tag = f"pcheck_obb_sum {s6m.name}{view_tag(s6m)} {scope(win)}"
    s6m.last_consumed = consumed_stats(got)
    np.testing.assert_array_equal(got["radii"].cpu().numpy(), want["radii"], err_msg=tag + ": radii")
    n, longest = compare_lists(got, want, win, tag)
    check_image(crop(got["color"], win).cpu().numpy(), crop(want["color"], win), name=tag, count=FRAME_COUNT_BUDGETS[s6m.name] if WHOLE else None)
    g_nc, w_nc = crop(got["n_contrib"], win).cpu().numpy().astype(np.uint32), crop(want["n_contrib"], win)
    same = g_nc == w_nc
    parity_report.record("count", tag + " n_contrib", frac_differ=float(np.mean(~same)), n=int(same.size))
    assert np.mean(~same) <= 1e-5
    gT, wT = crop(got["final_T"], win).cpu().numpy()[same], crop(want["final_T"], win)[same]
    offT = np.abs(gT - wT) > 1e-4 * np.abs(wT) + 1e-7  # a flipped pair in the middle of a list moves T by <= alpha without moving n_contrib
    parity_report.record("count", tag + " final_T outside 1e-4 relative", frac=float(offT.mean()), max_rel=float((np.abs(gT - wT) / np.maximum(np.abs(wT), 1e-12)).max()))
    assert offT.mean() <= FINAL_T_OUTLIERS[s6m.name] and np.abs(gT - wT).max() <= 1.5e-2
    if WHOLE:
        # RS statistics: +1 per entry of every 256-entry round a tile starts -- integer, expected bit-exact; a tile whose
        # last live pixel saturates within an ulp of T = 1e-4 at a round boundary may start one round more or less
        differ = compare_statistics(got, want, tag)
        assert differ <= 1e-5, f"gaussians_count differs on {differ:.2e} of the Gaussians"
        check_grad(got["contributions"].cpu().numpy(), want["contributions"], tag + " contributions",
                   **budget_kw(s6m, "contributions"))
        parity_report.record("lists", tag, compared_instances=n, longest_compared_list=longest, rounds_of_longest_list=int((longest + 255) // 256),
                             tiles_compared=int(len(window_tiles(win))), **s6m.last_consumed)
        if s6m.view == 0:
            against_the_contracted_flavour(s6m, "pcheck_obb_sum", s6m.scene_plain, s6m.cam_dict(window=owin), got, want, tag)
    # backward: random dL_dpix (inside the window only when the oracle only has the window's lists)
    x0, y0, x1, y1 = win
    dpix = np.zeros((3, H, W), np.float32)
    ys, xs = slice(y0 * 16, min(y1 * 16, H)), slice(x0 * 16, min(x1 * 16, W))
    dpix[:, ys, xs] = np.random.default_rng(3).normal(size=dpix[:, ys, xs].shape)
    # The gradients are compared where the two FORWARD passes agree. A (pixel, Gaussian) pair that flips at a blend threshold
    # (v_exp_f32 against expf, a few pixels per frame: the image / final_T checks above count them) changes that pixel's
    # transmittance by >= 1/255 for EVERY entry behind it -- hundreds to thousands of Gaussians, each of which then differs by 0.4 %
    # of that pixel's share of its gradient. On S-6M-T's deep lists the two dozen flipped pixels put 1.4e-3 of the 1 M rows outside
    # 1e-4 relative, three times what the arithmetic itself does: a property of the forward pass, already measured there. So the
    # loss gradient is zero on the pixels whose n_contrib or final_T differ (both sides get the same dL_dpix).
    fT_g, fT_w = crop(got["final_T"], win).cpu().numpy(), crop(want["final_T"], win)
    agree = same & ~(np.abs(fT_g - fT_w) > 1e-5 * np.abs(fT_w) + 1e-9)
    parity_report.record("count", tag + " pixels left out of the backward comparison (forward state differs)", n=int((~agree).sum()), frac=float((~agree).mean()))
    assert (~agree).mean() <= 2.0 * FINAL_T_OUTLIERS[s6m.name]
    dpix[:, ys, xs] *= agree[None].astype(np.float32)
    wg = orc.backward("pcheck_obb_sum", s6m.scene_plain, s6m.cam_dict(window=owin), want, dpix)
    wg64 = None
    if WHOLE:
        # the same arithmetic in DOUBLE on the fp32 forward's state (lists, n_contrib, final_T: no discrete decision differs): what the
        # reference's own fp32 arithmetic loses on this frame -- the yardstick for the rows outside 1e-4 (check_against_noise)
        want64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in want.items()}
        wg64 = orc.backward("pcheck_obb_sum", {k: v.astype(np.float64) for k, v in s6m.scene_plain.items()}, s6m.cam_dict(window=owin), want64,
                            dpix.astype(np.float64), dtype=np.float64)
        del want64
    geom, binb, img = got["buffers"]
    E = torch.Tensor([])

    def run_backward():
        res = _backward_native(s6m.native.VARIANT_IDS["pcheck_obb_sum"], s6m.rs, s6m.xyz, got["radii"], E, s6m.opac, s6m.sc, s6m.rot, E,
                               torch.as_tensor(dpix, device=s6m.dev), s6m.sh, geom, got["num_rendered"], binb, img, want_cov3D_grad=True, want_color_grad=True)
        torch.cuda.synchronize()
        return res
    res = run_backward()
    names = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot")
    touched = None
    for k, v in zip(names, res):
        g = v.cpu().numpy().reshape(wg[k].shape)
        # rows the window reaches: compare those (the rest must be exactly zero on both sides)
        rows = np.abs(wg[k]).reshape(len(g), -1).max(axis=1) > 0
        grows = np.abs(g).reshape(len(g), -1).max(axis=1) > 0
        if k == "dL_dopacity":
            touched = rows
        assert not (grows & ~rows).any() or np.abs(g[grows & ~rows]).max() < 1e-6, k + ": gradient on a Gaussian the window cannot reach"
        check_grad(g[rows], wg[k][rows], f"{tag} {k}", **budget_kw(s6m, k))
        if wg64 is not None:
            check_against_noise(g[rows], wg[k][rows], wg64[k][rows], f"{tag} {k}")
    assert touched.sum() > (min_rows if WHOLE else min_rows // 10)  # (S-6M is dense: of 1.9 M visible Gaussians 131 k reach a pixel before it saturates)
    parity_report.record("count", tag + " Gaussians with a gradient", n=int(touched.sum()))
    # the check is sensitive where round 2's was not: a 1 % error in the degree-3 SH gradients (coefficients 9..15) fails it
    sh_g = res[5].cpu().numpy().reshape(wg["dL_dsh"].shape)
    rows = np.abs(wg["dL_dsh"]).reshape(len(sh_g), -1).max(axis=1) > 0
    spoiled = sh_g[rows].copy()
    spoiled[:, 9:, :] *= 1.01
    from tests.checks import grad_stats
    st = grad_stats(spoiled, wg["dL_dsh"][rows])
    parity_report.record("sensitivity", tag + " dL_dsh with 1 % injected into coefficients 9..15", **st)
    assert st["frac_bad"] > 0.9, "the gradient check must catch a 1 % error in SH coefficients 9..15"
    # fr_backward is idempotent: a second call over the same forward state gives the same gradients (the reference
    # allocates fresh zeros per call; here the per-Gaussian sums are cleared by the call that reads them)
    res2 = run_backward()
    for k, a, b in zip(names, res, res2):
        st = grad_stats(b.cpu().numpy().reshape(len(wg[k]), -1), a.cpu().numpy().reshape(len(wg[k]), -1))
        parity_report.record("grad", f"{tag} second backward vs first {k}", **st)
        # (the same kernel twice: only the order of the float atomics differs -- on this frame that alone puts 1e-4 of the
        # dL_dopacity rows, the ones whose terms cancel, outside 1e-4 relative)
        assert st["frac_bad"] <= 1e-3 and st["rel_l2"] < 1e-5, f"second backward call differs in {k}: {st}"


@pytest.mark.parametrize("variant", ("pcheck_obb_max", "pcheck_obb_loss_weighted_max_count"))
def test_pruning_metric_variants_full_size(s6m, variant):
    """SURVEY 8f rank 1 at full size: the two pruning-metric flavours' statistics over the whole frame (prune.py /
    metric_mask_learn.py run them over whole training views)."""
    if not WHOLE:
        pytest.skip("per-Gaussian statistics need the whole-frame oracle (>= 64 host cores)")
    scene = dict(s6m.scene_plain)
    if variant == "pcheck_obb_loss_weighted_max_count":
        scene["loss_map"] = np.random.default_rng(11).random((3, H, W)).astype(np.float32)
    want = orc.forward(variant, scene, s6m.cam_dict(window=None))
    rz, E = s6m.rz, torch.Tensor([])
    vid = s6m.native.VARIANT_IDS[variant]
    with torch.no_grad():
        res = rz._forward_native(vid, s6m.rs, s6m.xyz, s6m.sh, E, s6m.opac, s6m.sc, s6m.rot, E,
                                 loss_map=None if "loss_map" not in scene else torch.as_tensor(scene["loss_map"]).to(s6m.dev))
        torch.cuda.synchronize()
    got = _native_lists(s6m, vid, res)
    got["gaussians_count"], got["contributions"] = res[6], res[7]
    tag = f"{variant} S-6M whole frame"
    assert got["num_rendered"] == want["num_rendered"], tag
    compare_lists(got, want, FULL_WIN, tag)
    check_image(got["color"].cpu().numpy(), want["color"], name=tag)
    differ = compare_statistics(got, want, tag)
    gcb, wcb = got["contributions"].cpu().numpy(), want["contributions"]
    if variant == "pcheck_obb_max":
        # count = live in-support pixels per entry (a pixel that saturates an ulp apart moves a count by one)
        assert differ <= 2e-3, differ
        check_grad(gcb, wcb, tag + " contributions (max alpha T)", rtol=1e-5)
    else:
        assert differ <= 1e-5, differ
        # every pixel's loss goes to ONE Gaussian; two best contributions within an ulp may credit the other one
        np.testing.assert_allclose(gcb.sum(dtype=np.float64), wcb.sum(dtype=np.float64), rtol=1e-5)
        moved = float(np.mean(np.abs(gcb - wcb) > 1e-3))
        parity_report.record("count", tag + " contributions moved to another Gaussian", frac=moved)
        assert moved <= 1e-4, moved


def test_raw_parameters_full_size():
    """fr_forward_args.raw_activations on the S-6M cloud at 1080p: the training variant fed with the model's raw parameters
    gives the image, radii and statistics of the activate-then-render path bit for bit, and the same gradients (w.r.t. the
    raw parameters) up to the order of the float atomics."""
    from fov3dgs_amd.activations import activate
    from fov3dgs_amd.diff_gaussian_rasterization_pcheck_obb_sum import GaussianRasterizationSettings, GaussianRasterizer
    dev = "cuda:0"
    cam = syn.camera_ring(0, 8).to(dev)
    W, H = cam.image_width, cam.image_height
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3, device=dev), 1.0,
                                       cam.world_view_transform, cam.full_proj_transform, 3, cam.camera_center, False, False)
    w = torch.rand(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) - 0.5
    res = []
    for raw in (False, True):
        cloud = syn.scene_bicycle_scale(P=6_000_000, seed=1).to(dev).requires_grad_(True)
        s, q, o = (cloud._scaling, cloud._rotation, cloud._opacity) if raw else activate(cloud._scaling, cloud._rotation, cloud._opacity)
        out = GaussianRasterizer(rs)(means3D=cloud.get_xyz, means2D=torch.zeros_like(cloud.get_xyz, requires_grad=True), opacities=o,
                                     shs=cloud.get_features_split, scales=s, rotations=q, **({"raw_activations": True} if raw else {}))
        (out[0] * w).sum().backward()
        res.append(dict(img=out[0].detach(), radii=out[1], count=out[2], contrib=out[3].detach(),
                        grads={n: getattr(cloud, "_" + n).grad for n in ("xyz", "scaling", "rotation", "opacity", "features_dc", "features_rest")}))
        del cloud, out, s, q, o
    a, b = res
    assert torch.equal(a["img"], b["img"]) and torch.equal(a["radii"], b["radii"]) and torch.equal(a["count"], b["count"])
    assert int((a["radii"] > 0).sum()) > 1_000_000
    tol = float((a["contrib"] - b["contrib"]).abs().max()) / (float(a["contrib"].abs().max()) + 1e-12)
    assert tol < 1e-5, tol  # sums of float atomics
    for n in a["grads"]:
        check_grad(b["grads"][n].cpu().numpy(), a["grads"][n].cpu().numpy(), "S-6M raw parameters: " + n)
