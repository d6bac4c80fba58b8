"""The foveated appearance backward pass (k_render_bwd_fov / k_fov_appearance_bwd over the state k_render_fov<..., KEEP> keeps) judged
on thousands of rows, on every level state, on lists thousands of entries deep, on short lists and on tiny frames: the GPU half of
tests/fov_backward_scenes.py (the scenes, their census and the comparison; tests/test_fov_backward_scenes_cpu.py asserts the census
conditions and proves that the comparison rejects a defect in every branch).

Per scene: `ranges` and `point_list` equal the forward's (the C oracle's; the numpy derivation's under the two settings) bit for bit;
the image passes check_image; the loss gradient is zero on the pixels whose KEPT state differs from the reference's -- n_contrib
unequal, or final_T off by more than 1e-5 |T| + 1e-9, in plane 0 and, inside two-level tiles, in plane 1 -- at most 1e-3 of the frame
(MAX_FLIPPED, the cap tests/test_backward_branches_gpu.py holds the same cloud to at the same opacity factor; the reference alone
leaves out none), and the reference's gradients are computed for that loss gradient ON THE LIBRARY'S LEVEL MAP (_both_passes); then the three
gradient tensors are held to the reference arithmetic's own noise, as whole tensors and on the live rows of every branch the scene
claims (fov_backward_scenes.judge), dL_dshs_dcs is exactly zero on clamped channels and rows the reference leaves at zero are exact
zeros. Every comparison's measured shares and every flipped-pixel share go to the parity report. Every gradient tensor starts as NaN
(tests/conftest.py)."""
import numpy as np
import pytest
import torch

from tests import fov_backward_scenes as fs
from tests import test_fov_backward_gpu as fb
from tests import parity_report
from tests.checks import _where, check_image

pytestmark = pytest.mark.gpu

MAX_FLIPPED = 1e-3  # share of the frame's pixels left out of the loss because their kept state differs between the two passes
FACTORS = fs.FACTORS  # per-tensor exceptions to the factor 1.5, with their measurements (tests/fov_backward_scenes.py)


def _both_passes(name, allow_empty=False):
    """The state-keeping forward and the backward pass of the library on the named scene, and the reference's float32 / float64
    gradients and census for the same loss gradient (zero on the pixels whose kept state differs).
    -> (got, g32, g64, census, reference dict, forward dict)"""
    r = fs.reference(name)
    fwd = fb.keep_forward(r["scene"], r["cam"], r["settings"], allow_empty=allow_empty)
    # the lists, before anything else is judged
    assert fwd["num_rendered"] == r["fwd"]["num_rendered"]
    np.testing.assert_array_equal(fwd["ranges"], r["fwd"]["ranges"])
    np.testing.assert_array_equal(fwd["point_list"], r["fwd"]["point_list"])
    check_image(fwd["color"].cpu().numpy(), r["fwd"]["color"], name=f"{name} image")
    # ONE forward state for both passes: the reference is rebuilt on the LIBRARY's level map. k_tile_levels evaluates acosf / tanf on
    # the device, so its tile_min and gradients differ from the oracle's in the last bits (held to 2e-5 here as in
    # tests/test_gpu_parity.py), and the blend weight w1 ~ 3 (1 - x)^2 turns a difference of 1e-6 in est into 2 d x / (1 - x) = 7e-5
    # RELATIVE in a share of 1e-2: on faint-main eleven rows that meet the lower state at one pixel of one tile carried exactly that,
    # and it is a property of the forward state, not of the backward pass (as the pixels whose kept state differs, below).
    lib_map = {k: fwd[k] for k in ("tile_min", "tile_gx", "tile_gy")}
    np.testing.assert_array_equal(fwd["tile_blend"], np.asarray(r["fwd"]["tile_blend"]).astype(np.uint8))
    worst = max(float(np.nanmax(np.abs(lib_map[k] - r["fwd"][k]), initial=0.0)) for k in lib_map)
    parity_report.record("level_map", f"{_where()} {name}", max_abs_difference=worst)
    print(f"{name}: the library's level map differs from the forward's by at most {worst:.2e}")
    for k in lib_map:
        np.testing.assert_allclose(lib_map[k], r["fwd"][k], rtol=0, atol=2e-5, equal_nan=True)
    ref = fs.make_ref(dict(r["fwd"], **lib_map), r["scene"], r["cam"], r["settings"])
    fT, nc, single = ref.state_planes()
    agree = np.ones_like(single)
    for plane, mask in ((0, np.ones_like(single)), (1, ~single)):
        same = (fwd["n_contrib"][plane] == nc[plane]) & ~(np.abs(fwd["final_T"][plane] - fT[plane]) > 1e-5 * np.abs(fT[plane]) + 1e-9)
        print(f"{name}: plane {plane} differs on {int((~same & mask).sum())} of {int(mask.sum())} pixels")
        agree &= same | ~mask
    left_out = fs.record_flipped_pixels(name, agree)
    print(f"{name}: {int((~agree).sum())} of {agree.size} pixels left out of the loss")
    assert left_out <= MAX_FLIPPED
    dpix = r["dpix"] * agree[None].astype(np.float32)
    g32, g64 = fs.gradients(ref, dpix)
    cen = fs.census(ref, r["fwd"], r["scene"], g64)
    r = dict(r, ref=ref)
    got = fb.backward(fwd, dpix)
    return got, g32, g64, cen, r, fwd


def _branches(name):
    if name in fs.LARGE:
        return fs.LARGE[name]
    return fs.LEVELS[:int(name[-1])] + fs.STATES + ("upper_skips", "clamped")


@pytest.mark.parametrize("name", tuple(fs.LARGE) + fs.SETTINGS)
def test_every_level_and_state_on_its_own_rows(name):
    """faint / faint-main (thousands of live rows at every level, in single-level tiles and in both states of two-level tiles), deep
    (n_contrib to 4612 in plane 0, beyond 1000 in plane 1: T recovered by division thousands of times in a row), piled (lists of 8953
    in the 8192..16383 sort class, walked 139 batches deep) and the two-/three-level settings: all three tensors, whole and on the
    live rows of every level, of the single / lower / upper state, of Gaussians an upper state skipped by the existence test and of
    rows with a clamped channel, on their own. Factor over the reference's own share: 1.5 (fov_backward_scenes.FACTORS holds no
    exception; DESIGN.md has the run-to-run spread of the counts).
    What these scenes found, all about the blend weight w1 = 1 - smoothstep(x) ~ 3 (1 - x)^2 of two-level tiles, which is
    ill-conditioned where x is near 1: (1) against a reference on the ORACLE's level map, faint-main had 15 .. 19 of 1305 dL_dopacities
    rows beyond 5e-5 (16 allowed), eleven of them 7.3e-5 off through ONE pixel of one tile: the device's level map differs from the
    oracle's by up to 2e-6 (acosf / tanf), i.e. the forward states differed -- the reference is now rebuilt on the library's map
    (_both_passes) and the same rows are 1 outside 1e-4 and 3 beyond 5e-5 in each of eight runs; (2) tests/fov_backward_ref.py froze the
    float32 w1 of its own forward pass into its float64 gradients: the float64 flavour now forms w1 in double; (3) k_render_bwd_fov
    formed w1 by the forward's cancelling expression 1 - (3 x^2 - 2 x^3): it now uses the factored polynomials (csrc/backward.hip; 18
    against 15 rows beyond 5e-5 on faint-main, measured before (1)). Over eight runs every comparison stayed at or below 0.72 of its
    limit."""
    fb._need_gpu()
    got, g32, g64, cen, r, _ = _both_passes(name)
    fs.record_census(name, cen, r["depth"])
    branches = _branches(name)
    for br in branches:
        assert int(cen[br].sum()) >= fs.MIN_BRANCH, br
    assert got["dL_dopacities"].shape == (r["ref"].P, r["L"])
    fs.judge(got, g32, g64, cen, name, r["L"], branches=branches, factors=FACTORS.get(name))


@pytest.mark.parametrize("name", fs.SHORT_NAMES)
def test_short_lists_take_every_tail_of_the_level_routed_fold(name):
    """Lists of 1, 2, 3 and 5 entries in single-level tiles and in both states of two-level tiles, every level live: the fold ends
    with one entry pending or none, after zero, one or two full folds, and the pending entry goes through the level routing. Judged
    against the DOUBLE-precision reference, EVERY row within 1e-4 relative -- no outlier share (the reference's own fp32 arithmetic is
    within 5.1e-6 on every row of these scenes; flipped pixels are out of the loss): a fold that dropped or doubled an entry, or
    routed it to another level's components, is off by the entry."""
    fb._need_gpu()
    got, g32, g64, cen, r, _ = _both_passes(name)
    P = int(name.split("-")[1])
    whole, two_level = fs.whole_tiles(r["ref"], P)
    assert whole >= 4 and two_level >= 1 and all(cen[lv].any() for lv in fs.LEVELS)
    fs.judge_short(got, g32, g64, cen, name, 4, min_rows=int(cen["live"].sum()))


@pytest.mark.parametrize("name", tuple(fs.TINY))
def test_tiny_frames(name):
    """16 x 16 (one whole single-level tile), 17 x 15 (two tiles: one whose tile_min is -1.95 -- level 0 -- and a two-level one),
    8 x 8 (a frame smaller than its only tile, which is two-level) and 15 x 1 (a frame one pixel high): lists, image and judge() with
    min_rows from the census.
    17 x 15 is where a defect sat (seen while sizing this scene, as heap corruption in the CPU oracle): its first tile has
    tile_min = -1.95, and k_render_fov took its level row at int(tile_min) = -1, i.e. the PREVIOUS Gaussian's level-3 row (16 bytes in
    front of the level rows for Gaussian 0), while k_bin had evaluated the level-0 rows of that tile's Gaussians, and k_render_bwd_fov
    returned early for such a tile (no gradient at all). The reference indexes the same way (undefined behaviour: outside its arrays
    for Gaussian 0); the CPU oracle, following it, wrote 12 bytes in front of fov_colors (tests/test_oracle_sanitized_cpu.py). Now the
    kernels, the oracle and the numpy derivation take level 0 for a negative tile_min, as k_bin always did (csrc/render.hip,
    csrc/backward.hip, oracle/fovraster_oracle.c); such a tile never blends, so the index is the level's only use."""
    fb._need_gpu()
    got, g32, g64, cen, r, _ = _both_passes(name)
    fs.record_census(name, cen, r["depth"])
    # every level and state that has a live row is judged on its own rows too (17 x 15: 14 lower and 10 upper rows); min_rows: the
    # census of the loss gradient that was used (the CPU census when no pixel was left out: none was on an MI355X)
    branches = tuple(b for b in fs.LEVELS + fs.STATES if cen[b].any())
    assert branches and set(branches) == {b for b in fs.LEVELS + fs.STATES if r["census"][b].any()}
    fs.judge(got, g32, g64, cen, name, 4, branches=branches, min_rows=int(cen["live"].sum()), factors=FACTORS.get(name))


@pytest.mark.parametrize("name", fs.NOTHING)
def test_a_frame_that_renders_nothing_gives_exact_zeros(name):
    """300 Gaussians behind the camera, and the faint cloud at 3 x 40 where every tile's level is NaN (no Gaussian passes the level
    filter): num_rendered == 0, the image is the oracle's (background), and all three gradient tensors -- NaN before the call -- are
    exact zeros."""
    fb._need_gpu()
    r = fs.reference(name)
    fwd = fb.keep_forward(r["scene"], r["cam"], allow_empty=True)
    assert fwd["num_rendered"] == 0 == r["fwd"]["num_rendered"] and not (fwd["radii"] > 0).any()
    check_image(fwd["color"].cpu().numpy(), r["fwd"]["color"], name=f"{name} image")
    got = fb.backward(fwd, r["dpix"])
    P = r["ref"].P
    for k, shape in (("dL_dopacities", (P, 4)), ("dL_dshs_dcs", (P, 4, 3)), ("dL_dlevel_colours", (P, 4, 3))):
        assert got[k].shape == shape and np.isfinite(got[k]).all() and not got[k].any(), k
