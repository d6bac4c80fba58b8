"""Named, seeded scenes for the FOVEATED appearance backward pass (k_render_bwd_fov / fr_backward_fov_appearance), each with a CENSUS
of which (Gaussian, level) rows reach which branch, and the comparison the CPU half (tests/test_fov_backward_scenes_cpu.py) and the
GPU half (tests/test_fov_backward_scenes_gpu.py) both judge with: the counterpart of tests/backward_scenes.py.

Why: every scene of tests/fov_backward_ref.py is helpers.small_case("fov_pcheck_obb") -- 3000 Gaussians with +1.0 on every raw
opacity, where a pixel finishes a few splats deep: 890 of 12 000 (Gaussian, level) rows carry a gradient (53 at level 0), the deepest
n_contrib is 521, and check_grad's fixed budget of 3e-3 is judged on them. Here:

  faint         the same cloud, opacities x 0.1, gaze (0.4, 0.55), alpha 0.6      -> thousands of live rows, every list consumed
  faint-main    the same at fov_backward_ref.MAIN's gaze (0.2, 0.35)
  deep          small_cloud(20000, 5), opacities x 0.1, gaze (0.3, 0.45)          -> n_contrib beyond 4000: T recovered by division
                                                                                    thousands of times in a row, in both state planes
  piled         scene_1k(9000, 9) drawn together (xy x 0.05), raw opacity - 3.5,   -> lists in the 8192..16383 sort class, walked
                64 x 64, gaze (0.3, 0.6), alpha 2.0                                   ~139 batches deep
  short-1/2/3/5 P large splats of scene_1k, every highest level 3, 200 x 120,      -> the short-list tails of the fold (one entry
                gaze (0.1, 0.9), alpha 0.3                                            pending or none) through the level routing
  tiny-16x16 / -17x15 / -8x8 / -15x1   the faint cloud under small_camera(W, H)     -> one whole tile; two tiles, one two-level, one
                                                                                    with tile_min <= -1; a frame smaller than its
                                                                                    only (two-level) tile; a frame one pixel high
  nothing       300 Gaussians behind the camera                                     -> num_rendered == 0
  nothing-3x40  the faint cloud at 3 x 40: every tile level is NaN                  -> num_rendered == 0 through the level filter
  faint-L2 / faint-L3   test_fov_backward_gpu.SETTINGS' two FoveationSettings, opacities x 0.1 (forward: the numpy derivation)

A row is one (Gaussian, level) pair; a LIVE row has dL_dopacities != 0 in the float64 reference. The census conditions are asserted
by the CPU half: conditions, not measurements. A plain module: not a conftest, nothing here is collected."""
import copy
import functools

import numpy as np

from oracle import oracle as orc
from tests import backward_scenes as bs
from tests import fov_backward_ref as R
from tests import parity_report
from tests.checks import GRAD_COSINE, GRAD_OUTLIERS, GRAD_REL_L2, _where, check_against_noise, check_grad, grad_stats
from tests.helpers import cam_dict, scene_dict, small_camera, small_cloud, syn

TENSORS = ("dL_dopacities", "dL_dlevel_colours", "dL_dshs_dcs")
MIN_LIVE, MIN_BRANCH = bs.MIN_LIVE, bs.MIN_BRANCH
FACTOR, FLOOR, ABS_ROWS, TAIL_FLOOR, OPACITY_FACTOR = bs.FACTOR, bs.FLOOR, bs.ABS_ROWS, bs.TAIL_FLOOR, bs.OPACITY_FACTOR
SHORT = bs.SHORT
SHORT_RTOL = 1e-4          # short scenes: EVERY row within this of the float64 reference (the reference's fp32 arithmetic: <= 5.1e-6)
SHORT_REF_NOISE = 1e-5     # ... whose own fp32 arithmetic must stay ten times inside that bound on every row (a condition of the CPU half)
VARIANT = "fov_pcheck_obb"
LEVELS = ("level0", "level1", "level2", "level3")
STATES = ("single", "lower", "upper")

# name -> what the scene CLAIMS: the branches (census masks) judged on their own rows, each with >= MIN_BRANCH live rows.
LARGE = {
    "faint": LEVELS + STATES + ("upper_skips", "clamped"),
    "faint-main": LEVELS + STATES + ("upper_skips", "clamped"),
    "deep": LEVELS + STATES + ("upper_skips", "clamped"),
    "piled": ("level0", "level2", "single"),   # (its three two-level tiles hold one entry between them)
}
TINY = {"tiny-16x16": (16, 16), "tiny-17x15": (17, 15), "tiny-8x8": (8, 8), "tiny-15x1": (15, 1)}
NOTHING = ("nothing", "nothing-3x40")
SETTINGS = ("faint-L2", "faint-L3")
SHORT_NAMES = tuple(f"short-{P}" for P in SHORT)
# Per-(scene, tensor) exceptions to the factor 1.5 (the rule of tests/backward_scenes.py: where a tensor needs more, measure both
# shares on the GPU, factor = measured ratio x 1.25, named with its measurement here and in the test's docstring).
# None so far: every comparison holds at 1.5 (the run-to-run spread is in DESIGN.md).
FACTORS = {}
# conditions of the deep scenes (pixels' deepest n_contrib, either state plane)
MIN_DEPTH = {"deep": 4000, "piled": 8192}
PILED_MIN = {"level0": 900, "level2": 40}


def _faint(scene):
    scene = dict(scene)
    scene["opacities"] = (scene["opacities"] * OPACITY_FACTOR).astype(np.float32)
    return scene


def _faint_cloud(gaze, alpha=0.6, width=200, height=120):
    from tests.helpers import small_case
    scene, cam = small_case(VARIANT, bg=R.BG, gaze=gaze, alpha=alpha, width=width, height=height)
    return _faint(scene), cam


def build(name):
    """-> (scene, cam, settings): the oracle-style input dicts of the named scene; settings: None (the four-level defaults, forward by
    the C oracle) or a FoveationSettings (forward by the numpy derivation under its constants)."""
    if name == "faint":
        return _faint_cloud((0.4, 0.55)) + (None,)
    if name == "faint-main":
        return _faint_cloud(R.MAIN["gaze"], R.MAIN["alpha"]) + (None,)
    if name == "deep":
        cloud = small_cloud(20000, 5)
        scene = _faint(scene_dict(cloud, VARIANT, syn.foveation_layers(cloud, seed=4)))
        return scene, cam_dict(small_camera(), bg=R.BG, gaze=(0.3, 0.45), alpha=0.6), None
    if name == "piled":
        cloud = syn.scene_1k(P=9000, seed=9)
        cloud._xyz[:, :2] *= 0.05
        cloud._opacity -= 3.5
        scene = scene_dict(cloud, VARIANT, syn.foveation_layers(cloud, seed=4))
        return scene, cam_dict(syn.camera_1k(64, 64), bg=R.BG, gaze=(0.3, 0.6), alpha=2.0), None
    if name in SHORT_NAMES:
        P = int(name.split("-")[1])
        cloud = syn.scene_1k(P=P, seed=40 + P)
        cloud._scaling += 2.3
        cloud._xyz[:, :2] *= 0.3
        highest, dcs, opac = syn.foveation_layers(cloud, seed=4)
        scene = scene_dict(cloud, VARIANT, (highest * 0 + 3.0, dcs, opac.clamp(0.3, 0.7)))  # (neither skipped by the alpha test nor saturating at once)
        return scene, cam_dict(syn.camera_1k(200, 120), bg=R.BG, gaze=(0.1, 0.9), alpha=0.3), None
    if name in TINY:
        return _faint_cloud((0.4, 0.55), width=TINY[name][0], height=TINY[name][1]) + (None,)
    if name == "nothing":
        cloud = syn.scene_1k(P=300, seed=6)
        cloud._xyz[:, 2] -= 8.0   # z in [-5, -3]: behind the identity camera
        scene = scene_dict(cloud, VARIANT, syn.foveation_layers(cloud, seed=7))
        return scene, cam_dict(syn.camera_1k(200, 120), bg=R.BG, gaze=(0.4, 0.55), alpha=0.6), None
    if name == "nothing-3x40":
        return _faint_cloud((0.4, 0.55), width=3, height=40) + (None,)
    if name in SETTINGS:
        from tests import foveation_helpers as fh
        from tests.test_fov_backward_gpu import SETTINGS as S
        settings, alpha, gaze = S[name.split("-")[1]]
        scene, cam = fh.fov_case(settings, alpha, gaze, width=200, height=120, bg=R.BG)
        return _faint(scene), cam, settings
    raise KeyError(name)


def forward(scene, cam, settings):
    if settings is None:
        return orc.forward(VARIANT, scene, cam)
    import pytest
    from tests import foveation_helpers as fh
    with pytest.MonkeyPatch.context() as mp:   # (the derivation reads its constants as module globals at call time)
        return fh.derivation(mp, settings, scene, cam)


def make_ref(fwd, scene, cam, settings):
    if settings is None:
        return R.FovBackwardRef(fwd, scene, cam)
    return R.FovBackwardRef(fwd, scene, cam, levels=settings.levels, start_blend=settings.start_blend, blend_width=settings.blend_width)


def gradients(ref, dpix):
    """-> (g32, g64): the reference's arithmetic in float32 and in double, both on the same frozen forward decisions."""
    return ref.backward(dpix, dtype=np.float32), ref.backward(dpix)


def census(ref, fwd, scene, g64):
    """Masks over the [P, L] rows, from the reference and the float64 gradients:
      live           dL_dopacities != 0                          level0 .. level3   live rows of that level
      single         live rows a single-level tile accumulated   lower / upper      ... state 0 / state 1 of a two-level tile did
      upper_skips    live rows of Gaussians that the upper state of some two-level tile skipped by the existence test
      clamped        live rows with a colour channel clamped at that level
    and `channels_clamped` [P, L, 3]: the clamped channels of the rows a tile used."""
    P, L = ref.P, ref.L
    live = np.asarray(g64["dL_dopacities"]) != 0
    cen = dict(live=live)
    for lev in range(4):
        m = np.zeros((P, L), bool)
        if lev < L:
            m[:, lev] = live[:, lev]
        cen[f"level{lev}"] = m
    lower, upper, skipped = np.zeros((P, L), bool), np.zeros((P, L), bool), np.zeros(P, bool)
    highest = np.asarray(scene["highest_levels"], np.float32).reshape(-1)
    tmin = np.asarray(fwd["tile_min"], np.float32)
    for t, tl in enumerate(ref.tiles):
        if not tl["blend"]:
            continue
        for mask, st in zip((lower, upper), tl["states"]):
            mask[tl["g"][st["acc"].any(axis=1)], st["lev"]] = True
        with np.errstate(all="ignore"):
            skipped[tl["g"][(highest[tl["g"]] + np.float32(1)) < (tmin[t] + np.float32(1))]] = True
    used = ref.used_single | ref.used_blend
    channels = (np.nan_to_num(ref.colours, nan=1.0) == 0) & used[..., None]
    cen.update(single=live & ref.used_single, lower=live & lower, upper=live & upper, upper_skips=live & skipped[:, None],
               clamped=live & channels.any(axis=2), channels_clamped=channels)
    return cen


def counts(cen):
    return {k: int(v.sum()) for k, v in cen.items() if k != "channels_clamped"}


def depth(ref):
    """-> (longest tile list, deepest n_contrib over both state planes, two-level tiles, state-0 pixels that start finished)"""
    longest = max((len(tl["g"]) for tl in ref.tiles), default=0)
    deepest = max((int(st["n_contrib"].max()) for tl in ref.tiles for st in tl["states"]), default=0)
    blend = sum(1 for tl in ref.tiles if tl["blend"])
    started = sum(int(((tl["states"][0]["n_contrib"] == 0) & tl["inside"] & (tl["states"][1]["n_contrib"] > 0)).sum()) for tl in ref.tiles if tl["blend"])
    return dict(longest_list=longest, deepest_n_contrib=deepest, two_level_tiles=blend, start_finished=started)


def _lock(*dicts):
    for d in dicts:
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The named scene's forward (C oracle, or the derivation under a setting), FovBackwardRef, loss gradient, float32 / float64
    gradients and census: computed once per session and shared (read-only: the arrays are locked)."""
    scene, cam, settings = build(name)
    fwd = forward(scene, cam, settings)
    ref = make_ref(fwd, scene, cam, settings)
    dpix = R.dL_for(cam)
    g32, g64 = gradients(ref, dpix)
    out = dict(name=name, scene=scene, cam=cam, settings=settings, fwd=fwd, ref=ref, dpix=dpix, g32=g32, g64=g64, census=census(ref, fwd, scene, g64),
               L=ref.L, depth=depth(ref))
    _lock(scene, {k: v for k, v in fwd.items() if isinstance(v, np.ndarray)}, g32, g64, out["census"])
    dpix.setflags(write=False)
    return out


def whole_tiles(ref, P):
    """-> (tiles whose list holds all P entries, the two-level ones among them)"""
    full = [tl for tl in ref.tiles if len(tl["g"]) == P]
    return len(full), sum(1 for tl in full if tl["blend"])


def rows(x, L):
    return R.rows(x, L)


def judge(got, g32, g64, cen, tag, L, branches=(), min_rows=MIN_LIVE, factors=None, against_f32=True):
    """THE comparison of the scene tests: backward_scenes.judge's clauses on the three tensors, one row per (Gaussian, level). `got`
    (the HIP library's gradients, or a doctored copy of the float32 reference in the CPU half) and the float32 reference `g32` are
    both held against the float64 reference `g64` on the same forward decisions (checks.check_against_noise: factor 1.5, floor 1e-4,
    abs_rows 3.5, tail_floor 0.5e-4; `factors`: per-tensor exceptions, measured x 1.25) -- on all rows AND on the live rows of every
    branch in `branches` on their own; (against_f32) the whole tensor agrees with the float32 reference within check_grad's cosine /
    relative-L2 bounds wherever the reference's own arithmetic is well inside them, with at least `min_rows` rows; dL_dshs_dcs is
    EXACTLY zero on clamped channels; and every row the reference leaves at zero is exactly zero, but for the stray allowance of
    test_fov_backward_gpu.compare() (max(3, GRAD_OUTLIERS x live rows): rows next to a flipped threshold pair)."""
    factors = factors or {}
    for k in TENSORS:
        assert np.shape(got[k]) == np.shape(g64[k]), f"{tag} {k}: shape {np.shape(got[k])}"
        g, f32, f64 = rows(got[k], L), rows(g32[k], L), rows(g64[k], L)
        assert np.isfinite(g).all(), f"{tag} {k}"   # (the harness poisons the outputs with NaN)
        kw = dict(factor=factors.get(k, FACTOR), floor=FLOOR, abs_rows=ABS_ROWS, tail_floor=TAIL_FLOOR)
        check_against_noise(g, f32, f64, f"{tag} {k}", **kw)
        for br in branches:
            sel = cen[br].reshape(-1)
            check_against_noise(g[sel], f32[sel], f64[sel], f"{tag} {k} [{br}: {int(sel.sum())} rows]", **kw)
        if against_f32:
            whole = bs.whole_tensor_judged(f32, f64)
            check_grad(g, f32, f"{tag} {k} (whole tensor)", outlier_frac=1.0, cosine=GRAD_COSINE if whole else np.inf,
                       rel_l2=GRAD_REL_L2 if whole else np.inf, min_rows=min_rows)
    exact_zeros(got, g64, cen, tag)


def exact_zeros(got, g64, cen, tag):
    assert np.all(np.asarray(got["dL_dshs_dcs"])[cen["channels_clamped"]] == 0.0), f"{tag}: a clamped channel passed a gradient to its DC coefficient"
    unused = np.asarray(g64["dL_dopacities"]) == 0
    allowed = stray_allowance(g64)
    for k in TENSORS:
        x = np.asarray(got[k])
        stray = int((x[unused] != 0).any(axis=-1).sum()) if x.ndim == 3 else int((x[unused] != 0).sum())
        assert stray <= allowed, f"{tag} {k}: {stray} (Gaussian, level) rows the reference leaves at zero carry a gradient (allowed {allowed})"


def stray_allowance(g64):
    return int(max(3, GRAD_OUTLIERS * int((np.asarray(g64["dL_dopacities"]) != 0).sum())))


def judge_short(got, g32, g64, cen, tag, L, min_rows):
    """Short scenes: EVERY row within 1e-4 relative of the float64 reference, no outlier share (the reference's own fp32 arithmetic
    is within 5.1e-6 on every row: a row sums at most a few hundred pixels of at most five entries), and the exact zeros."""
    for k in TENSORS:
        g, f64 = rows(got[k], L), rows(g64[k], L)
        st = grad_stats(g, f64, rtol=SHORT_RTOL)
        print(f"{tag} {k}: worst row {st['row_rel_max']:.2e} (float32 reference: {grad_stats(rows(g32[k], L), f64)['row_rel_max']:.2e})")
        check_grad(g, f64, f"{tag} {k} vs the double-precision reference", min_rows=min_rows)
        assert st["frac_bad"] == 0.0, f"{tag} {k}: a row is {st['row_rel_max']:.2e} off the double-precision gradient"
    exact_zeros(got, g64, cen, tag)


def without_last_entry_of_odd_lists(ref):
    """A copy of `ref` whose tiles with an odd number of entries never accumulate their last entry: what a fold that drops the pending
    entry computes (the CPU half's doctored defect)."""
    r2 = copy.copy(ref)
    r2.tiles = []
    for tl in ref.tiles:
        if len(tl["g"]) % 2 == 1:
            tl = dict(tl, states=[dict(st, acc=np.vstack([st["acc"][:-1], np.zeros((1, 256), bool)])) for st in tl["states"]])
        r2.tiles.append(tl)
    return r2


def with_cached_exponentials(ref):
    """A copy of `ref` that computes every tile's float64 exponentials once (the central differences evaluate a tile many times)."""
    r2 = copy.copy(ref)
    cache = {}

    def G(tl, F):
        key = (id(tl), np.dtype(F).name)
        if key not in cache:
            cache[key] = ref._G(tl, F)
        return cache[key]
    r2._G = G
    return r2


def without_background(ref):
    r2 = copy.copy(ref)
    r2.bg = np.zeros(3, np.float32)
    return r2


def record_census(name, cen, dep, extra=None):
    parity_report.record("census", f"{_where()} {name}", **counts(cen), **dep, **(extra or {}))


record_flipped_pixels = bs.record_flipped_pixels
