"""The CPU half of the foveated backward-scene tests (tests/fov_backward_scenes.py; the GPU half is
tests/test_fov_backward_scenes_gpu.py), all on the reference alone.

For every scene: the CENSUS CONDITIONS the GPU comparisons rely on (conditions, not measurements), the reference's forward image
against the oracle's, the reference arithmetic's own noise (float32 against float64 on the same frozen decisions: recorded), central
differences of the frozen loss on the deep and the short scenes, and proof that the comparison the GPU half uses REJECTS a defect in
every branch: the float32 reference with one defect injected must fail judge(), the untouched one must pass.

Measured here (live = (Gaussian, level) rows with dL_dopacities != 0; per level 0 / 1 / 2 / 3; single / lower / upper state; rows of
Gaussians an upper state skipped; rows with a clamped channel; longest list; deepest n_contrib; two-level tiles; share of the
float32 reference's dL_dopacities rows outside 1e-4 of float64):
  faint        3034   2078 /  494 /  328 /  134   2339 /  964 /  617    895   459    792   792  15   1.3e-3
  faint-main   1305    301 /  348 /  242 /  414    751 /  549 /  582    372   188    545   545  18   0.8e-3
  deep         8916   2249 / 2972 / 1950 / 1745   4895 / 3200 / 4411   2456  1252   5146  4612  18   2.2e-3
  piled        2190   1440 /    0 /  750 /    0   2190 /    0 /    0      -   ...   8953  8868   3   2.7e-3
  faint-L2     3023   2049 /  974                 2604 /  778 /  537    457   470    792   792  13   1.3e-3
  faint-L3     2967   1250 / 1061 /  656          2416 / 1040 /  838    672   443    761   761  17   1.0e-3
  tiny-16x16   2502 (level 0, one single-level tile, list of 2981)     tiny-17x15  2518: 2494 / 14 / 10 (tile 0: tile_min -1.95)
  tiny-8x8     1837: 1184 lower / 653 upper (one two-level tile)        tiny-15x1    711 (level 1)
  short-1/2/3/5: tiles holding all P entries 64 / 24 / 38 / 16, two-level among them 11 / 4 / 8 / 5; float32 within 5.1e-6 of float64
dL_dlevel_colours and dL_dshs_dcs: a handful of float32 rows outside 1e-4 (worst row 1.6e-3, faint-L2): rows that meet a two-level tile
only where the blend weight 1 - smoothstep cancels (tests/fov_backward_ref.py)."""
import numpy as np
import pytest

from tests import backward_scenes as bs
from tests import fov_backward_scenes as fs
from tests import parity_report
from tests.checks import check_image, grad_stats

ALL_JUDGED = tuple(fs.LARGE) + fs.SETTINGS
# Sanity bound on the reference's own noise (share of live dL_dopacities rows outside 1e-4 of float64): the worst measured (piled,
# 2.7e-3) x 2, as tests/test_backward_scenes_cpu.py sets its own. Not a tolerance of the library.
NOISE_SANITY = 5.4e-3
SAMPLES_PER_LEVEL = 30


def _branches(name):
    if name in fs.LARGE:
        return fs.LARGE[name]
    L = int(name[-1])
    return fs.LEVELS[:L] + fs.STATES + ("upper_skips", "clamped")


@pytest.mark.parametrize("name", ALL_JUDGED)
def test_census_conditions(name):
    r = fs.reference(name)
    n, dep = fs.counts(r["census"]), r["depth"]
    print(name, n, dep, "instances", r["fwd"]["num_rendered"])
    fs.record_census(name, r["census"], dep)
    assert n["live"] >= fs.MIN_LIVE
    for br in _branches(name):
        assert n[br] >= fs.MIN_BRANCH, (br, n[br])
        # ten times as many live rows in the branch as the comparison lets be wrong within the branch's rows, tensor by tensor
        sel = r["census"][br].reshape(-1)
        for k in fs.TENSORS:
            share = grad_stats(fs.rows(r["g32"][k], r["L"])[sel], fs.rows(r["g64"][k], r["L"])[sel])["frac_bad"]
            wrong = bs.allowed_wrong_rows(share, n[br], factor=fs.FACTORS.get(name, {}).get(k, fs.FACTOR))
            assert n[br] >= 10 * wrong, (br, k, n[br], wrong)
    if name == "piled":
        for br, least in fs.PILED_MIN.items():
            assert n[br] >= least, (br, n[br])
    if name in fs.MIN_DEPTH:
        assert dep["deepest_n_contrib"] >= fs.MIN_DEPTH[name] and dep["longest_list"] >= fs.MIN_DEPTH[name]
    if name == "deep":   # the second state plane is walked deep as well, and some state-0 pixels start finished
        deepest_upper = max(int(tl["states"][1]["n_contrib"].max()) for tl in r["ref"].tiles if tl["blend"])
        assert deepest_upper >= 1000 and dep["start_finished"] > 0, deepest_upper
    if name != "piled":
        assert dep["two_level_tiles"] >= 10


@pytest.mark.parametrize("name", fs.SHORT_NAMES)
def test_short_scenes_hold_lists_of_every_length(name):
    P = int(name.split("-")[1])
    r = fs.reference(name)
    whole, two_level = fs.whole_tiles(r["ref"], P)
    n = fs.counts(r["census"])
    print(name, "tiles holding all entries", whole, "two-level among them", two_level, n)
    fs.record_census(name, r["census"], r["depth"], dict(whole_tiles=whole, whole_two_level_tiles=two_level))
    assert r["depth"]["longest_list"] == P and whole >= 4 and two_level >= 1
    assert all(n[lv] >= 1 for lv in fs.LEVELS) and n["lower"] >= 1 and n["upper"] >= 1
    for k in fs.TENSORS:   # the yardstick of the GPU half: the reference's own fp32 arithmetic is far inside 1e-4 on every row
        assert grad_stats(fs.rows(r["g32"][k], 4), fs.rows(r["g64"][k], 4))["row_rel_max"] <= fs.SHORT_REF_NOISE, k


@pytest.mark.parametrize("name", tuple(fs.TINY))
def test_tiny_frames(name):
    r = fs.reference(name)
    ref, n = r["ref"], fs.counts(r["census"])
    W, H = fs.TINY[name]
    print(name, n, r["depth"], "tile_min", r["fwd"]["tile_min"])
    fs.record_census(name, r["census"], r["depth"])
    assert (ref.W, ref.H) == (W, H) and len(ref.tiles) == ((W + 15) // 16) * ((H + 15) // 16)
    if name == "tiny-16x16":
        assert len(ref.tiles) == 1 and not ref.tiles[0]["blend"] and ref.tiles[0]["inside"].all() and n["live"] >= fs.MIN_LIVE
    elif name == "tiny-17x15":
        # two tiles: the first has tile_min <= -1 (level 0: see oracle/fovraster_oracle.c walk_one), the second is two-level
        assert [tl["blend"] for tl in ref.tiles] == [False, True] and r["fwd"]["tile_min"][0] <= -1.0
        assert n["level0"] >= fs.MIN_LIVE and n["lower"] >= 1 and n["upper"] >= 1
    elif name == "tiny-8x8":
        assert len(ref.tiles) == 1 and ref.tiles[0]["blend"] and int(ref.tiles[0]["inside"].sum()) == 64
        assert n["lower"] >= fs.MIN_BRANCH and n["upper"] >= fs.MIN_BRANCH
    else:
        assert len(ref.tiles) == 1 and int(ref.tiles[0]["inside"].sum()) == 15 and n["live"] >= fs.MIN_BRANCH


@pytest.mark.parametrize("name", fs.NOTHING)
def test_nothing_is_rendered(name):
    r = fs.reference(name)
    assert r["fwd"]["num_rendered"] == 0 and not (r["fwd"]["radii"] > 0).any()
    assert all(not np.asarray(r["g64"][k]).any() for k in fs.TENSORS)
    if name == "nothing-3x40":
        assert np.isnan(r["fwd"]["tile_min"]).all()
    else:   # the Gaussians are behind the camera, the tiles have levels
        assert np.isfinite(r["fwd"]["tile_min"]).all()


@pytest.mark.parametrize("name", ALL_JUDGED + fs.SHORT_NAMES + tuple(fs.TINY) + fs.NOTHING)
def test_reference_image_matches_the_forward(name):
    """The reference's forward image -- the frozen decisions evaluated in double and in float32 -- against the oracle's (the numpy
    derivation's under the two settings)."""
    r = fs.reference(name)
    check_image(r["ref"].image().astype(np.float32), r["fwd"]["color"], name=f"{name} reference image")
    check_image(r["ref"].image(dtype=np.float32), r["fwd"]["color"], name=f"{name} reference image fp32")


@pytest.mark.parametrize("name", ALL_JUDGED + tuple(fs.TINY))
def test_reference_noise_is_recorded_and_sane(name):
    r = fs.reference(name)
    L = r["L"]
    for k in fs.TENSORS:
        st = grad_stats(fs.rows(r["g32"][k], L), fs.rows(r["g64"][k], L))
        parity_report.record("oracle_noise", f"{name} fp32 vs fp64 reference backward {k}", **st)
        print(f"{name} {k}: outside 1e-4 {st['frac_bad']:.2e}, worst row {st['row_rel_max']:.1e}, rows {st['rows_with_gradient']}")
        assert st["frac_bad"] <= NOISE_SANITY, (k, st["frac_bad"])


# ---- central differences --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("deep",) + fs.SHORT_NAMES)
def test_reference_gradients_match_central_differences(name):
    """Check (b) of tests/test_fov_backward_cpu.py on the deep and the short scenes: loss = sum(dL_dpix * image) with the decisions
    frozen is linear in any single opacity or DC coefficient (no opacity is above 0.7: the 0.99 saturation binds nowhere), so a
    central difference is exact up to rounding: agreement to 1e-6 relative, on up to 30 sampled rows per level and tensor (every row
    of a short scene); entries whose gradient is below 1e-6 of the tensor's largest are not sampled."""
    r = fs.reference(name)
    ref, dL, g = fs.with_cached_exponentials(r["ref"]), r["dpix"], r["g64"]
    assert ref.opac.max() <= np.float32(0.98)
    rng = np.random.default_rng(5)
    h = 1e-2
    opac0, dcs0 = ref.opac.astype(np.float64), ref.dcs.astype(np.float64)
    worst, n = 0.0, 0
    for key, per_level in (("dL_dopacities", SAMPLES_PER_LEVEL), ("dL_dshs_dcs", SAMPLES_PER_LEVEL)):
        grad = g[key]
        big = np.abs(grad) >= 1e-6 * np.abs(grad).max()
        for lev in range(4):
            cand = np.argwhere(big[:, lev])
            take = cand[rng.permutation(len(cand))[:per_level]]
            assert len(take) >= (1 if name != "deep" else per_level), (key, lev, len(take))
            for c in take:
                idx = (int(c[0]), lev) + tuple(int(x) for x in c[1:])
                # (a tile none of whose states blends level `lev` gives both evaluations the same value: left out, exactly)
                tiles = [t for t in ref.tiles_with(idx[0]) if any(st["lev"] == lev for st in ref.tiles[t]["states"])]
                base = opac0 if key == "dL_dopacities" else dcs0
                hi, lo = base.copy(), base.copy()
                hi[idx] += h
                lo[idx] -= h
                if key == "dL_dopacities":
                    fd = (ref.frozen_loss(dL, hi, dcs0, tiles) - ref.frozen_loss(dL, lo, dcs0, tiles)) / (2 * h)
                else:
                    fd = (ref.frozen_loss(dL, opac0, hi, tiles) - ref.frozen_loss(dL, opac0, lo, tiles)) / (2 * h)
                an = grad[idx]
                worst, n = max(worst, abs(fd - an) / abs(an)), n + 1
                assert abs(fd - an) <= 1e-6 * abs(an), (key, idx, fd, an)
    print(name, "samples", n, "worst relative difference", worst)


# ---- the comparison rejects a defect in every branch ---------------------------------------------------------------------------
def _copy(g):
    return {k: np.array(v) for k, v in g.items()}


def _scale_rows(mask_name):
    def f(r, g):
        sel = r["census"][mask_name]
        for k in fs.TENSORS:
            g[k][sel] *= np.float32(1 + 3e-4)
    return f


def _swap_levels(a, b):
    def f(r, g):
        for k in fs.TENSORS:
            g[k][:, [a, b]] = g[k][:, [b, a]]   # what a misrouted row_comp leaves
    return f


def _no_background(r, g):
    g.update(_copy(fs.without_background(r["ref"]).backward(r["dpix"], dtype=np.float32)))


def _defects():
    out = []
    for name in ALL_JUDGED:
        br = _branches(name)
        levels = [b for b in br if b.startswith("level")]
        for b in levels:
            out.append(pytest.param(name, _scale_rows(b), id=f"{name}-{b}-scaled"))
        for b in br:
            if b in ("upper", "lower", "single", "upper_skips", "clamped"):
                out.append(pytest.param(name, _scale_rows(b), id=f"{name}-{b}-scaled"))
        a, b = int(levels[0][-1]), int(levels[-1][-1])
        out.append(pytest.param(name, _swap_levels(a, b), id=f"{name}-levels-{a}-{b}-swapped"))
        out.append(pytest.param(name, _no_background, id=f"{name}-no-background"))
    return out


@pytest.mark.parametrize("name,defect", _defects())
def test_the_comparison_rejects_a_defect(name, defect):
    """One level's rows, or one state's (single / lower / upper), or the rows of Gaussians an upper state skipped, or the rows with a
    clamped channel scaled by 1 + 3e-4; the components of two levels swapped; the background term dropped from dL_dopacities: each
    fails the ROW comparison against the reference's noise (the whole-tensor bounds against the float32 reference are left out: the
    doctored tensor IS the float32 reference but for the defect). The untouched float32 reference passes."""
    r = fs.reference(name)
    br = _branches(name)
    g = _copy(r["g32"])
    defect(r, g)
    assert any(not np.array_equal(g[k], r["g32"][k]) for k in fs.TENSORS)
    with parity_report.muted():   # (doctored inputs: nothing measured here belongs in the report)
        fs.judge(r["g32"], r["g32"], r["g64"], r["census"], f"{name} untouched", r["L"], branches=br, factors=fs.FACTORS.get(name))
        with pytest.raises(AssertionError, match="outside|beyond"):
            fs.judge(g, r["g32"], r["g64"], r["census"], f"{name} defect", r["L"], branches=br, against_f32=False, factors=fs.FACTORS.get(name))


@pytest.mark.parametrize("name", ("faint", "deep"))
def test_a_defect_confined_to_the_upper_state_is_caught_by_its_branch(name):
    """The rows of `upper` off by 3e-4 fail the branch's own comparison, tensor by tensor, also when the whole tensor's fraction is
    not asked."""
    r = fs.reference(name)
    g = _copy(r["g32"])
    _scale_rows("upper")(r, g)
    sel = r["census"]["upper"].reshape(-1)
    for k in fs.TENSORS:
        with parity_report.muted(), pytest.raises(AssertionError, match=r"\[upper"):
            fs.check_against_noise(fs.rows(g[k], 4)[sel], fs.rows(r["g32"][k], 4)[sel], fs.rows(r["g64"][k], 4)[sel], f"{k} [upper", floor=fs.FLOOR,
                                   abs_rows=fs.ABS_ROWS, tail_floor=fs.TAIL_FLOOR)


@pytest.mark.parametrize("name", fs.SHORT_NAMES)
def test_the_short_comparison_rejects_a_dropped_last_entry(name):
    """The last entry of every odd-length list dropped -- a fold that loses its pending entry -- fails the every-row comparison of the
    short scenes; so do a level's rows off by 3e-4. The untouched float32 reference passes."""
    r = fs.reference(name)
    live = int(r["census"]["live"].sum())
    odd = sum(1 for tl in r["ref"].tiles if len(tl["g"]) % 2 == 1)
    assert odd >= 4
    with parity_report.muted():
        fs.judge_short(r["g32"], r["g32"], r["g64"], r["census"], f"{name} untouched", 4, min_rows=live)
        dropped = fs.without_last_entry_of_odd_lists(r["ref"]).backward(r["dpix"], dtype=np.float32)
        assert not np.array_equal(dropped["dL_dopacities"], r["g32"]["dL_dopacities"])
        with pytest.raises(AssertionError):
            fs.judge_short(dropped, r["g32"], r["g64"], r["census"], f"{name} dropped", 4, min_rows=0)
        for lev in range(4):
            g = _copy(r["g32"])
            _scale_rows(f"level{lev}")(r, g)
            with pytest.raises(AssertionError, match="off the double-precision|outside"):
                fs.judge_short(g, r["g32"], r["g64"], r["census"], f"{name} level {lev}", 4, min_rows=live)


@pytest.mark.parametrize("name", ("faint", "piled", "tiny-8x8"))
def test_values_on_rows_the_reference_leaves_at_zero_are_rejected(name):
    """1e-30 on rows the reference leaves at zero is inside every relative tolerance; the exact-zero clause catches it as soon as
    there are more such rows than compare()'s stray allowance (max(3, 3e-3 x live rows): neighbours of a flipped pair). And 1e-30 on
    a clamped channel of dL_dshs_dcs is caught on a single element."""
    r = fs.reference(name)
    dead = np.argwhere((r["g64"]["dL_dopacities"] == 0) & ~r["census"]["channels_clamped"].any(axis=2))
    allowed = fs.stray_allowance(r["g64"])
    assert len(dead) > allowed + 1
    with parity_report.muted():
        g = _copy(r["g32"])
        for i, lv in dead[:allowed]:
            g["dL_dopacities"][i, lv] = np.float32(1e-30)
        fs.judge(g, r["g32"], r["g64"], r["census"], f"{name} allowed strays", r["L"], against_f32=False)
        for k in fs.TENSORS:
            g = _copy(r["g32"])
            for i, lv in dead[:allowed + 1]:
                g[k][i, lv] = np.float32(1e-30)
            with pytest.raises(AssertionError, match="leaves at zero"):
                fs.judge(g, r["g32"], r["g64"], r["census"], f"{name} strays", r["L"], against_f32=False)
        g = _copy(r["g32"])
        ch = np.argwhere(r["census"]["channels_clamped"])
        assert len(ch) >= 1
        g["dL_dshs_dcs"][tuple(ch[0])] = np.float32(1e-30)
        with pytest.raises(AssertionError, match="clamped channel"):
            fs.judge(g, r["g32"], r["g64"], r["census"], f"{name} clamped", r["L"], against_f32=False)


def test_min_rows_guard():
    r = fs.reference("faint")
    n = min(grad_stats(fs.rows(r["g32"][k], 4), fs.rows(r["g32"][k], 4))["rows_with_gradient"] for k in fs.TENSORS)
    assert n >= fs.MIN_LIVE
    with parity_report.muted():
        fs.judge(r["g32"], r["g32"], r["g64"], r["census"], "guard", 4, min_rows=n)
        with pytest.raises(AssertionError, match="rows carry a gradient"):
            fs.judge(r["g32"], r["g32"], r["g64"], r["census"], "guard", 4, min_rows=n + 1)
