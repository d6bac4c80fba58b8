"""The foveated metameric (HVS) loss at sizes whose backward pass cuts texel footprints into row slices, without a GPU
(tests/golden/ref_hvs_fov_large.npz from make_hvs_fov_large_golden.py; cases S0 .. S6, tests/hvs_fov_large_cases.py):
the pictures drawn again from (seed, amplitude) have the stored CRC; the restatement (tests/hvs_fov_ref.py) in float64 and in
float32 against the reference's stored vectors, on their stride, under tests/test_hvs_fov_cpu.py's rules; a census, on the
LIBRARY's own backward plan (fr_hvs_fov_backward_plan), of what every case reaches: the slices, their populations, the seam
rows, one lane per texel, six levels; and the sensitivity of the GPU half's figures (tests/test_hvs_fov_large_gpu.py) to the
defects it is written for: a seam row or a whole slice that the backward pass leaves out."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native
from fov3dgs_amd.odak_perception import _native_hvs_fov
from tests import hvs_cases as hc
from tests import hvs_fov_cases as fc
from tests import hvs_fov_large_cases as lc
from tests import hvs_fov_ref, hvs_ref, parity_report

CASES = list(range(7))
LOD_ABS = 5e-3   # tests/test_hvs_fov_cpu.py's, for its reason (test_restated_lod_maps_match_the_stored_ones)
S = lc.STRIDE
#       (H, W, levels, orientations, alpha, mode, gaze, width, distance, colour space, Hs, Ws, asymmetric); the loss type apart
WANT = [(136, 244, 2, 2, 1.5, "quadratic", (0.3, 0.6), 1.0, 0.5, "RGB", 0, 0, False),
        (200, 344, 3, 2, 0.8, "quadratic", (0.2, 0.3), 1.0, 0.5, "RGB", 0, 0, False),
        (392, 408, 3, 2, 0.6, "linear", (0.5, 0.5), 1.0, 0.5, "RGB", 0, 0, False),
        (392, 408, 3, 2, 0.05, "quadratic", (0.5, 0.5), 1.0, 0.5, "RGB", 0, 0, False),
        (64, 64, 6, 6, 0.5, "quadratic", (0.4, 0.6), 1.0, 0.5, "RGB", 0, 0, False),
        (32, 32, 5, 1, 2.0, "quadratic", (0.3, 0.6), 1.0, 0.5, "RGB", 0, 0, True),
        (200, 344, 3, 2, 0.8, "quadratic", (0.2, 0.3), 1.0, 0.5, "RGB", 196, 340, False)]
# (case, pyramid level, k) -> (S, R, G): every chain level that is cut, and into what (make_hvs_fov_large_golden.py names them)
SLICED = {(0, 0, 7): (2, 68, 64),
          (1, 0, 7): (3, 67, 64), (1, 0, 8): (3, 67, 64),
          (2, 0, 7): (3, 89, 64), (2, 0, 8): (5, 79, 64), (2, 1, 7): (2, 98, 64),
          (3, 0, 7): (3, 89, 64), (3, 0, 8): (5, 79, 64), (3, 1, 7): (2, 98, 64),
          (6, 0, 7): (3, 67, 64), (6, 0, 8): (3, 67, 64)}


def _case(i):
    """the case, with its pictures proven to be the generator's"""
    c = lc.case(i)
    assert c.crc == int(lc.golden()[f"crc_{i}"]), f"{c.name}: the pictures drawn from (seed {c.seed}, amplitude {c.amp}) are not the generator's"
    return c


def test_fixture_holds_the_cases():
    z = lc.golden()
    assert int(z["n"]) == 7 == len(lc.NAMES)
    for i, want in enumerate(WANT):
        c = _case(i)
        got = (c.H, c.W, c.levels, c.orientations, c.alpha, c.mode, c.gaze, c.width, c.distance, c.colorspace, c.Hs, c.Ws, c.asymmetric)
        assert got == want, (i, got)
        assert c.loss_type == ("L1" if i == 0 else "MSE")   # (S0: the generator found a seed that meets KINK_SHARE)
        h, w = c.Hs or c.H, c.Ws or c.W
        assert c.img.shape == (1, 3, h, w) == c.tgt.shape and c.img.dtype == np.float32
        assert z[f"grad_{i}"].dtype == np.float32 and z[f"grad_{i}"].shape == (1, 3, -(-h // S), -(-w // S))
        assert z[f"refdist_{i}"].shape == (3,) and (z[f"refdist_{i}"] > 0).all()
        for l in range(c.levels - 1):
            assert z[f"lod_{i}_{l}"].dtype == np.float32 and z[f"lod_{i}_{l}"].shape == (-(-(c.H >> l) // S), -(-(c.W >> l) // S))
    assert all(v.dtype.kind in "fiu" for v in z.values())
    assert os.path.getsize(os.path.join(hc.GOLDEN, "ref_hvs_fov_large.npz")) < 850_000
    assert hc.asymmetry(lc.filters_of(lc.case(5))["b"][0]) >= hc.ASYMMETRY


def _strided(a):
    return a[..., ::S, ::S]


@pytest.mark.parametrize("i", CASES)
def test_restatement_in_float64_matches_the_reference_vectors(i):
    """tests/test_hvs_fov_cpu.py's rule, on the stored stride: 1e-4 relative for the loss, the gradient's relative L2 and its
    max/max. The stored distances over the WHOLE gradient (refdist) were measured against this yardstick by the generator: the
    yardstick here is the same one."""
    c, z, y = _case(i), lc.golden(), lc.yardstick(i)
    rel_loss = abs(float(z[f"loss_{i}"]) - y["loss"]) / y["loss"]
    l2, mx = hc.distances(z[f"grad_{i}"], _strided(y["grad"]))
    parity_report.record("hvs_fov", f"reference_vs_float64/{c.name}", rel_loss=rel_loss, grad_rel_l2_strided=l2, grad_max_over_max_strided=mx,
                         stored_rel_loss=z[f"refdist_{i}"][0], stored_grad_rel_l2=z[f"refdist_{i}"][1], stored_grad_max_over_max=z[f"refdist_{i}"][2])
    print(f"{c.name}: reference fp32 vs float64 on the stride: rel loss {rel_loss:.3e} grad rel L2 {l2:.3e} max/max {mx:.3e}; "
          f"stored, whole gradient: {z[f'refdist_{i}'].tolist()}")
    assert abs(rel_loss - z[f"refdist_{i}"][0]) <= 1e-9 + 1e-3 * rel_loss   # the generator's yardstick is this one
    assert rel_loss < 1e-4 and l2 < 1e-4 and mx < 1e-4


@pytest.mark.parametrize("i", CASES)
def test_restatement_in_float32_matches_the_reference_vectors(i):
    """tests/test_hvs_fov_cpu.py's rule: two float32 evaluations of one formula, each about one reference-distance from the
    yardstick, differ by at most twice the GPU tests' allowance of the reference's own distance (here on the stored stride)."""
    c, z, y, got = _case(i), lc.golden(), lc.yardstick(i), lc.float32_restatement(i)
    ref_rel = abs(float(z[f"loss_{i}"]) - y["loss"]) / y["loss"]
    ref_l2, ref_mx = hc.distances(z[f"grad_{i}"], _strided(y["grad"]))
    rel = abs(got["loss"] - float(z[f"loss_{i}"])) / y["loss"]
    l2, mx = hc.distances(_strided(got["grad"]), z[f"grad_{i}"])
    parity_report.record("hvs_fov", f"float32_restatement_vs_reference/{c.name}", rel_loss=rel, grad_rel_l2=l2, grad_max_over_max=mx)
    print(f"{c.name}: fp32 restatement vs reference: rel loss {rel:.3e} ({ref_rel:.3e}) grad rel L2 {l2:.3e} ({ref_l2:.3e}) "
          f"max/max {mx:.3e} ({ref_mx:.3e})")
    assert rel <= 2 * hc.allowance(ref_rel) and l2 <= 2 * hc.allowance(ref_l2) and mx <= 2 * hc.allowance(ref_mx)


@pytest.mark.parametrize("i", CASES)
def test_restated_lod_maps_match_the_stored_ones(i):
    """tests/test_hvs_fov_cpu.py's LOD_ABS and its reasoning: the smallest ecc^2 with lod > 0 among THESE cases is S2's (linear,
    alpha 0.6, 408 pixels wide: the pooling size 0.886 alpha ecc (distance / width) W reaches one pixel at ecc = 9.2e-3), where
    2.4e-7 x 2 / (8.5e-5 ln 2) / 2 = 4.1e-3"""
    c, z, y = _case(i), lc.golden(), lc.yardstick(i)
    for l in range(c.levels - 1):
        d = fc.max_abs(z[f"lod_{i}_{l}"], y["lods"][l][::S, ::S])
        parity_report.record("hvs_fov", f"reference_vs_float64/{c.name}/lod{l}", max_abs=d)
        print(f"{c.name} level {l}: reference fp32 LOD map vs float64 on the stride: max |d| {d:.3e} (max LOD {y['lods'][l].max():.3f})")
        assert d < LOD_ABS


@pytest.mark.parametrize("i", CASES)
def test_inputs_keep_both_kinks_away(i):
    c, y = _case(i), lc.yardstick(i)
    f = hvs_ref.filters_to(lc.filters_of(c), dtype=torch.float64)
    lods = [torch.tensor(m) for m in y["lods"]]
    img, tgt = torch.tensor(c.img, dtype=torch.float64), torch.tensor(c.tgt, dtype=torch.float64)
    if c.Hs:
        img, tgt = (torch.nn.functional.interpolate(v, size=(c.H, c.W), mode="bilinear", align_corners=False) for v in (img, tgt))
    assert hvs_fov_ref.variances_outside_band(img, tgt, f, lods, c.levels, image_colorspace=c.colorspace) == 0
    if c.loss_type == "L1":
        n, share = hvs_fov_ref.undecided_sign_gradient(img, tgt, f, lods, c.levels, image_colorspace=c.colorspace)
        print(f"{c.name}: {n} statistics differ by less than {hvs_ref.UNDECIDED}, share of the largest gradient {share:.3e}")
        assert share <= 2e-7                           # (the generator's KINK_SHARE)
        assert lc.golden()[f"refdist_{i}"][1] < 2e-5   # (the generator's REF_L2)


# ---------------------------------------------------------------- the census, on the library's own plan
def test_backward_plan_query():
    c = lc.case(2)
    p = lc.plan(c, 0, 7)
    assert p == lc.Plan(K=8, h=3, w=3, rows=267, cols=278, G=64, S=3, R=89, g=p.g, gpart=p.gpart)
    # the workspace holds g[k] [2,nmc,cells] and gpart[k] [S,2,nmc,cells] of every chain level, one behind the other
    st = _native_hvs_fov.Settings(c.H, c.W, 0.6, 1.0, 0.5, 0, 0.5, 0.5, c.levels, c.orientations, 1, 1)
    total = _native_hvs_fov.floats(st, 1)
    spans = []
    for l, k, q in lc.chain_levels(c):
        cells = 3 * (c.orientations + (1 if l == 0 else 0)) * q.h * q.w
        spans += [(q.g, q.g + 2 * cells), (q.gpart, q.gpart + q.S * 2 * cells)]
    spans.sort()
    assert spans[0][0] >= (c.orientations + 1) * 3 * c.H * c.W and spans[-1][1] <= total
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    lib, out = _native.load(), (ctypes.c_int64 * 10)()
    for args, msg in (((392, 408, 3, 2, 2, 1), "pyramid level 2 outside 0..1"), ((392, 408, 3, 2, -1, 1), "pyramid level"),
                      ((392, 408, 3, 2, 0, 0), "chain level 0 outside 1..8"), ((392, 408, 3, 2, 0, 9), "chain level 9"),
                      ((392, 404, 3, 2, 0, 1), "multiple of 2"), ((392, 408, 7, 2, 0, 1), "n_pyramid_levels"),
                      ((392, 408, 3, 9, 0, 1), "orientations"), ((64, 32, 5, 6, 0, 1), "reference")):
        assert lib.fr_hvs_fov_backward_plan(*args, out) == -1 and msg in _native.last_error(), (args, _native.last_error())
    assert lib.fr_hvs_fov_backward_plan(392, 408, 3, 2, 0, 1, None) == -1 and "null" in _native.last_error()


@pytest.mark.parametrize("i", CASES)
def test_every_case_reaches_the_plan_it_is_named_for(i):
    c = _case(i)
    got = {(i, l, k): (p.S, p.R, p.G) for l, k, p in lc.chain_levels(c) if p.S > 1}
    assert got == {key: v for key, v in SLICED.items() if key[0] == i}
    for l, k, p in lc.chain_levels(c):
        assert p.G == (1 if p.rows * p.cols <= 16 else 8 if p.rows * p.cols <= 256 else 64)
        assert (p.S > 1) == (p.rows * p.cols > 512 * p.G) and (p.S - 1) * p.R < p.rows <= p.S * p.R
        assert (p.h, p.w) == hvs_fov_ref.chain_sizes(c.H >> l, c.W >> l)[k] and p.K == len(hvs_fov_ref.chain_sizes(c.H >> l, c.W >> l)) - 1
    if i == 1:     # an uneven last slice: 67 + 67 + 66
        assert [b - a + 1 for a, b in lc.slices(lc.plan(c, 0, 8), 8, c.H, 0)] == [67, 67, 66]
    if i == 2:     # the interior texel row of the 3x3 level: its footprint starts and ends inside the picture; 5 slices, the last of 76
        p = lc.plan(c, 0, 7)
        assert 0 < lc.footprint_rows(p, 7, c.H, 1)[0] and lc.footprint_rows(p, 7, c.H, 1)[1] < c.H - 1 and (3 * 2 ** 20) % c.H
        assert lc.footprint_rows(p, 7, c.H, 0)[0] == 0 and lc.footprint_rows(p, 7, c.H, 2)[1] == c.H - 1
        assert [b - a + 1 for a, b in lc.slices(lc.plan(c, 0, 8), 8, c.H, 0)] == [79, 79, 79, 79, 76]
    if i == 4:     # six levels; level 4 is 4x4: one lane per texel
        assert c.levels == 6 and [(p.h, p.w, p.G) for l, k, p in lc.chain_levels(c) if l == 4] == [(2, 2, 1), (1, 1, 1)]
    if i == 5:     # a single orientation: one map above level 0; level 3 is 4x4
        assert c.orientations == 1 and [(p.h, p.w, p.G) for l, k, p in lc.chain_levels(c) if l == 3] == [(2, 2, 1), (1, 1, 1)]
    if i in (4, 5):  # ... and those levels are blended: their gradients are no zeros
        y = lc.yardstick(i)
        l = c.levels - 2
        assert y["lods"][l].max() > 1 and all(np.abs(y["chain"][(l, k)]).max() > 0 for k in (1, 2))


@pytest.mark.parametrize("i", [0, 1, 2, 3, 6])
def test_census_of_the_slices(i):
    """on the yardstick's LOD map: every slice of every sliced level holds, in at least one texel row's own row range, at least
    500 pixels that blend the level, and the two rows on either side of every seam at least 10 each; in S3 none holds any"""
    c, y = _case(i), lc.yardstick(i)
    for (ci, l, k), _ in sorted(SLICED.items()):
        if ci != i:
            continue
        p, h = lc.plan(c, l, k), c.H >> l
        rows = lc.contributing(y["lods"][l], k, p.K)
        per = [[int(rows[a:b + 1].sum()) for a, b in lc.slices(p, k, h, jy)] for jy in range(p.h)]
        best = [max(col) for col in zip(*per)]
        seams = sorted({a for jy in range(p.h) for a, b in lc.slices(p, k, h, jy)[1:] if a <= b})
        near = [int(rows[a + d]) for a in seams for d in (-2, -1, 0, 1)]
        parity_report.record("hvs_fov", f"census/{c.name}/level{l}/k{k}", slices=p.S, rows_per_slice=p.R, pixels_per_slice=str(best),
                             least_seam_row=min(near))
        print(f"{c.name} level {l} k {k}: S {p.S} R {p.R}: pixels per slice {per}, seams before rows {seams}, seam rows hold {near}")
        if i == 3:
            assert rows.sum() == 0 and np.floor(y["lods"][l].max()) + 1 < 7
        else:
            assert min(best) >= 500, best
            assert len(seams) >= p.S - 1 and min(near) >= 10, near


# ---------------------------------------------------------------- would the GPU half notice?
def _chain_allowance(i, key):
    """the GPU half's allowance on g[k]: 3 x the float32 restatement's own distance from the yardstick, floor 16 eps"""
    l2, mx = hc.distances(lc.float32_restatement(i)["chain"][key], lc.yardstick(i)["chain"][key])
    return hc.allowance(l2), hc.allowance(mx)


@pytest.mark.parametrize("i,l,k", [key for key in sorted(SLICED) if key[0] in (0, 1, 2)])
def test_a_dropped_seam_row_moves_the_chain_gradient_tenfold_beyond_its_allowance(i, l, k):
    """the first row of the second slice (of the middle texel row) passes nothing to level k: g[k] moves by more than ten times
    what tests/test_hvs_fov_large_gpu.py allows it"""
    c, y = _case(i), lc.yardstick(i)
    p = lc.plan(c, l, k)
    row = lc.slices(p, k, c.H >> l, p.h // 2)[1][0]
    got = lc.restate(c, torch.float64, cut=(l, k, row, row + 1))
    l2, mx = hc.distances(got["chain"][(l, k)], y["chain"][(l, k)])
    al2, amx = _chain_allowance(i, (l, k))
    gl2, _ = hc.distances(got["grad"], y["grad"])
    print(f"{c.name} level {l} k {k}: without row {row}: g[k] rel L2 {l2:.3e} (allowance {al2:.3e}) max/max {mx:.3e} ({amx:.3e}); "
          f"image gradient rel L2 {gl2:.3e} (allowance {hc.allowance(lc.golden()[f'refdist_{i}'][1]):.3e})")
    assert l2 > 10 * al2 and mx > 10 * amx


@pytest.mark.parametrize("i,l,k", [(0, 0, 7), (1, 0, 8), (2, 0, 8)])
def test_a_dropped_slice_moves_the_image_gradient_beyond_its_allowance(i, l, k):
    c, y, z = _case(i), lc.yardstick(i), lc.golden()
    p = lc.plan(c, l, k)
    a, b = lc.slices(p, k, c.H >> l, 0)[1]
    got = lc.restate(c, torch.float64, cut=(l, k, a, b + 1), chains=False)
    l2, mx = hc.distances(got["grad"], y["grad"])
    print(f"{c.name} level {l} k {k}: without rows {a}..{b}: image gradient rel L2 {l2:.3e} (allowance {hc.allowance(z[f'refdist_{i}'][1]):.3e}) "
          f"max/max {mx:.3e} ({hc.allowance(z[f'refdist_{i}'][2]):.3e})")
    assert l2 > hc.allowance(z[f"refdist_{i}"][1])
