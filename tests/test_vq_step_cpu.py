"""The judges of the VQ codebook step (tests/vq_step_cases.py), judged without a GPU: the exact cases really are exact, the general
cases cannot pass vacuously (one dropped member moves a code by at least 8 times the rounding bound), the float32 emulation of the
kernels (vq_ref.emulate_update) lies within the derived bounds of the float64 step, the inputs hold the structure they claim, and
every judge rejects a restatement that carries one defect of the kind a kernel could have."""
import numpy as np
import pytest

from tests import parity_report, vq_ref
from tests import vq_step_cases as C

F32_DECAY, F32_EPS = float(np.float32(C.DECAY)), float(np.float32(C.EPS))
ids = dict(ids=C.case_id)


def emulate(I, decay=C.DECAY, **kw):
    r = vq_ref.emulate_update(I["x"], I["w"], I["ind"], I["embed"], I["cs"], decay, C.EPS, **kw)
    return r["embed"], r["cluster_size"]


def rejected(judge, *args):
    with parity_report.muted():
        with pytest.raises(AssertionError):
            judge(*args)


# ---- the table -------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_the_paths_it_names():
    shapes = {(c.n, c.K, c.D) for c in C.EXACT}
    assert shapes == {(1, 1, 1), (1023, 3, 3), (1024, 3, 3), (1025, 3, 3), (4097, 257, 27), (5000, 1025, 48), (3000, 2500, 64), (9000, 8192, 48),
                      (300, 1024, 27), (6000, 5, 27)}
    assert [c for c in C.EXACT if c not in C.GENERAL] == [C.Case(6000, 5, 27, "long", None)]
    assert {(c.n, c.rows) for c in C.GENERAL if c.rows} == {(n, r) for n in (4097, 5000) for r in ("int32", "int64")}
    per = {c.K: (c.K + 1023) // 1024 for c in C.EXACT}
    assert per[1025] == 2 and per[2500] == 3 and per[8192] == 8 and 1023 * per[1025] > 1025  # (threads whose `lo` lies beyond K)
    for c in C.EXACT:
        ind = C.assignment(c)
        lengths = np.bincount(ind, minlength=c.K)
        assert lengths[c.K - 1] > 0 or c.n < c.K
        if c in C.GENERAL:
            assert lengths.max() <= C.MAX_GENERAL_SEGMENT
        if c.assign == "skewed":
            assert lengths[:8].tolist() == [0, 1, 63, 64, 65, 128, 129, 749] and (lengths == 0).sum() > c.K // 2 and lengths[256] > 64
            assert (c.n + 1023) // 1024 == 5 and c.K % 4 == 1 and c.K > 256
            # every tile holds members of the long segments: their sums cross every seam
            assert all(np.unique(ind[t * 1024:(t + 1) * 1024][np.isin(ind[t * 1024:(t + 1) * 1024], (5, 6, 7))]).size == 3 for t in range(4))
        if c.assign == "long":
            assert lengths.tolist() == [700, 3500, 900, 0, 900]
            assert all((ind[t * 1024:(t + 1) * 1024] == 1).sum() > 64 for t in range(6))
        if c.rows:
            I = C.inputs(c, "general")
            assert I["rows"].dtype == np.dtype(c.rows) and I["feats"].shape[0] == c.n + c.n // 2 == I["weights"].shape[0]
            assert np.unique(I["rows"]).size < c.n and np.array_equal(I["w"], I["weights"][I["rows"]])


# ---- judge 1: the exact cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", (True, False))
@pytest.mark.parametrize("c", C.EXACT, **ids)
def test_exact_cases_are_exact(c, weighted):
    I = C.inputs(c, "exact", weighted)
    x, ind = I["x"].astype(np.float64), I["ind"]
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 8
    r = vq_ref.emulate_update(I["x"], I["w"], ind, I["embed"], I["cs"], C.DECAY, C.EPS)
    wp = r["wp"].astype(np.float64)
    if weighted:
        assert set(np.unique(I["w"])) <= {1.0, 2.0, 4.0} and I["w"].astype(np.float64).sum() == 2.0 * c.n
        assert np.array_equal(wp, I["w"] / 2.0)
    else:
        assert I["w"] is None and (wp == 1.0).all()
    # every term is a multiple of 1/2 and the magnitudes of a code's terms add to less than 2^23: every partial sum, in any order,
    # is a multiple of 1/2 below 2^23, which float32 holds exactly
    terms = wp[:, None] * x
    assert np.array_equal(2 * terms, np.round(2 * terms))
    mag = np.zeros(I["embed"].shape)
    np.add.at(mag, ind, np.abs(terms))
    assert mag.max() < 2.0 ** 23 and np.bincount(ind, weights=wp).max() < 2.0 ** 23
    exact = np.zeros(I["embed"].shape)
    np.add.at(exact, ind, terms)
    assert np.array_equal(r["embed_sum"].astype(np.float64), exact)
    assert np.array_equal(r["batch"].astype(np.float64), np.bincount(ind, weights=wp, minlength=c.K))
    # so the order inside a segment cannot matter: the reversed order gives the same bits
    perm, seg = vq_ref.sort_rows(ind, c.K)
    back = np.concatenate([perm[seg[k]:seg[k + 1]][::-1] for k in range(c.K)])
    for decay in (C.DECAY, 0.0):
        e, cs = emulate(I, decay)
        C.judge_exact(e, cs, I, decay)
        e2, cs2 = emulate(I, decay, perm=back, seg=seg)
        C.same_bits(e2, e, "embed")
        C.same_bits(cs2, cs, "cluster_size")
    if not weighted:
        assert np.array_equal(emulate(I, 0.0)[1], np.bincount(ind, minlength=c.K))


# ---- judge 2: the general cases --------------------------------------------------------------------------------------------
def removal_margin(I):
    """For every row: the largest move, in units of the bound, of a component of its code's embed row when that one member is taken
    out of the float64 sums. -> the smallest over the rows"""
    x, e, cs, ind = I["x"].astype(np.float64), I["embed"].astype(np.float64), I["cs"].astype(np.float64), I["ind"].astype(np.int64)
    n, K = x.shape[0], e.shape[0]
    w = I["w"].astype(np.float64)
    wp = w * n / w.sum()
    ref = vq_ref.train_step(x, w, e, cs, ind, F32_DECAY, F32_EPS)
    B = vq_ref.update_bounds(x, w, ind, e, cs, F32_DECAY, F32_EPS)["embed"]
    esum = np.zeros_like(e)
    np.add.at(esum, ind, wp[:, None] * x)
    omd = 1 - F32_DECAY
    S = ref["cluster_size"].sum()
    cs_i, S_i = ref["cluster_size"][ind] - omd * wp, S - omd * wp
    esum_i = esum[ind] - wp[:, None] * x
    with np.errstate(invalid="ignore", divide="ignore"):
        sm_i = (cs_i + F32_EPS) / (S_i + K * F32_EPS) * S_i
        mean_i = np.where(esum_i == 0, 0.0, esum_i / sm_i[:, None])  # (the only member: nothing is left to divide)
    moved = np.abs(F32_DECAY * e[ind] + omd * mean_i - ref["embed"][ind])
    return float((moved / B[ind]).max(axis=1).min())


@pytest.mark.parametrize("c", C.GENERAL, **ids)
def test_general_cases_cannot_pass_vacuously_and_the_emulation_is_within_the_bounds(c):
    I = C.inputs(c, "general")
    assert I["w"].min() >= 0.5 and I["w"].max() <= 2.0
    margin = removal_margin(I)
    assert margin >= 8.0, margin
    e, cs = emulate(I)
    ratios = C.judge_general(e, cs, I)
    assert 0 < max(ratios.values()) <= 1.0 or c.n == 1
    C.judge_order(e, cs, I)
    print(f"{C.case_id(c)}: a dropped member moves its code by >= {margin:.0f} bounds; the emulation lies at {ratios} of the bounds")


# ---- judge 3 and the defects -------------------------------------------------------------------------------------------------
def test_reversed_segments_change_the_bits_of_general_data_and_the_absorbing_segment():
    c = C.Case(4097, 257, 27, "skewed", None)
    I = C.inputs(c, "general")
    perm, seg = vq_ref.sort_rows(I["ind"], c.K)
    back = np.concatenate([perm[seg[k]:seg[k + 1]][::-1] for k in range(c.K)])
    e, _ = emulate(I)
    e2, _ = emulate(I, perm=back, seg=seg)
    several = np.bincount(I["ind"], minlength=c.K) > 1
    changed = (C.bits(e) != C.bits(e2)).any(axis=1)
    assert not changed[~several].any() and changed[several].mean() > 0.95
    # the segment that absorbs: ascending order gives exactly 2^24, any other start gives more
    x, ind, e0, cs0 = C.absorbing_segment()
    r = vq_ref.emulate_update(x, None, ind, e0, cs0, 0.0, 0.0)
    assert r["embed_sum"][1, 0] == 2.0 ** 24 and r["cluster_size"][1] == 256 and r["smoothed"][1] == 256 and r["embed"][1, 0] == 65536.0
    perm, seg = vq_ref.sort_rows(ind, 3)
    perm[[seg[1], seg[1] + 2]] = perm[[seg[1] + 2, seg[1]]]  # the large row third
    r = vq_ref.emulate_update(x, None, ind, e0, cs0, 0.0, 0.0, perm=perm, seg=seg)
    assert r["embed_sum"][1, 0] >= 2.0 ** 24 + 2 and r["embed"][1, 0] >= 65536.0 + 2.0 ** -7


def without_row(ind, K, row):
    perm, seg = vq_ref.sort_rows(ind, K)
    seg = seg.copy()
    seg[ind[row] + 1:] -= 1
    return perm[perm != row], seg


@pytest.mark.parametrize("c", (C.Case(1025, 3, 3, "uniform", None), C.Case(4097, 257, 27, "skewed", None), C.Case(5000, 1025, 48, "uniform", "int64")), **ids)
def test_the_first_row_of_the_second_tile_dropped_is_rejected(c):
    for kind, judges in (("exact", ("exact",)), ("general", ("general", "order"))):
        I = C.inputs(c, kind)
        perm, seg = without_row(I["ind"], c.K, 1024)
        e, cs = emulate(I, perm=perm, seg=seg)
        if "exact" in judges:
            rejected(C.judge_exact, e, cs, I, C.DECAY)
            e0, cs0 = emulate(I, 0.0, perm=perm, seg=seg)
            rejected(C.judge_exact, e0, cs0, I, 0.0)
        else:
            rejected(C.judge_general, e, cs, I)
            rejected(C.judge_order, e, cs, I)


@pytest.mark.parametrize("c", (C.Case(4097, 257, 27, "skewed", None), C.Case(5000, 1025, 48, "uniform", "int32")), **ids)
def test_two_members_swapped_across_a_tile_seam_are_rejected_by_the_order_judge_alone(c):
    I, X = C.inputs(c, "general"), C.inputs(c, "exact")
    assert np.array_equal(I["ind"], X["ind"])
    perm, seg = vq_ref.sort_rows(I["ind"], c.K)
    code_of = I["ind"][perm]
    at = np.nonzero((perm[:-1] < 1024) & (perm[1:] >= 1024) & (code_of[:-1] == code_of[1:]))[0]
    assert at.size > 0
    perm = perm.copy()
    perm[[at[0], at[0] + 1]] = perm[[at[0] + 1, at[0]]]
    e, cs = emulate(I, perm=perm, seg=seg)
    rejected(C.judge_order, e, cs, I)
    C.judge_general(e, cs, I)             # (the membership is intact: the rounding bound holds) ...
    e, cs = emulate(X, perm=perm, seg=seg)
    C.judge_exact(e, cs, X, C.DECAY)      # ... and judge 1 is blind to order by construction


@pytest.mark.parametrize("c", (C.Case(5000, 1025, 48, "uniform", None), C.Case(3000, 2500, 64, "uniform", None), C.Case(9000, 8192, 48, "uniform", None)), **ids)
def test_seg_off_by_one_for_codes_from_1024_is_rejected(c):
    for kind in ("exact", "general"):
        I = C.inputs(c, kind)
        perm, seg = vq_ref.sort_rows(I["ind"], c.K)
        seg = seg.copy()
        seg[1024:c.K] += 1
        e, cs = emulate(I, perm=perm, seg=seg)
        if kind == "exact":
            rejected(C.judge_exact, e, cs, I, C.DECAY)
        else:
            rejected(C.judge_general, e, cs, I)
            rejected(C.judge_order, e, cs, I)


@pytest.mark.parametrize("c", (C.Case(1, 1, 1, "uniform", None), C.Case(1024, 3, 3, "uniform", None), C.Case(300, 1024, 27, "uniform", None)), **ids)
def test_decay_and_its_complement_exchanged_in_the_cluster_size_ema_is_rejected(c):
    I = C.inputs(c, "exact")
    e, cs = emulate(I, defect="ema")
    rejected(C.judge_exact, e, cs, I, C.DECAY)
    e, cs = emulate(I, 0.0, defect="ema")
    rejected(C.judge_exact, e, cs, I, 0.0)
    I = C.inputs(c, "general")
    e, cs = emulate(I, defect="ema")
    rejected(C.judge_general, e, cs, I)
    rejected(C.judge_order, e, cs, I)


# ---- replacement -------------------------------------------------------------------------------------------------------------
def ties_seen_below_1024_only(v, k):
    """A selection whose tie rule holds only among indices below 1024: an index beyond goes before them, the highest first"""
    v = np.asarray(v)
    i = np.arange(v.shape[0])
    return np.lexsort((np.where(i < 1024, i, -i), v))[:k]


@pytest.mark.parametrize("K,n,k", C.REPLACE)
def test_replacement_inputs_hold_their_ties_and_the_judge_sees_a_lost_one(K, n, k):
    R = C.replace_inputs(K, n, k)
    want, codes, rows = vq_ref.replace(R["embed"], R["cs"], R["x"], R["w"], k)
    C.judge_replace(want, R["cs"], R)
    cs, w = R["cs"], R["w"]
    # cluster sizes: ties between one thread's strides, between neighbours, and one that k cuts
    assert cs[0] == cs[1024] == cs[1] and {0, 1, 1024} <= set(codes.tolist()) and cs[517] == cs[518] and {517, 518} <= set(codes.tolist())
    assert codes.max() >= (K - 1) // 1024 * 1024
    rest = np.setdiff1d(np.arange(K), codes)
    assert cs[rest].min() == cs[codes].max() and rest[cs[rest] == cs[codes].max()].min() > codes[-1]
    # weights: chosen beyond position 1024 and in the last partial stride, ties (one cut by k), a pool row drawn twice
    assert rows.max() >= (n - 1) // 1024 * 1024 and (rows > 1024).sum() >= min(k, n - 1025)
    assert np.unique(w[rows]).size < k
    left = np.setdiff1d(np.arange(n), rows)
    assert w[left].max() == w[rows].min() and left[w[left] == w[rows].min()].min() > rows[-1]
    assert np.unique(R["rows"][rows]).size < k
    if n > 2054:
        assert w[1030] == w[2054] == w[1031] and {1030, 1031, 2054} <= set(rows.tolist())
    # the defective selection differs on these inputs, and the judge says so
    bad_codes, bad_rows = ties_seen_below_1024_only(cs, k), ties_seen_below_1024_only(-w, k)
    assert not np.array_equal(bad_codes, codes) and not np.array_equal(bad_rows, rows)
    for c_, r_ in ((bad_codes, rows), (codes, bad_rows)):
        got = np.array(R["embed"], copy=True)
        got[c_] = R["x"][r_]
        rejected(C.judge_replace, got, R["cs"], R)
    got = want.copy()
    got[rest[0], 0] = np.nextafter(got[rest[0], 0], np.float32(9))  # a row that was not to be touched
    rejected(C.judge_replace, got, R["cs"], R)


def test_the_loss_judge():
    g = np.random.default_rng(5)
    x, e = g.standard_normal((1025, 27)).astype(np.float32), g.standard_normal((3, 27)).astype(np.float32)
    ind = g.integers(0, 3, 1025)
    d = x - e[ind]
    got = np.float32((d * d).astype(np.float64).sum() / (1025 * 27))
    assert C.judge_loss(got, x, e, ind, 27) <= 1.0
    with pytest.raises(AssertionError):
        C.judge_loss(np.float32((d[:1024] * d[:1024]).astype(np.float64).sum() / (1025 * 27)), x, e, ind, 27)  # the row past the stride lost
