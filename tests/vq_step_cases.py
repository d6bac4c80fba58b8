"""The cases and the judges of the VQ codebook step (fr_vq_update, fr_vq_replace, the loss of fr_vq_gather), shared by
tests/test_vq_step_cpu.py (which shows that the judges judge) and tests/test_vq_step_gpu.py (which hands them the kernels' output).
A plain module: numpy only, every input a function of its case.

The shapes are the smallest that reach each path of csrc/vq.hip's step:
  1 / 1 / 1            degenerate
  1023, 1024, 1025 / 3 / 3   the first tile seam of the counting sort (VQ_TILE = 1024); k_vq_segsum's last workgroup (4 codes) not full
  4097 / 257 / 27      5 tiles: k_vq_rank's second workgroup holds one wave; k_vq_colscan's second workgroup holds one code (256, which
                       has members); segments of 0, 1, 63, 64, 65, 128, 129 and 749 rows around k_vq_segsum's 64-row batches; many codes empty
  5000 / 1025 / 48     k_vq_segscan with per = 2 and threads beyond K
  3000 / 2500 / 64     per = 3, n ~ K, every lane of D in use
  9000 / 8192 / 48     the shipped K (per = 8)
  300 / 1024 / 27      n < K, less than one tile
  6000 / 5 / 27        one code with 3500 members (its segment crosses four seams of the sorted order and lies across all six tiles), one
                       empty: the exact judge only -- general-data segments stay below 800 rows, where a dropped row still moves
                       the result by many times the rounding bound
The 4097 and 5000 shapes run also through `rows` (int32 and int64) into a pool of 1.5 n rows with repeats, weights indexed by pool row."""
import collections
import functools

import numpy as np

from tests import parity_report, vq_ref

Case = collections.namedtuple("Case", "n K D assign rows")  # rows: None, "int32" or "int64"
DECAY, EPS = 0.8, 1e-5
MAX_GENERAL_SEGMENT = 800

_SHAPES = [(1, 1, 1, "uniform"), (1023, 3, 3, "uniform"), (1024, 3, 3, "uniform"), (1025, 3, 3, "uniform"), (4097, 257, 27, "skewed"),
           (5000, 1025, 48, "uniform"), (3000, 2500, 64, "uniform"), (9000, 8192, 48, "uniform"), (300, 1024, 27, "uniform")]
GENERAL = [Case(*s, None) for s in _SHAPES] + [Case(*s, r) for s in (_SHAPES[4], _SHAPES[5]) for r in ("int32", "int64")]
EXACT = GENERAL + [Case(6000, 5, 27, "long", None)]


def case_id(c):
    return f"{c.n}-{c.K}-{c.D}" + (f"-{c.rows}" if c.rows else "")


def _rng(c, salt):
    return np.random.default_rng([c.n, c.K, c.D, salt, 0 if c.rows is None else int(c.rows[3:])])


def assignment(c):
    """int32 [n]: the code of every row of the call"""
    g = _rng(c, 1)
    n, K = c.n, c.K
    if c.assign == "uniform":
        ind = g.integers(0, K, n)
        ind[n // 2] = K - 1  # the last code has a member (k_vq_segscan's last thread with work, k_vq_segsum's last wave)
    elif c.assign == "skewed":
        lengths = np.zeros(K, np.int64)
        lengths[:8] = (0, 1, 63, 64, 65, 128, 129, 749)
        lengths[K - 1] = 130
        used = np.arange(8, K - 1, 3)  # two codes of three have no member
        rest = n - lengths.sum()
        lengths[used] = rest // used.size
        lengths[used[:rest % used.size]] += 1
        ind = g.permutation(np.repeat(np.arange(K), lengths))
    else:  # long: code 1 holds 3500 rows, code 3 none
        lengths = np.array([700, 3500, 900, 0, 900])
        assert c.K == 5 and lengths.sum() == n
        ind = g.permutation(np.repeat(np.arange(K), lengths))
    assert ind.shape == (n,) and ind.min() >= 0 and ind.max() < K
    return ind.astype(np.int32)


def _exact_weights(g, gathered_to_pool, N):
    """Pool weights in {1, 2, 4} whose n gathered values have mean exactly 2: then w' = w n / (2 n) is exactly 0.5, 1 or 2"""
    n = gathered_to_pool.shape[0]
    w = g.choice(np.array([1.0, 2.0, 4.0], np.float32), N, p=(0.4, 0.4, 0.2))
    count = np.bincount(gathered_to_pool, minlength=N)
    deficit = 2 * n - int(w[gathered_to_pool].astype(np.int64).sum())
    for r in np.nonzero(count == 1)[0]:  # rows drawn exactly once move the sum by their own change
        if deficit == 0:
            break
        cur = int(w[r])
        new = min((1, 2, 4), key=lambda v: (abs(deficit - (v - cur)), v))
        deficit -= new - cur
        w[r] = new
    assert deficit == 0 and float(w[gathered_to_pool].astype(np.float64).sum()) == 2.0 * n
    return w


@functools.lru_cache(maxsize=None)
def inputs(c, kind, weighted=True):
    """kind "exact": x integer-valued in -8 .. 8, weights in {1, 2, 4} with mean exactly 2 (or None); "general": x ~ N(0, 1), weights in
    [0.5, 2]. -> dict(feats [N, D], weights [N] or None, rows [n] or None, ind int32 [n], embed [K, D], cs [K], x = feats[rows],
    w = weights[rows]); treat the arrays as read-only (they are shared)"""
    g = _rng(c, 2 if kind == "exact" else 3)
    n, K, D = c.n, c.K, c.D
    N = n if c.rows is None else n + n // 2
    rows = None if c.rows is None else g.integers(0, N, n).astype(c.rows)
    src = np.arange(n) if rows is None else rows.astype(np.int64)
    if kind == "exact":
        feats = g.integers(-8, 9, (N, D)).astype(np.float32)
        weights = _exact_weights(g, src, N) if weighted else None
    else:
        feats = g.standard_normal((N, D)).astype(np.float32)
        weights = g.uniform(0.5, 2.0, N).astype(np.float32) if weighted else None
    embed = g.standard_normal((K, D)).astype(np.float32)
    cs = (g.uniform(0.0, 2.0, K) * max(n / K, 1.0)).astype(np.float32)
    cs[g.integers(0, K, max(K // 16, 1))] = 0.0  # codes that start from nothing, as every code does in the first iteration
    out = dict(feats=feats, weights=weights, rows=rows, ind=assignment(c), embed=embed, cs=cs, x=feats[src],
               w=None if weights is None else weights[src])
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def same_bits(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (f"{what}: {bad.shape[0]} of {np.asarray(want).size} elements differ in their bits, first at {bad[0].tolist()}: "
                           f"got {np.asarray(got)[tuple(bad[0])]!r}, want {np.asarray(want)[tuple(bad[0])]!r}")


# ---- the three judges of fr_vq_update: each takes the state a step left behind ------------------------------------------------------
def judge_exact(got_embed, got_cs, I, decay):
    """Judge 1: on exact inputs every partial sum is representable, so no order of addition can excuse a difference"""
    want = vq_ref.emulate_update(I["x"], I["w"], I["ind"], I["embed"], I["cs"], decay, EPS)
    if decay == 0 and I["w"] is None:
        assert np.array_equal(got_cs, np.bincount(I["ind"], minlength=I["embed"].shape[0]).astype(np.float32)), "cluster_size is not the member count"
    same_bits(got_cs, want["cluster_size"], "cluster_size")
    same_bits(got_embed, want["embed"], "embed")


def judge_general(got_embed, got_cs, I, name=None):
    """Judge 2: within update_bounds of the float64 step (taken at the float32 decay and eps the kernels are handed); a code with no
    member decays by exactly `decay`. -> the largest ratios to the bound"""
    decay, eps = float(np.float32(DECAY)), float(np.float32(EPS))
    ref = vq_ref.train_step(I["x"], I["w"], I["embed"], I["cs"], I["ind"], decay, eps)
    B = vq_ref.update_bounds(I["x"], I["w"], I["ind"], I["embed"], I["cs"], decay, eps)
    ratios = {}
    for what, got in (("cluster_size", got_cs), ("embed", got_embed)):
        d = np.abs(np.asarray(got, np.float64) - ref[what])
        assert np.isfinite(d).all(), what
        ratios[what] = float(np.max(d / np.maximum(B[what], 1e-300))) if (d > 0).any() else 0.0
    if name is not None:
        print(f"{name}: largest |got - float64| / bound: cluster_size {ratios['cluster_size']:.3f}, embed {ratios['embed']:.3f}")
        parity_report.record("vq", name, cluster_size_ratio_to_bound=ratios["cluster_size"], embed_ratio_to_bound=ratios["embed"])
    for what, r in ratios.items():
        assert r <= 1.0, f"{what}: {r:.3f} times the bound"
    empty = np.bincount(I["ind"], minlength=I["embed"].shape[0]) == 0
    same_bits(np.asarray(got_embed)[empty], (I["embed"] * np.float32(DECAY))[empty], "embed rows of codes with no member")
    return ratios


def judge_order(got_embed, got_cs, I):
    """Judge 3: ascending row position inside a code is the contract, so general data must give the emulation's bits"""
    want = vq_ref.emulate_update(I["x"], I["w"], I["ind"], I["embed"], I["cs"], DECAY, EPS)
    same_bits(got_cs, want["cluster_size"], "cluster_size")
    same_bits(got_embed, want["embed"], "embed")


def absorbing_segment():
    """The cross-check of the order that needs no emulation: unweighted, D = 1, K = 3; code 1's lowest row holds 2^24 and its 255 other rows
    1.0. Added in ascending row position every 1.0 is absorbed (2^24 + 1 rounds to even): the sum is exactly 2^24; any order that adds two
    of the small rows first gives at least 2^24 + 2. The segment spans the seam at row 1024. With decay 0, eps 0 and cluster sizes
    that start at 0, cluster_size[1] = 256, smoothed = fl(fl(256 / 2048) 2048) = 256 and embed[1] = sum / 256: exactly 65536 for
    2^24, 65536 + 2^-7 (representable) for 2^24 + 2. -> (x [n, 1], ind, embed0, cs0)"""
    n, K = 2048, 3
    g = np.random.default_rng(24)
    ind = g.choice(np.array([0, 2], np.int32), n)
    members = np.sort(g.choice(np.arange(900, 1200), 256, replace=False))
    assert members[0] < 1024 < members[-1]
    ind[members] = 1
    x = g.integers(-8, 9, (n, 1)).astype(np.float32)
    x[members] = 1.0
    x[members[0]] = 2.0 ** 24
    return x, ind, np.zeros((K, 1), np.float32), np.zeros(K, np.float32)


# ---- replacement ------------------------------------------------------------------------------------------------------------------------
REPLACE = [(1025, 1025, 10), (2500, 4097, 64), (8192, 9000, 10)]  # (K, n, k)


@functools.lru_cache(maxsize=None)
def replace_inputs(K, n, k, D=27):
    """Ties where k_vq_select could lose them: equal cluster sizes at i and i + 1024 (one thread's consecutive strides), at i and i + 1
    (neighbouring threads), and in the last partial stride; the k largest weights, in tied pairs (a triple first, so that k cuts a tie),
    at positions beyond 1024, in the last partial stride, and on pool rows that `rows` repeats.
    -> dict(feats, weights, rows int64, embed, cs, x, w)"""
    g = np.random.default_rng([K, n, k])
    N = n + n // 2
    m = k + 3
    tied = np.concatenate([[0], np.arange(m - 1) // 2]).astype(np.float32)  # 0 0 0 1 1 2 2 ...: k = m - 3 ends inside a pair

    def places(first, count):  # `first` (those that exist, once each), then the others: beyond 1024 before the rest
        first = list(dict.fromkeys(i for i in first if 0 <= i < count))
        others = [i for i in np.concatenate([1025 + g.permutation(max(count - 1025, 0)), g.permutation(min(count, 1025))]).tolist()
                  if i not in first]
        return np.array((first + others)[:m])
    cs = (100.0 + g.uniform(0, 50, K)).astype(np.float32)
    # the triple: one thread's strides (0, 1024) and its neighbour; a pair of neighbours; the last stride's first and last
    low = places([0, 1024, 1, 517, 518, (K - 1) // 1024 * 1024, K - 1], K)
    cs[low] = 0.25 + tied
    rows = g.integers(0, N, n).astype(np.int64)
    weights = g.uniform(0.0, 1.0, N).astype(np.float32)
    pos = places([1030, 2054, 1031, 1100, 1101, (n - 1) // 1024 * 1024, n - 1], n)
    fresh = g.permutation(N)[:m]  # distinct pool rows for the chosen positions, so that they tie by value ...
    stray = np.isin(rows, fresh)  # (no other position draws them: where the largest weights sit is decided here)
    rows[stray] = np.setdiff1d(np.arange(N), fresh)[g.integers(0, N - m, int(stray.sum()))]
    rows[pos] = fresh
    weights[fresh] = 10.0 + (tied.max() - tied)  # the triple largest
    rows[pos[4]] = rows[pos[3]]  # ... and one pool row drawn twice among the largest
    for a in (rows, weights, cs):
        a.setflags(write=False)
    feats = g.standard_normal((N, D)).astype(np.float32)
    embed = g.standard_normal((K, D)).astype(np.float32)
    return dict(feats=feats, weights=weights, rows=rows, embed=embed, cs=cs, x=feats[rows], w=weights[rows], k=k)


def judge_replace(got_embed, got_cs, R):
    """The k overwritten embed rows equal the chosen input rows, every other row and all of cluster_size keep their bits"""
    want, codes, rows = vq_ref.replace(R["embed"], R["cs"], R["x"], R["w"], R["k"])
    assert codes.size == R["k"] and np.unique(codes).size == R["k"]
    same_bits(got_cs, R["cs"], "cluster_size")
    same_bits(np.asarray(got_embed)[codes], R["x"][rows], "the overwritten rows")
    same_bits(got_embed, want, "embed")
    return codes, rows


# ---- loss ---------------------------------------------------------------------------------------------------------------------------
LOSS = [(1025, 3, 27, None), (4097, 257, 27, "int64"), (9000, 8192, 48, None)]  # (n, K, D, rows)


def judge_loss(got, x, embed, ind, D, weight=1.0):
    """|got - float64| <= (D + 2) u: per row a rounded difference (twice in its square), the square and the additions of at most D
    terms in float32, then a double sum and one rounding to float"""
    want = weight * np.mean((np.asarray(embed, np.float64)[ind] - np.asarray(x, np.float64)) ** 2)
    rel = abs(float(got) - want) / want
    assert rel <= (D + 2) * vq_ref.U, (float(got), want, rel / vq_ref.U)
    return rel / ((D + 2) * vq_ref.U)


# ---- SH-like data for the runs through the module ---------------------------------------------------------------------------------
def sh_like(n, K, D, seed):
    """-> (pool [1.5 n, D], importance [1.5 n], codebook [K, D]: perturbed pool rows)"""
    g = np.random.default_rng([n, K, D, seed])
    N = n + n // 2
    pool = (g.standard_normal((N, D)) * 0.3).astype(np.float32)
    pool[:, :3] += 0.8
    codes = pool[g.permutation(N)[:K]] + (0.05 * g.standard_normal((K, D))).astype(np.float32)
    return pool, (g.uniform(0, 1, N) ** 3 * 10 + 1e-3).astype(np.float32), codes.astype(np.float32)
