"""The VQ codebook step on the MI355X beyond one sort tile and 64 codes: fr_vq_update (k_vq_rank, k_vq_colscan, k_vq_segscan, k_vq_place,
k_vq_segsum, k_vq_sum, k_vq_embed), fr_vq_replace (k_vq_select, k_vq_copy) and the loss of fr_vq_gather, called through
_native.load() with a workspace of the test's own, so that the test chooses the assignment (the search has its own tests).

Three judges (tests/vq_step_cases.py; tests/test_vq_step_cpu.py shows that each rejects a defective restatement):
  1  exact cases, bit for bit: integer x in -8 .. 8, weights None or in {1, 2, 4} with mean exactly 2 (w' in {0.5, 1, 2}): every partial
     sum is representable, so cluster_size and embed must equal vq_ref.emulate_update whatever the order of addition -- a difference
     is a membership or an arithmetic error. decay 0.8 and 0; at decay 0 without weights cluster_size is np.bincount(ind).
  2  general data (x ~ N(0, 1), weights in [0.5, 2], decay 0.8) against the float64 step: |got - train_step| <= vq_ref.update_bounds on
     every element (derived first-order bounds, not measured ones); rows of codes with no member equal fl(e decay) exactly.
  3  order: on the same data cluster_size and embed equal the emulation bit for bit (ascending row position is the contract), and a
     segment whose lowest row holds 2^24 and whose other rows hold 1.0 sums to exactly 2^24.
The replacement is judged by vq_ref.replace on ties between one thread's strides, between neighbouring threads, in the last partial
stride and on pool rows drawn twice; the loss by (D + 2) 2^-24 of the float64 value; the module and the loop by the emulation fed the
kernel's own assignment (itself held to vq_ref.check_assignment).

What the kernels gave on the MI355X (every comparison passed on its first run; tests/parity_report_gpu.json, kind vq, names "step ..."):
judges 1 and 3 and the replacement: equal bits in every case. Judge 2, largest |got - float64| / bound over the 13 cases: cluster_size
0.49 (5000 / 1025 / 48), embed 0.62 (5000 / 1025 / 48; 0.62 at 9000 / 8192 / 48, 0.57 at 3000 / 2500 / 64, 0.34 - 0.37 at 4097 / 257 / 27,
<= 0.05 at the K = 3 shapes) -- the figures of the numpy emulation, as equal bits imply. Loss: <= 0.015 of its bound. Ambiguous share
of the assignments handed on: <= 0.0027 (cap 0.02)."""
import functools

import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native, vectree
from tests import parity_report, vq_ref
from tests import vq_step_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_EXPIRE = 10
ids = dict(ids=C.case_id)


def _need_gpu():
    assert torch.cuda.is_available(), "this test needs the MI355X"


def t(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def ptr(x):
    return None if x is None else x.data_ptr()


def workspace(lib, n, K, D):
    need = int(lib.fr_vq_workspace_bytes(n, K, D, 1))
    assert need > 0
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)  # (nothing may be read that the call did not write)
    assert ws.data_ptr() % 16 == 0
    return ws


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def update(feats, weights, rows, ind, embed, cs, decay, eps=C.EPS):
    """fr_vq_update on numpy inputs -> (embed, cluster_size) as numpy"""
    lib = _native.load()
    n, (K, D) = ind.shape[0], embed.shape
    f, w, r, i, e, s = t(feats), t(weights), t(rows), t(ind), t(embed), t(cs)
    assert i.dtype == torch.int32 and f.shape[1] == D and (r is None or r.shape[0] == n) and (r is not None or f.shape[0] == n)
    ws = workspace(lib, n, K, D)
    with torch.cuda.device(DEV):
        rc = lib.fr_vq_update(n, K, D, f.data_ptr(), f.shape[0], ptr(r), int(r is not None and r.dtype == torch.int64), ptr(w), i.data_ptr(),
                              float(decay), float(eps), e.data_ptr(), s.data_ptr(), ws.data_ptr(), stream())
    assert rc == 0, lib.fr_last_error()
    return e.cpu().numpy(), s.cpu().numpy()


def update_case(I, decay):
    return update(I["feats"], I["weights"], I["rows"], I["ind"], I["embed"], I["cs"], decay)


# ---- judge 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", (True, False), ids=("weighted", "unweighted"))
@pytest.mark.parametrize("c", C.EXACT, **ids)
def test_exact_cases_bit_for_bit(c, weighted):
    _need_gpu()
    I = C.inputs(c, "exact", weighted)
    for decay in (C.DECAY, 0.0):
        e, cs = update_case(I, decay)
        C.judge_exact(e, cs, I, decay)


# ---- judges 2 and 3 ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def general_step(c):
    return update_case(C.inputs(c, "general"), C.DECAY)


@pytest.mark.parametrize("c", C.GENERAL, **ids)
def test_general_data_within_the_derived_bounds_of_float64(c):
    _need_gpu()
    e, cs = general_step(c)
    C.judge_general(e, cs, C.inputs(c, "general"), f"step {C.case_id(c)}")


@pytest.mark.parametrize("c", C.GENERAL, **ids)
def test_general_data_in_ascending_row_order_bit_for_bit(c):
    _need_gpu()
    e, cs = general_step(c)
    C.judge_order(e, cs, C.inputs(c, "general"))


def test_a_segment_that_absorbs_its_small_rows_sums_to_two_to_the_24():
    _need_gpu()
    x, ind, e0, cs0 = C.absorbing_segment()
    e, cs = update(x, None, None, ind, e0, cs0, 0.0, 0.0)
    assert cs[1] == 256.0 and np.array_equal(cs, np.bincount(ind, minlength=3))
    assert e[1, 0] == 65536.0, float(e[1, 0])  # = 2^24 / 256; any other order gives at least 65536 + 2^-7


# ---- replacement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n,k", C.REPLACE)
def test_replacement_with_ties_across_strides(K, n, k):
    _need_gpu()
    R = C.replace_inputs(K, n, k)
    lib = _native.load()
    D = R["embed"].shape[1]
    f, w, cs = t(R["feats"]), t(R["weights"]), t(R["cs"])
    got = []
    for dt in (torch.int64, torch.int32):
        r, e = t(R["rows"]).to(dt), t(R["embed"])
        ws = workspace(lib, n, K, D)
        with torch.cuda.device(DEV):
            rc = lib.fr_vq_replace(n, K, D, k, f.data_ptr(), f.shape[0], r.data_ptr(), int(dt == torch.int64), w.data_ptr(), e.data_ptr(),
                                   cs.data_ptr(), ws.data_ptr(), stream())
        assert rc == 0, lib.fr_last_error()
        C.judge_replace(e.cpu().numpy(), cs.cpu().numpy(), R)
        got.append(e)
    assert torch.equal(got[0], got[1])


# ---- loss --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,D,rows", C.LOSS)
def test_loss_against_float64(n, K, D, rows):
    _need_gpu()
    g = np.random.default_rng([n, K, D])
    N = n if rows is None else n + n // 2
    feats, embed = g.standard_normal((N, D)).astype(np.float32), g.standard_normal((K, D)).astype(np.float32)
    r = None if rows is None else g.integers(0, N, n).astype(rows)
    ind = g.integers(0, K, n).astype(np.int32)
    lib = _native.load()
    f, rt, e, i = t(feats), t(r), t(embed), t(ind)
    loss = torch.full((1,), float("nan"), device=DEV)
    ws = workspace(lib, n, K, D)
    with torch.cuda.device(DEV):
        rc = lib.fr_vq_gather(n, K, D, f.data_ptr(), N, ptr(rt), int(r is not None), e.data_ptr(), i.data_ptr(), 0, None, None, loss.data_ptr(),
                              1.0, ws.data_ptr(), stream())
    assert rc == 0, lib.fr_last_error()
    share = C.judge_loss(loss.cpu().numpy()[0], feats if r is None else feats[r], embed, ind, D)
    print(f"loss n={n} K={K} D={D}: {share:.3f} of the bound")
    parity_report.record("vq", f"step loss n={n} K={K} D={D}", loss_ratio_to_bound=share)


# ---- through the module --------------------------------------------------------------------------------------------------------
def _module(codes, cs0):
    K, D = codes.shape
    m = vectree.VectorQuantize(dim=D, codebook_size=K, decay=C.DECAY, commitment_weight=1.0, use_cosine_sim=False, threshold_ema_dead_code=0,
                               codebook=torch.from_numpy(codes.copy())).to(DEV)
    m._codebook.cluster_size.copy_(t(cs0)[None])
    return m.train()


def _emulated_iteration(pool, imp, rows, ind, e, cs, name):
    """One iteration of the loop restated: the kernel's assignment, held to the derived rule, handed to the emulation and the replacement"""
    x, w = pool[rows], imp[rows]
    share = vq_ref.check_assignment(ind, x, e, 0.02)
    parity_report.record("vq", name, ambiguous_share=share, cap=0.02)
    r = vq_ref.emulate_update(x, w, ind, e, cs, C.DECAY, C.EPS)
    return vq_ref.replace(r["embed"], r["cluster_size"], x, w, K_EXPIRE)[0], r["cluster_size"]


MODULE = ((4097, 257, 27), (5000, 1025, 48))


def _loop_inputs(n, K, D):
    pool, imp, codes = C.sh_like(n, K, D, 1)
    g = np.random.default_rng([n, K, D, 2])
    return pool, imp, codes, g.uniform(0.0, 2.0 * n / K, K).astype(np.float32), g.integers(0, pool.shape[0], (3, n))


@pytest.mark.parametrize("n,K,D", MODULE)
def test_module_step_equals_the_emulation_and_the_replacement(n, K, D):
    _need_gpu()
    pool, imp, codes, cs0, indexes = _loop_inputs(n, K, D)
    m = _module(codes, cs0)
    q, ind, loss = m.step(t(pool), t(imp), t(indexes[0]), k_expire=K_EXPIRE)
    assert q is None and ind.dtype == torch.int32 and tuple(ind.shape) == (n,)
    ind = ind.cpu().numpy()
    e, cs = _emulated_iteration(pool, imp, indexes[0], ind, codes, cs0, f"module step n={n} K={K} D={D}")
    C.same_bits(m._codebook.cluster_size[0].cpu().numpy(), cs, "cluster_size")
    C.same_bits(m._codebook.embed[0].cpu().numpy(), e, "embed")
    C.judge_loss(loss.cpu().numpy()[0], pool[indexes[0]], codes, ind, D)


@pytest.mark.parametrize("n,K,D", MODULE)
def test_three_loop_iterations_equal_the_emulation(n, K, D):
    """The assignment of every iteration is the kernel's on the emulated state, which equals the module's bit for bit"""
    _need_gpu()
    pool, imp, codes, cs0, indexes = _loop_inputs(n, K, D)
    m = _module(codes, cs0)
    losses = vectree.train_codebook(t(pool), t(imp), m, k_expire=K_EXPIRE, indexes=t(indexes))
    e, cs = codes, cs0
    for it in range(3):
        ind = vectree.nearest_code(t(pool), t(e), rows=t(indexes[it])).cpu().numpy()
        C.judge_loss(losses[it].cpu().numpy(), pool[indexes[it]], e, ind, D)
        e, cs = _emulated_iteration(pool, imp, indexes[it], ind, e, cs, f"loop iteration {it} n={n} K={K} D={D}")
    C.same_bits(m._codebook.cluster_size[0].cpu().numpy(), cs, "cluster_size")
    C.same_bits(m._codebook.embed[0].cpu().numpy(), e, "embed")
