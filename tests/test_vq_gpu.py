"""VecTree vector quantisation on the MI355X (csrc/vq.hip, fov3dgs_amd.vectree).

The assignment is judged by a rule that is derived, not measured (tests/vq_ref.py): with d^2 the float64 squared distances and
B_i = 2 (D + 2) 2^-24 (||x_i|| + max_c ||e_c||)^2 -- what a (D+1)-term fp32 fmaf chain can do to the difference of two scores -- a row
is ambiguous when its second-best d^2 lies within B_i of its best. On every other row the kernel's index must EQUAL the float64
argmin; on an ambiguous row it must be one of the codes within B_i. The ambiguous share is capped (2 % on the random inputs, 20 % on
the one ill-conditioned input, data and codes offset by +20) so that the rule cannot pass vacuously.

The step is compared with the float64 restatement; the tolerance of each quantity is FOUR TIMES the distance of the reference's own
float32 output to that restatement on the same fixture (tests/golden/ref_vq.npz err_*, measured on the CPU by make_vq_golden.py;
times 4 for the different summation order). Those distances, largest over D = 48 / 27 and the weighted / unweighted step, and in
brackets what the kernels gave on the MI355X:
  embed 2.8e-7 (allowed 1.1e-6; got <= 1.8e-7), cluster_size 1.06e-6 (allowed 4.2e-6; got <= 3.0e-6, against 3.2e-6 allowed for that
  fixture), quantize 6.0e-8 (allowed 2.4e-7; got 0: the reference returns x + (q - x), here q itself), loss 5.4e-9 (allowed 2.1e-8; got
  <= 3.6e-9); after three loop iterations embed 2.5e-7 (got <= 3.0e-7), cluster_size 8.6e-7 (got <= 9.2e-7), loss 9.1e-9 (got <= 4.8e-9).
Each test uses the figure of its own fixture, not the largest."""
import functools
import os

import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import vectree
from fov3dgs_amd import vq as vq_dropin
from tests import parity_report, vq_ref
from tests.helpers import small_camera, small_cloud

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_EXPIRE = 10


def _need_gpu():
    assert torch.cuda.is_available(), "this test needs the MI355X"


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_vq.npz")))


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def close(got, want, err, what):
    d = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))))
    print(f"{what}: distance {d:.3e}, reference's own {err:.3e}, allowed {4 * err:.3e}")
    parity_report.record("vq", what, distance_to_float64=d, reference_own_distance=err, allowed=4 * err)
    assert d <= 4 * err, (what, d, 4 * err)


# ---- search ----------------------------------------------------------------------------------------------------------------
def _data(kind, n, K, D, seed):
    g = torch.Generator().manual_seed(seed)
    if kind in ("normal", "offset"):  # offset: the ill-conditioned input, ||x|| and ||e|| far above the distances between them
        off = 20.0 if kind == "offset" else 0.0
        return torch.randn(n, D, generator=g) + off, torch.randn(K, D, generator=g) + off
    x = torch.randn(n, D, generator=g) * 0.3  # SH-like: the codes are perturbed rows (K <= n of them, each row at most once)
    x[:, :min(3, D)] += 0.8
    return x, x[torch.randperm(n, generator=g)[:K]] + 0.05 * torch.randn(K, D, generator=g)


SEARCH = [(n, K, D) for n, K, D in ((1, 1, 1), (63, 10, 3), (64, 33, 27), (65, 256, 48), (1000, 1000, 64), (4099, 256, 27), (4099, 1000, 48),
                                    (1000, 33, 1), (63, 1, 64), (1, 1000, 48), (65, 128, 3), (64, 10, 64), (1000, 129, 3))]
CASES = [("normal",) + c for c in SEARCH] + [("sh",) + c for c in SEARCH if c[1] <= c[0] and c[2] >= 3]


@pytest.mark.parametrize("kind,n,K,D", CASES)
def test_search_follows_the_derived_rule(kind, n, K, D):
    _need_gpu()
    x, e = _data(kind, n, K, D, 1000 * n + K + D)
    ind, dist = vectree.nearest_code(t(x), t(e), return_distance=True)
    assert ind.dtype == torch.int32 and tuple(ind.shape) == (n,)
    vq_ref.check_assignment(ind.cpu().numpy(), x.numpy(), e.numpy(), 0.02)
    # the returned distance: fp32 rounding of D squared differences and their sum around the float64 value
    d2 = vq_ref.sq_dists(x.numpy(), e.numpy())[np.arange(n), ind.cpu().numpy()]
    want = np.sqrt(d2)
    tol = (D + 4) * 2.0 ** -24 * (np.linalg.norm(x.numpy().astype(np.float64), axis=1) + np.linalg.norm(e.numpy().astype(np.float64), axis=1).max()) ** 2
    assert (np.abs(dist.cpu().numpy().astype(np.float64) ** 2 - d2) <= tol + 1e-30).all()
    assert (np.abs(dist.cpu().numpy() - want) <= np.sqrt(tol) + 1e-6 * want).all()  # |sqrt a - sqrt b| <= sqrt |a - b|, and the root's own rounding


@pytest.mark.parametrize("n,K,D", ((4099, 256, 48), (1000, 1000, 27), (65, 33, 3)))
def test_search_on_the_ill_conditioned_input(n, K, D):
    _need_gpu()
    x, e = _data("offset", n, K, D, n + K + D)
    share = vq_ref.check_assignment(vectree.nearest_code(t(x), t(e)).cpu().numpy(), x.numpy(), e.numpy(), 0.20)
    parity_report.record("vq", f"search, offset input n={n} K={K} D={D}", ambiguous_share=share, cap=0.20)


def test_search_ties_exact_rows_and_indirection():
    _need_gpu()
    g = torch.Generator().manual_seed(7)
    n, K, D = 1000, 256, 48
    x, base = torch.randn(n, D, generator=g), torch.randn(K // 2, D, generator=g)
    # every code twice (c and c + K/2, and once more next to each other): the lowest index wins on every row
    e = torch.cat([base, base])
    ind = vectree.nearest_code(t(x), t(e)).cpu().numpy()
    assert (ind < K // 2).all()
    vq_ref.check_assignment(ind, x.numpy(), base.numpy(), 0.02)
    e2 = base.repeat_interleave(2, dim=0)
    assert np.array_equal(vectree.nearest_code(t(x), t(e2)).cpu().numpy(), 2 * ind)  # (equal codes have equal scores, bit for bit)
    # rows that equal a code exactly take it (its first copy), at distance 0
    pick = torch.randint(0, K // 2, (n,), generator=g)
    ind, dist = vectree.nearest_code(t(base[pick]), t(e), return_distance=True)
    assert torch.equal(ind.cpu().long(), pick) and not dist.any()
    # rows= equals the materialised gather bit for bit, int32 and int64, repeats included; [1,K,D] codebooks are taken
    rows = torch.randint(0, n, (4099,), generator=g)
    want = vectree.nearest_code(t(x[rows]), t(e))
    for dt in (torch.int64, torch.int32):
        got, dist = vectree.nearest_code(t(x), t(e)[None], rows=t(rows.to(dt)), return_distance=True)
        assert torch.equal(got, want)
        assert torch.equal(dist, vectree.nearest_code(t(x[rows]), t(e), return_distance=True)[1])
    assert vectree.nearest_code(t(x[:0]), t(e)).shape == (0,)
    with pytest.raises(ValueError):
        vectree.nearest_code(t(x), t(e[:, :40]))


# ---- the step --------------------------------------------------------------------------------------------------------------
def _module(D, embed0, cs0, K=64):
    m = vq_dropin.VectorQuantize(dim=D, codebook_size=K, decay=0.8, commitment_weight=1.0, use_cosine_sim=False, threshold_ema_dead_code=0,
                                 codebook=torch.from_numpy(embed0)).to(DEV)
    m._codebook.cluster_size.copy_(t(cs0)[None])
    return m


@pytest.mark.parametrize("D", (48, 27))
@pytest.mark.parametrize("tag", ("aw_", "au_"))
def test_training_step_against_the_fixture(D, tag):
    _need_gpu()
    G, p = gold(), f"{D}_"
    x, w, e0, cs0 = G[p + "x"], G[p + "w"] if tag == "aw_" else None, G[p + "embed0"], G[p + "cs0"]
    m = _module(D, e0, cs0).train()
    q, ind, loss = m(t(x)[None], weight=None if w is None else t(w).reshape(1, -1, 1))
    assert tuple(q.shape) == (1, 500, D) and ind.dtype == torch.int64 and tuple(ind.shape) == (1, 500) and tuple(loss.shape) == (1,)
    assert np.array_equal(ind[0].cpu().numpy(), G[p + tag + "ind"])
    r = vq_ref.train_step(x, w, e0, cs0, G[p + tag + "ind"])
    got = dict(embed=m._codebook.embed[0], cluster_size=m._codebook.cluster_size[0], quantize=q[0], loss=loss)
    for name, v in got.items():
        close(v.cpu().numpy(), r[name], float(G["err_" + p + tag + name]), p + tag + name)
    assert torch.equal(q[0], t(e0)[ind[0]])  # gathered from the codebook BEFORE the update
    # a code with no member decays by exactly 0.8
    empty = np.bincount(G[p + tag + "ind"], minlength=64) == 0
    assert empty.sum() >= 2
    assert torch.equal(m._codebook.embed[0][t(empty)], t(e0)[t(empty)] * 0.8)


@pytest.mark.parametrize("D", (48, 27))
def test_eval_changes_no_state(D):
    _need_gpu()
    G, p = gold(), f"{D}_"
    m = _module(D, G[p + "embed0"], G[p + "cs0"]).eval()
    q, ind, loss = m(t(G[p + "x"])[None])
    assert np.array_equal(ind[0].cpu().numpy(), G[p + "c_ind"])
    assert np.array_equal(q[0].cpu().numpy(), G[p + "c_quantize"]) and loss.cpu().tolist() == G[p + "c_loss"].tolist() == [0.0]
    assert torch.equal(m._codebook.embed[0], t(G[p + "embed0"])) and torch.equal(m._codebook.cluster_size[0], t(G[p + "cs0"]))
    q2, ind2, _ = m(t(G[p + "x"]))  # [n, D] as the reference also takes it
    assert torch.equal(q2, q[0]) and torch.equal(ind2, ind[0])


# ---- the loop and its replacement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (48, 27))
def test_loop_with_replacement_against_the_fixture(D):
    _need_gpu()
    G, p = gold(), f"{D}_"
    pool, imp, indexes = t(G[p + "pool"]), t(G[p + "imp"]), t(G[p + "indexes"])
    m = _module(D, G[p + "embed0"], G[p + "cs0"])
    # the restatement, replayed in float64 with the fixture's (asserted unambiguous) assignments left to its own argmin
    e, cs, l64 = G[p + "embed0"].astype(np.float64), G[p + "cs0"].astype(np.float64), []
    for it in range(3):
        idx = G[p + "indexes"][it]
        r = vq_ref.train_step(G[p + "pool"][idx], G[p + "imp"][idx], e, cs)
        e, codes, rows = vq_ref.replace(r["embed"], r["cluster_size"], G[p + "pool"][idx], G[p + "imp"][idx], K_EXPIRE)
        cs = r["cluster_size"]
        l64.append(r["loss"])
    losses = vectree.train_codebook(pool, imp, m, k_expire=K_EXPIRE, indexes=indexes)
    assert m.training  # (the mode it was in is restored)
    close(m._codebook.embed[0].cpu().numpy(), e, float(G["err_" + p + "b_embed"]), p + "b_embed")
    close(m._codebook.cluster_size[0].cpu().numpy(), cs, float(G["err_" + p + "b_cluster_size"]), p + "b_cluster_size")
    close(losses.cpu().numpy(), l64, float(G["err_" + p + "b_loss"]), p + "b_loss")
    # the rows the last iteration wrote are the sampled rows, bit for bit
    idx = G[p + "indexes"][2]
    assert torch.equal(m._codebook.embed[0][t(G[p + "b_codes"][2]).long()], pool[t(idx[G[p + "b_rows"][2]])])
    assert np.array_equal(codes, G[p + "b_codes"][2]) and np.array_equal(rows, G[p + "b_rows"][2])
    # int32 indexes give the same bits
    m2 = _module(D, G[p + "embed0"], G[p + "cs0"])
    vectree.train_codebook(pool, imp, m2, k_expire=K_EXPIRE, indexes=indexes.to(torch.int32))
    assert torch.equal(m2._codebook.embed, m._codebook.embed) and torch.equal(m2._codebook.cluster_size, m._codebook.cluster_size)


def test_replacement_ties_and_k_above_K():
    _need_gpu()
    g = torch.Generator().manual_seed(3)
    n, K, D = 300, 8, 27
    x, e0 = torch.randn(n, D, generator=g), torch.randn(K, D, generator=g)
    # k > K replaces nothing (vectree.py:194-195): the codebook equals the plain step's
    a, b = _module(D, e0.numpy(), np.ones(K, np.float32), K), _module(D, e0.numpy(), np.ones(K, np.float32), K)
    vectree.train_codebook(t(x), None, a, k_expire=10, indexes=torch.arange(n, device=DEV)[None])
    b(t(x)[None])
    assert torch.equal(a._codebook.embed, b._codebook.embed) and torch.equal(a._codebook.cluster_size, b._codebook.cluster_size)
    # ties: three far codes take no member from cluster_size 0 -> all three end at 0 and tie; weights tie in pairs. Lowest index first.
    e1 = e0.clone()
    e1[[1, 4, 6]] += 100.0
    w = torch.ones(n)
    w[[250, 17, 99]] = 5.0  # the three largest, tied: positions 17, 99, 250 in that order
    c = _module(D, e1.numpy(), np.zeros(K, np.float32), K)
    vectree.train_codebook(t(x), t(w), c, k_expire=3, indexes=torch.arange(n, device=DEV)[None])
    assert torch.equal(c._codebook.embed[0][[1, 4, 6]], t(x)[[17, 99, 250]])
    assert not c._codebook.cluster_size[0][[1, 4, 6]].any()


# ---- determinism, no synchronisation ---------------------------------------------------------------------------------------
def test_twenty_iterations_are_deterministic_and_never_synchronise():
    _need_gpu()
    g = torch.Generator().manual_seed(9)
    N, n, K, D = 6000, 4099, 256, 48
    pool, e0 = _data("sh", N, K, D, 5)
    imp = t(torch.rand(N, generator=g) ** 3 * 10 + 1e-3)
    indexes = t(torch.randint(0, N, (20, n), generator=g))
    pool = t(pool)
    books = []
    for run in range(2):
        # (modules and generators are made outside the checked region: a host-to-device copy of pageable memory synchronises)
        m, m2 = (_module(D, e0.numpy(), np.zeros(K, np.float32), K) for _ in range(2))
        gen = torch.Generator(device=DEV).manual_seed(1)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            losses = vectree.train_codebook(pool, imp, m, k_expire=K_EXPIRE, indexes=indexes)
            drawn = vectree.train_codebook(pool, imp, m2, iterations=2, chunk=n, k_expire=K_EXPIRE, generator=gen)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        books.append((m._codebook.embed.clone(), m._codebook.cluster_size.clone(), losses.clone(), drawn.clone()))
    for a, b in zip(*books):
        assert torch.equal(a, b)
    assert torch.isfinite(books[0][0]).all() and torch.isfinite(books[0][2]).all() and (books[0][2] > 0).all()


# ---- bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (1, 4, 13, 16))
def test_bits_equal_np_packbits(bits):
    _need_gpu()
    for count in (1, 7, 8, 9, 1001):
        g = torch.Generator().manual_seed(bits * 1000 + count)
        v = torch.randint(0, 2 ** bits, (count,), generator=g)
        v[0] = 2 ** bits - 1
        mask = 2 ** torch.arange(bits - 1, -1, -1)
        want = np.packbits(v.unsqueeze(-1).bitwise_and(mask).ne(0).numpy().reshape(-1))  # the reference's dec2bin, then np.packbits
        for dt in (torch.int64, torch.int32):
            got = vectree.pack_bits(t(v.to(dt)), bits)
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
        back = vectree.unpack_bits(got, count, bits)
        assert back.dtype == torch.int32 and torch.equal(back.cpu().long(), v)


# ---- end to end ------------------------------------------------------------------------------------------------------------
class Pipe:
    debug = False
    compute_cov3D_python = False
    convert_SHs_python = False


def test_quantize_model_end_to_end(tmp_path):
    _need_gpu()
    from fov3dgs_amd.gaussian_renderer import render
    cloud = small_cloud(3000, 3, 0.1)
    g = torch.Generator().manual_seed(2)
    imp = torch.rand(3000, generator=g) ** 2
    folder = str(tmp_path / "extreme_saving")
    out = vectree.quantize_model(cloud, imp, folder=folder, codebook_size=64, iterations=5, chunk=1000, generator=torch.Generator(device=DEV).manual_seed(4))
    mask, ind, table = out["non_vq_mask"], out["all_indice"], out["table"]
    assert int(mask.sum()) == int(3000 * (1 - 0.6)) and ind.dtype == torch.int64 and tuple(table.shape) == (3000, 62)
    cb = out["vq"]._codebook.embed[0]
    vq_ref.check_assignment(ind.cpu().numpy(), table[:, 6:54].cpu().numpy(), cb.cpu().numpy(), 0.02)
    assert torch.equal(out["all_feat"], cb[ind].half().float())
    full = vectree.load_vq(folder, device=DEV)
    assert tuple(full.shape) == (3000, 62)
    assert torch.equal(full[:, 0:3], table[:, 0:3]) and not full[:, 3:6].any()                # xyz exact, normals zero
    assert torch.equal(full[mask, 6:54], table[mask, 6:54].half().float())                    # non-VQ rows: their own SH through fp16
    assert torch.equal(full[~mask, 6:54], cb.half().float()[ind[~mask]])                      # VQ rows: codebook.half()[ind]
    assert torch.equal(full[:, -8:], table[:, -8:].half().float())
    assert torch.equal(full.cpu(), vectree.load_vq(folder))                                   # the CPU decoder gives the same table
    # the decoded model renders
    decoded = vectree.cloud_from_table(full, 3)
    assert torch.equal(vectree.feature_table(decoded), full)
    cam = small_camera(200, 120).to(DEV)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    with torch.no_grad():
        img = render(cam, decoded, Pipe(), bg, cuda_type="original")["render"]
    assert tuple(img.shape) == (3, 120, 200) and torch.isfinite(img).all()
    assert float((img - bg[:, None, None]).abs().max()) > 0.05  # (something other than the background was drawn)
