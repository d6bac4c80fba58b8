"""VecTree vector quantisation, what can be checked without a GPU: the float64 restatement (tests/vq_ref.py) against the reference's
recorded float32 outputs (tests/golden/ref_vq.npz, made by tests/golden/make_vq_golden.py), the container against the reference's
decoder, the bit packing, the tie rules, the refusals, the new exports.

Tolerance of the restatement: the fixture records, per quantity, the distance of the reference's float32 output to the restatement
(err_*; largest over both D: embed 2.8e-7, cluster_size 1.06e-6, quantize 6.0e-8, loss 9.1e-9) -- here the two are compared with
exactly that figure (it is the same comparison, so it must reproduce), and with the reference's float32 resolution as a sanity bound."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native, vectree
from tests import vq_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fr_vq_workspace_bytes", "fr_vq_nearest", "fr_vq_gather", "fr_vq_update", "fr_vq_replace", "fr_pack_bits", "fr_unpack_bits")
K_EXPIRE = 10


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_vq.npz")))


def close(got, want, err):
    d = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))))
    assert d <= err * (1 + 1e-9) + 1e-300, (d, err)
    return d


@pytest.mark.parametrize("D", (48, 27))
@pytest.mark.parametrize("tag", ("aw_", "au_"))
def test_restatement_reproduces_a_training_step(gold, D, tag):
    p = f"{D}_"
    x, w, e0, cs0 = gold[p + "x"], gold[p + "w"] if tag == "aw_" else None, gold[p + "embed0"], gold[p + "cs0"]
    ind, amb, _, _ = vq_ref.assignment(x, e0)
    assert not amb.any() and np.array_equal(ind, gold[p + tag + "ind"])
    r = vq_ref.train_step(x, w, e0, cs0)
    for name in ("embed", "cluster_size", "quantize", "loss"):
        e = float(gold["err_" + p + tag + name])
        assert e <= 2e-6, (name, e)  # a few float32 ulps of values of order 1 .. 16
        close(r[name], gold[p + tag + name], e)
    # a code with no member decays by exactly the decay
    empty = np.bincount(ind, minlength=e0.shape[0]) == 0
    assert empty.any()
    assert np.array_equal(r["embed"][empty], 0.8 * e0[empty].astype(np.float64))


@pytest.mark.parametrize("D", (48, 27))
def test_restatement_reproduces_the_loop_and_eval(gold, D):
    p = f"{D}_"
    e, cs = gold[p + "embed0"].astype(np.float64), gold[p + "cs0"].astype(np.float64)
    losses = []
    for it in range(3):
        idx = gold[p + "indexes"][it]
        x, w = gold[p + "pool"][idx], gold[p + "imp"][idx]
        assert not vq_ref.assignment(x, e)[1].any()
        r = vq_ref.train_step(x, w, e, cs)
        e, codes, rows = vq_ref.replace(r["embed"], r["cluster_size"], x, w, K_EXPIRE)
        cs = r["cluster_size"]
        assert np.array_equal(codes, gold[p + "b_codes"][it]) and np.array_equal(rows, gold[p + "b_rows"][it])
        assert np.array_equal(e[codes], x[rows].astype(np.float64))
        losses.append(r["loss"])
    close(e, gold[p + "b_embed"], float(gold["err_" + p + "b_embed"]))
    close(cs, gold[p + "b_cluster_size"], float(gold["err_" + p + "b_cluster_size"]))
    close(losses, gold[p + "b_loss"], float(gold["err_" + p + "b_loss"]))
    # eval: the assignment and the gather alone
    ind = vq_ref.assignment(gold[p + "x"], gold[p + "embed0"])[0]
    assert np.array_equal(ind, gold[p + "c_ind"]) and np.array_equal(gold[p + "embed0"][ind], gold[p + "c_quantize"])
    assert gold[p + "c_loss"].tolist() == [0.0]
    # k > K replaces nothing
    e2, codes, rows = vq_ref.replace(e, cs, x, w, e.shape[0] + 1)
    assert codes.size == 0 and rows.size == 0 and np.array_equal(e2, e)


def test_load_vq_equals_the_references_decoder_bit_for_bit(gold, tmp_path):
    for name in vectree.FILES:
        (tmp_path / name).write_bytes(gold["d_file_" + name[:-4]].tobytes())
    got = vectree.load_vq(str(tmp_path), device="cpu")
    assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.uint32), gold["d_decoded"].view(np.uint32))


def test_save_load_round_trip(gold, tmp_path):
    table, mask = torch.from_numpy(gold["d_table"]), torch.from_numpy(gold["d_mask"])
    ind, cb = torch.from_numpy(gold["d_indice"]).long(), torch.from_numpy(gold["d_codebook"])
    D = cb.shape[1]
    folder = vectree.save_vq(str(tmp_path / "extreme_saving"), table, mask, ind, cb[None], D)
    assert sorted(os.listdir(folder)) == sorted(vectree.FILES)
    full = vectree.load_vq(folder)
    assert np.array_equal(full.numpy().view(np.uint32), gold["d_decoded"].view(np.uint32))  # (what the reference decoded from the same input)
    assert torch.equal(full[:, 0:3], table[:, 0:3]) and not full[:, 3:6].any() and not full[:, 6 + D:-8].any()
    assert torch.equal(full[:, -8:], table[:, -8:].half().float())
    assert torch.equal(full[mask, 6:6 + D], table[mask, 6:6 + D].half().float())
    assert torch.equal(full[~mask, 6:6 + D], cb.half().float()[ind[~mask]])
    meta = np.load(os.path.join(folder, "metadata.npz"), allow_pickle=True)["metadata"].item()
    assert meta == dict(input_pc_num=203, input_pc_dim=62, codebook_size=16, codebook_dim=27)
    assert np.load(os.path.join(folder, "codebook.npz"))["arr_0"].dtype == np.float16
    assert np.load(os.path.join(folder, "xyz.npz"))["arr_0"].dtype == np.float32
    # vq_way other than "half" keeps float32
    folder = vectree.save_vq(str(tmp_path / "full"), table, mask, ind, cb, D, vq_way="full")
    assert torch.equal(vectree.load_vq(folder)[:, -8:], table[:, -8:])
    with pytest.raises(ValueError, match="power-of-two"):
        vectree.save_vq(str(tmp_path / "bad"), table, mask, ind.clamp(max=9), cb[:10], D)


@pytest.mark.parametrize("bits", (1, 4, 13, 16))
@pytest.mark.parametrize("count", (1, 7, 8, 9, 1001))
def test_bits_on_the_cpu(bits, count):
    g = torch.Generator().manual_seed(bits * 1000 + count)
    v = torch.randint(0, 2 ** bits, (count,), generator=g)
    v[0] = 2 ** bits - 1
    # the reference's dec2bin (a float matrix) and np.packbits, restated
    mask = 2 ** torch.arange(bits - 1, -1, -1)
    want = np.packbits(v.unsqueeze(-1).bitwise_and(mask).ne(0).numpy().reshape(-1))
    got = vectree.pack_bits(v, bits)
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want) and np.array_equal(vq_ref.pack_bits(v.numpy(), bits), want)
    back = vectree.unpack_bits(got, count, bits)
    assert back.dtype == torch.int32 and torch.equal(back.long(), v)
    with pytest.raises(ValueError):
        vectree.unpack_bits(got[:-1], count, bits)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="bits"):
            vectree.pack_bits(v, bad)


def test_select_non_vq_tie_rules():
    imp = torch.tensor([1.0, 5.0, 5.0, 0.5, 5.0, 2.0, 2.0, 0.0, 5.0, 2.0])
    # int(10 * (1 - 0.6)) = 4 (Python floats as the reference writes them): the four 5.0
    assert vectree.select_non_vq(imp, 0.6).tolist() == [False, True, True, False, True, False, False, False, True, False]
    # three of the four tied 5.0: the lowest indices
    assert torch.nonzero(vectree.select_non_vq(imp, 0.7)).flatten().tolist() == [1, 2, 4]
    # 4 x 5.0 and two of the three 2.0: the lowest indices again
    assert torch.nonzero(vectree.select_non_vq(imp, 0.4)).flatten().tolist() == [1, 2, 4, 5, 6, 8]
    assert not vectree.select_non_vq(imp, 1.0).any() and vectree.select_non_vq(imp, 0.0).all()
    assert vectree.select_non_vq(np.ones(7), 0.5).tolist() == [True, True, True, False, False, False, False]
    for n in (1, 7, 1161358):
        assert int(vectree.select_non_vq(torch.ones(n), 0.6).sum()) == int(n * (1 - 0.6))
    with pytest.raises(ValueError):
        vectree.select_non_vq(imp, 1.5)


def test_refused_configurations_raise():
    ok = dict(dim=48, codebook_size=64, decay=0.8, commitment_weight=1.0, use_cosine_sim=False, threshold_ema_dead_code=0)
    m = vectree.VectorQuantize(**ok)
    assert tuple(m._codebook.embed.shape) == (1, 64, 48) and tuple(m._codebook.cluster_size.shape) == (1, 64)
    assert tuple(m.codebook.shape) == (64, 48) and m.codebook_size == 64 and m.training
    assert 0 < float(m.codebook.abs().max()) <= (6.0 / (64 * 48)) ** 0.5 + 1e-7  # kaiming_uniform_(a=0) on [1,K,D]: sqrt(6 / (K D))
    assert not m.eval().training
    for bad in (dict(use_cosine_sim=True), dict(heads=2), dict(codebook_dim=32), dict(kmeans_init=True), dict(threshold_ema_dead_code=2),
                dict(sample_codebook_temp=0.5), dict(orthogonal_reg_weight=0.1), dict(separate_codebook_per_head=True),
                dict(accept_image_fmap=True), dict(channel_last=False), dict(sync_codebook=True), dict(dim=65), dict(dim=0),
                dict(codebook_size=0), dict(codebook_size=65537), dict(decay=1.5), dict(codebook=torch.zeros(3, 48))):
        with pytest.raises(ValueError):
            vectree.VectorQuantize(**{**ok, **bad})
    given = torch.randn(64, 48)
    assert torch.equal(vectree.VectorQuantize(**ok, codebook=given).codebook, given)
    # the device paths have no CPU fallback
    x = torch.randn(10, 48)
    for call in (lambda: vectree.nearest_code(x, given), lambda: m(x[None]), lambda: vectree.assign_all(x, m),
                 lambda: vectree.train_codebook(x, None, m, iterations=1, chunk=4)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_header_library_and_exports_carry_the_new_symbols(tmp_path):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fovraster.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fr_[a-z_0-9A-Z]+)\s*\(", txt))
    lib = _native.load()
    for n in NEW:
        assert n in declared and n in _native.EXPORTS and hasattr(lib, n), n
    assert lib.fr_abi_version() == _native.ABI_VERSION == 12  # (symbols are added; no struct changed)
    src = tmp_path / "h.c"
    src.write_text('#include "fovraster.h"\n'
                   "int (*const search)(int64_t, int32_t, int32_t, const float *, int64_t, const void *, int32_t, const float *, int32_t *, void *,"
                   " void *) = fr_vq_nearest;\n"
                   "int (*const pack)(int64_t, int32_t, const int32_t *, uint8_t *, void *) = fr_pack_bits;\n"
                   "int main(void) { return FR_ABI_VERSION != 12; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_native_refuses_bad_arguments_without_launching():
    lib = _native.load()
    p = 4096  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails validation first

    def bad(rc, *words):
        assert rc == -1 and all(w in lib.fr_last_error() for w in words), (rc, lib.fr_last_error())
    assert lib.fr_vq_workspace_bytes(100, 0, 48, 0) == 0 and lib.fr_vq_workspace_bytes(100, 64, 65, 1) == 0
    assert lib.fr_vq_workspace_bytes(80000, 8192, 48, 1) > lib.fr_vq_workspace_bytes(80000, 8192, 48, 0) > 80000 * 4
    bad(lib.fr_vq_nearest(10, 0, 48, p, 10, None, 0, p, p, p, None), b"K=0")
    bad(lib.fr_vq_nearest(10, 65537, 48, p, 10, None, 0, p, p, p, None), b"K=65537")
    bad(lib.fr_vq_nearest(10, 64, 65, p, 10, None, 0, p, p, p, None), b"D=65")
    bad(lib.fr_vq_nearest(-1, 64, 48, p, 10, None, 0, p, p, p, None), b"n=-1")
    bad(lib.fr_vq_nearest(10, 64, 48, p, 9, None, 0, p, p, p, None), b"N=9")
    bad(lib.fr_vq_nearest(10, 64, 48, p, 0, p, 0, p, p, p, None), b"N=0")
    bad(lib.fr_vq_nearest(10, 64, 48, None, 10, None, 0, p, p, p, None), b"null")
    bad(lib.fr_vq_nearest(10, 64, 48, p, 10, None, 0, p, p, None, None), b"null")
    bad(lib.fr_vq_nearest(10, 64, 48, p, 10, None, 0, p, p, p + 4, None), b"aligned")
    assert lib.fr_vq_nearest(0, 64, 48, None, 0, None, 0, None, None, None, None) == 0
    bad(lib.fr_vq_gather(10, 64, 48, None, 10, None, 0, p, p, 0, None, p, None, 1.0, p, None), b"feats")
    bad(lib.fr_vq_gather(10, 64, 48, p, 10, None, 0, None, p, 0, p, None, None, 1.0, p, None), b"null")
    bad(lib.fr_vq_update(0, 64, 48, p, 10, None, 0, None, p, 0.8, 1e-5, p, p, p, None), b"no rows")
    bad(lib.fr_vq_update(10, 64, 48, p, 10, None, 0, None, p, 1.5, 1e-5, p, p, p, None), b"decay")
    bad(lib.fr_vq_update(10, 64, 48, p, 10, None, 0, None, None, 0.8, 1e-5, p, p, p, None), b"null")
    bad(lib.fr_vq_replace(10, 64, 48, 65, p, 10, None, 0, p, p, p, p, None), b"k=65")
    bad(lib.fr_vq_replace(10, 8, 48, 9, p, 10, None, 0, p, p, p, p, None), b"k=9")
    bad(lib.fr_vq_replace(5, 64, 48, 6, p, 10, p, 0, p, p, p, p, None), b"k=6")
    assert lib.fr_vq_replace(10, 64, 48, 0, None, 10, None, 0, None, None, None, None, None) == 0
    for fn in (lib.fr_pack_bits, lib.fr_unpack_bits):
        bad(fn(10, 0, p, p, None), b"bits=0")
        bad(fn(10, 17, p, p, None), b"bits=17")
        bad(fn(-1, 13, p, p, None), b"count")
        bad(fn(10, 13, None, p, None), b"null")
        assert fn(0, 13, None, None, None) == 0
