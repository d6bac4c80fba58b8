"""Golden vectors for the VecTree vector quantisation from the REFERENCE's own code (run by hand in the build container, on the CPU:
python tests/golden/make_vq_golden.py -> tests/golden/ref_vq.npz). Only data is written; no reference source is copied.

LightGaussian/vectree/vq.py's VectorQuantize runs on the CPU as it is (einops is installed). vectree/utils.py imports plyfile, which
this environment lacks and load_vqgaussian never uses: an empty stand-in module of that name is put into sys.modules before the import,
nothing else is replaced.

Per D in (48, 27), with n = 500 rows, K = 64 codes ("{D}_" prefixes the names):
  (a) x, w, embed0, cs0 -> one weighted training step (aw_*) and one unweighted step (au_*) of the reference from that state:
      embed, cluster_size, ind, quantize, loss
  (b) pool, imp, indexes [3, 300]: three iterations of the loop of vectree.py:196-204 on the reference object, its replacement
      lines included: b_embed, b_cluster_size, b_loss [3], b_codes / b_rows [3, 10] (the topk results that were applied)
  (c) an eval() forward from (a)'s state: c_ind, c_quantize, c_loss; the state is asserted unchanged
  (d) once (D = 27): a container written by fov3dgs_amd.vectree.save_vq on the CPU (d_file_<name>: the bytes of its seven files) and the
      table the reference's load_vqgaussian decodes from it (d_decoded); d_table, d_mask, d_indice, d_codebook are save_vq's inputs
  err_*: the distance (max abs) of the reference's float32 outputs to the float64 restatement (tests/vq_ref.py) on the same inputs --
      what the GPU tests' tolerance is four times of.

Asserted here, so that torch's unspecified orders never enter a fixture: no row's assignment is ambiguous under the bound of
tests/vq_ref.py (second-best d^2 within B_i of the best) in any step; the k + 1 smallest cluster sizes and the k + 1 largest sampled
weights are distinct in every iteration of (b)."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FOVRASTER_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
from tests import vq_ref  # noqa: E402

N_ROWS, K, K_EXPIRE = 500, 64, 10


def reference_modules():
    vt = os.path.join(REF, "LightGaussian", "vectree")
    if not os.path.isdir(vt):
        sys.exit(f"no {vt} here: these vectors can only be made in the build container")
    sys.path.insert(0, vt)
    sys.modules.setdefault("plyfile", types.ModuleType("plyfile"))
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = None
    import vq
    import utils
    return vq, utils


def make_inputs(D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N_ROWS, D, generator=g) * 0.3
    x[:, :3] += 0.8  # the DC term of SH rows is offset from zero
    pick = torch.randperm(N_ROWS, generator=g)[:K]
    embed0 = x[pick] + 0.05 * torch.randn(K, D, generator=g)
    embed0[[5, 40], :3] += 2.0  # two codes no row is near: they take no member and must decay
    cs0 = 0.5 + 4.5 * torch.rand(K, generator=g)
    w = torch.rand(N_ROWS, generator=g) ** 3 * 10 + 1e-3
    return x, w, embed0, cs0


def ref_object(vqmod, D, embed0, cs0):
    m = vqmod.VectorQuantize(dim=D, codebook_size=K, decay=0.8, commitment_weight=1.0, use_cosine_sim=False, threshold_ema_dead_code=0)
    with torch.no_grad():
        m._codebook.embed.copy_(embed0[None])
        m._codebook.cluster_size.copy_(cs0[None])
    return m


def unambiguous(x, e, what):
    ind, amb, _, _ = vq_ref.assignment(x.numpy(), e.numpy())
    assert not amb.any(), f"{what}: {int(amb.sum())} ambiguous rows"
    return ind


def distinct(v, k, what):
    s = np.sort(np.asarray(v))
    assert (np.diff(s[:k + 1]) > 0).all(), f"{what}: ties among the {k + 1} smallest"


def err(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def main():
    vqmod, utils = reference_modules()
    out, errs = {}, {}
    for D, seed in ((48, 11), (27, 12)):
        p = f"{D}_"
        x, w, embed0, cs0 = make_inputs(D, seed)
        out.update({p + "x": x.numpy(), p + "w": w.numpy(), p + "embed0": embed0.numpy(), p + "cs0": cs0.numpy()})
        ind64 = unambiguous(x, embed0, "a")
        for tag, weight in (("aw_", w), ("au_", None)):
            m = ref_object(vqmod, D, embed0, cs0).train()
            with torch.no_grad():
                q, ind, loss = m(x[None], weight=None if weight is None else weight.reshape(1, -1, 1))
            assert np.array_equal(ind[0].numpy(), ind64)
            r = vq_ref.train_step(x.numpy(), None if weight is None else weight.numpy(), embed0.numpy(), cs0.numpy(), ind64)
            got = dict(embed=m._codebook.embed[0].numpy(), cluster_size=m._codebook.cluster_size[0].numpy(), quantize=q[0].numpy(),
                       loss=loss.detach().numpy())
            for name, v in got.items():
                out[p + tag + name] = np.array(v, copy=True)
                errs[p + tag + name] = err(v, r[name])
            out[p + tag + "ind"] = ind[0].numpy().astype(np.int32)
        # (c)
        m = ref_object(vqmod, D, embed0, cs0).eval()
        with torch.no_grad():
            q, ind, loss = m(x[None])
        assert torch.equal(m._codebook.embed[0], embed0) and torch.equal(m._codebook.cluster_size[0], cs0)
        assert np.array_equal(ind[0].numpy(), ind64)
        out.update({p + "c_ind": ind[0].numpy().astype(np.int32), p + "c_quantize": q[0].numpy(), p + "c_loss": loss.detach().numpy()})
        # (b)
        g = torch.Generator().manual_seed(seed + 100)
        pool = torch.cat([x, x[:200] * 0.9 + 0.02 * torch.randn(200, D, generator=g)])
        imp = torch.rand(pool.shape[0], generator=g) ** 3 * 10 + 1e-3
        indexes = torch.stack([torch.randperm(pool.shape[0], generator=g)[:300] for _ in range(3)])  # (no row twice: distinct weights)
        m = ref_object(vqmod, D, embed0, cs0).train()
        e64, cs64 = embed0.numpy().astype(np.float64), cs0.numpy().astype(np.float64)
        losses, codes, rows, l64 = [], [], [], []
        with torch.no_grad():
            for it in range(3):
                vq_weight, vq_feature = imp[indexes[it]], pool[indexes[it], :]
                i64 = unambiguous(vq_feature, m._codebook.embed[0], f"b{it}")
                _, embed_ind, loss = m(vq_feature.unsqueeze(0), weight=vq_weight.reshape(1, -1, 1))
                assert np.array_equal(embed_ind[0].numpy(), i64)
                distinct(m._codebook.cluster_size[0].numpy(), K_EXPIRE, f"b{it} cluster_size")
                distinct(-vq_weight.numpy(), K_EXPIRE, f"b{it} weights")
                _, replace_index = torch.topk(m._codebook.cluster_size, k=K_EXPIRE, largest=False)
                _, most_important_index = torch.topk(vq_weight, k=K_EXPIRE, largest=True)
                m._codebook.embed[:, replace_index, :] = vq_feature[most_important_index, :]
                losses.append(float(loss)); codes.append(replace_index[0].numpy()); rows.append(most_important_index.numpy())
                # the float64 replay, on its own state (the assignments were asserted equal and unambiguous on the reference's)
                r = vq_ref.train_step(vq_feature.numpy(), vq_weight.numpy(), e64, cs64, i64)
                e64, c64, r64 = vq_ref.replace(r["embed"], r["cluster_size"], vq_feature.numpy(), vq_weight.numpy(), K_EXPIRE)
                cs64 = r["cluster_size"]
                assert np.array_equal(c64, codes[-1]) and np.array_equal(r64, rows[-1])
                l64.append(r["loss"])
        out.update({p + "pool": pool.numpy(), p + "imp": imp.numpy(), p + "indexes": indexes.numpy().astype(np.int64),
                    p + "b_embed": m._codebook.embed[0].numpy().copy(), p + "b_cluster_size": m._codebook.cluster_size[0].numpy().copy(),
                    p + "b_loss": np.asarray(losses, np.float32), p + "b_codes": np.stack(codes).astype(np.int32),
                    p + "b_rows": np.stack(rows).astype(np.int32)})
        errs[p + "b_embed"] = err(out[p + "b_embed"], e64)
        errs[p + "b_cluster_size"] = err(out[p + "b_cluster_size"], cs64)
        errs[p + "b_loss"] = err(out[p + "b_loss"], l64)
    # (d)
    import fov3dgs_amd  # noqa: F401
    from fov3dgs_amd import vectree
    g = torch.Generator().manual_seed(5)
    Nd, Dd, Kd = 203, 27, 16
    table = torch.randn(Nd, 6 + 45 + 3 + 8, generator=g)  # a degree-3 PLY quantised at --sh_degree 2: 27 of its 48 SH columns
    mask = vectree.select_non_vq(torch.rand(Nd, generator=g), 0.6)
    indice = torch.randint(0, Kd, (Nd,), generator=g)
    codebook = torch.randn(Kd, Dd, generator=g)
    with tempfile.TemporaryDirectory() as tmp:
        vectree.save_vq(tmp, table, mask, indice, codebook, Dd)
        decoded = utils.load_vqgaussian(tmp, device="cpu").numpy()
        for name in vectree.FILES:
            out["d_file_" + name[:-4]] = np.frombuffer(open(os.path.join(tmp, name), "rb").read(), np.uint8)
    out.update(d_decoded=decoded, d_table=table.numpy(), d_mask=mask.numpy(), d_indice=indice.numpy().astype(np.int32), d_codebook=codebook.numpy())
    for name, v in sorted(errs.items()):
        print(f"err_{name} = {v:.3e}")
        out["err_" + name] = np.float64(v)
    np.savez_compressed(os.path.join(HERE, "ref_vq.npz"), **out)
    print("wrote ref_vq.npz", os.path.getsize(os.path.join(HERE, "ref_vq.npz")), "bytes")


if __name__ == "__main__":
    main()
