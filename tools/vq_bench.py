"""VecTree vector quantisation (fov3dgs_amd.vectree; csrc/vq.hip) on the MI355X against the reference's expression restated in torch
(LightGaussian/vectree/vq.py:262-299, vectree.py:196-204, :80-97: cdist, argmax, one_hot, einsum, topk), in ONE process, the two
forms alternating round by round; --warmup rounds, then the timed rounds; device events around each call; median, p10-p90, min and
max in ms. On the SH rows of S-6M (synthetic.scene_bicycle_scale), at D = 48 and at D = 27 (its leading 27 SH columns):
  step      one training iteration at n = 80 000 sampled rows (with replacement) of the 60 % least important rows, K = 8192: draw
            -> assignment -> loss -> EMA step -> replacement of the 10 emptiest codes. fused: VectorQuantize.step on the rows in
            place; torch_form: the gathers and the n x K matrices of the reference.
  search    the nearest-code search of that iteration alone, and its achieved TFLOP/s (2 n K D flop) against the 157.3 TFLOP/s of
            the f32 matrix instruction.
  assign    the final assignment of all N rows (vectree.assign_all; torch_form: 8192-row chunks of cdist + argmax + gather).
  peak_mb   torch.cuda.max_memory_allocated over one call of each form, above what was allocated before it.
  shapes    with --alt-lib (a second build of the library, tools/scratch/vq_mfma32.patch applied and built with EXTRA=-DVQ_MFMA32: the
            search on v_mfma_f32_32x32x2_f32 instead of the library's 16x16x4 form): the search of the step and of all N rows with
            each, alternating; alt_faster_beyond_spread: the alternative's p90 lies below the library's p10, lib_faster_beyond_spread:
            the other way round.
*_faster_beyond_spread: the fused form's p90 lies below the torch form's p10. No GPU, no run: there is no fallback.

usage: python tools/vq_bench.py [--rounds 10] [--slow-rounds 3] [--warmup 2] [--P 6000000] [--n 80000] [--K 8192] [--alt-lib PATH]
                                [--out profiles/vq_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fov3dgs_amd  # noqa: E402,F401
from fov3dgs_amd import _native  # noqa: E402
from fov3dgs_amd import synthetic as syn  # noqa: E402
from fov3dgs_amd import vectree  # noqa: E402

PEAK_TFLOPS, K_EXPIRE, DECAY, EPS = 157.3, 10, 0.8, 1e-5


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "p10_ms": round(sorted(ms)[len(ms) // 10], 4), "p90_ms": round(sorted(ms)[(9 * len(ms)) // 10], 4), "n": len(ms)}


def beyond_spread(fast, slow):
    return bool(fast["p90_ms"] < slow["p10_ms"])


def torch_step(embed, cluster_size, pool, imp, indexes, K):
    """one iteration of vectree.py:197-204 around vq.py:262-299 and :405-407, as the reference writes it"""
    vq_weight, x = imp[indexes], pool[indexes, :]
    weight = vq_weight.reshape(1, -1, 1)
    weight = weight * weight.numel() / weight.sum()
    flatten = x.unsqueeze(0)
    dist = -torch.cdist(flatten, embed, p=2)
    embed_ind = dist.argmax(dim=-1)
    embed_onehot = F.one_hot(embed_ind, K).type(flatten.dtype)
    quantize = embed[0][embed_ind[0]]
    cluster_size.mul_(DECAY).add_((embed_onehot * weight).sum(dim=1), alpha=1 - DECAY)
    embed_sum = torch.einsum("hnd,hnc->hcd", flatten * weight, embed_onehot)
    smoothed = (cluster_size + EPS) / (cluster_size.sum() + K * EPS) * cluster_size.sum()
    embed.mul_(DECAY).add_(embed_sum / smoothed.unsqueeze(-1), alpha=1 - DECAY)
    loss = F.mse_loss(quantize.unsqueeze(0), flatten)
    _, replace_index = torch.topk(cluster_size, k=K_EXPIRE, largest=False)
    _, most_important_index = torch.topk(vq_weight, k=K_EXPIRE, largest=True)
    embed[:, replace_index, :] = x[most_important_index, :]
    return loss


def torch_assign(embed, feats, chunk=8192):
    fl, il = [], []
    for i in range(0, feats.shape[0], chunk):
        flatten = feats[i:i + chunk, :].unsqueeze(0)
        ind = (-torch.cdist(flatten, embed, p=2)).argmax(dim=-1)
        il.append(ind[0])
        fl.append(embed[0][ind[0]])
    return torch.cat(fl).half().float(), torch.cat(il)


def second_library(path):
    """another build of the library beside the package's own (same ABI check), for A / B rounds under one Python"""
    own = _native.load()
    _native._lib, keep = None, _native.LIB_PATH
    try:
        _native.LIB_PATH = path
        other = _native.load()
    finally:
        _native.LIB_PATH, _native._lib = keep, own
    return own, other


def shapes(pool, feats, cb, idx, a):
    own, alt = second_library(a.alt_lib)

    def search(lib, x, rows):
        _native._lib = lib
        try:
            return vectree.nearest_code(x, cb, rows=rows)
        finally:
            _native._lib = own
    r = {}
    for name, x, rows, rounds in (("step", pool, idx, a.rounds), ("assign", feats, None, a.slow_rounds)):
        t = timed((("mfma_16x16x4", lambda: search(own, x, rows)), ("mfma_32x32x2", lambda: search(alt, x, rows))), rounds, a.warmup)
        t["same_indices"] = bool(torch.equal(search(own, x, rows), search(alt, x, rows)))
        t["alt_faster_beyond_spread"] = beyond_spread(t["mfma_32x32x2"], t["mfma_16x16x4"])
        t["lib_faster_beyond_spread"] = beyond_spread(t["mfma_16x16x4"], t["mfma_32x32x2"])
        r[name] = t
    return r


def timed(forms, rounds, warmup):
    ms = {k: [] for k, _ in forms}
    for it in range(warmup + rounds):
        evs = []
        for k, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs.append((k, e0, e1))
        torch.cuda.synchronize()
        if it >= warmup:
            for k, e0, e1 in evs:
                ms[k].append(e0.elapsed_time(e1))
    return {k: summary(v) for k, v in ms.items()}


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def one_dim(feats, imp, a, dev):
    N, D = feats.shape
    K, n = a.K, a.n
    g = torch.Generator(device=dev).manual_seed(1)
    mask = vectree.select_non_vq(imp, 0.6)
    pool, w = feats[~mask].contiguous(), imp[~mask].contiguous()
    start = pool[torch.randperm(pool.shape[0], device=dev, generator=g)[:K]].clone()  # (a spread-out codebook: rows of the pool)
    vq = vectree.VectorQuantize(dim=D, codebook_size=K, decay=DECAY, commitment_weight=1.0, use_cosine_sim=False, threshold_ema_dead_code=0,
                                codebook=start).to(dev)
    embed_t, cs_t = start[None].clone(), torch.zeros(1, K, device=dev)
    draw = lambda: torch.randint(0, pool.shape[0], (n,), device=dev, generator=g)
    r = {"rows": int(N), "pool_rows": int(pool.shape[0]), "n": n, "K": K, "D": D}
    with torch.no_grad():
        step = timed((("fused", lambda: vq.step(pool, w, draw(), k_expire=K_EXPIRE)),
                      ("torch_form", lambda: torch_step(embed_t, cs_t, pool, w, draw(), K))), a.rounds, a.warmup)
        step["fused_faster_beyond_spread"] = beyond_spread(step["fused"], step["torch_form"])
        idx = draw()
        step["peak_mb"] = {"fused": peak_mb(lambda: vq.step(pool, w, idx, k_expire=K_EXPIRE)),
                           "torch_form": peak_mb(lambda: torch_step(embed_t, cs_t, pool, w, idx, K))}
        r["step"] = step
        cb = vq._codebook.embed
        search = timed((("fused", lambda: vectree.nearest_code(pool, cb, rows=idx)),
                        ("torch_form", lambda: (-torch.cdist(pool[idx][None], cb, p=2)).argmax(dim=-1))), a.rounds, a.warmup)
        search["fused_tflops"] = round(2.0 * n * K * D / (search["fused"]["median_ms"] * 1e-3) / 1e12, 2)
        search["fused_share_of_peak"] = round(search["fused_tflops"] / PEAK_TFLOPS, 4)
        search["fused_faster_beyond_spread"] = beyond_spread(search["fused"], search["torch_form"])
        r["search"] = search
        if a.alt_lib:
            r["shapes"] = shapes(pool, feats, cb, idx, a)
        assign = timed((("fused", lambda: vectree.assign_all(feats, vq)), ("torch_form", lambda: torch_assign(cb, feats))), a.slow_rounds, 1)
        assign["fused_tflops"] = round(2.0 * N * K * D / (assign["fused"]["median_ms"] * 1e-3) / 1e12, 2)
        assign["fused_faster_beyond_spread"] = beyond_spread(assign["fused"], assign["torch_form"])
        assign["peak_mb"] = {"fused": peak_mb(lambda: vectree.assign_all(feats, vq)), "torch_form": peak_mb(lambda: torch_assign(cb, feats))}
        got, want = vectree.assign_all(feats, vq)[1], torch_assign(cb, feats)[1]
        assign["rows_that_differ_from_torch_form"] = int((got != want).sum())
        r["assign"] = assign
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--slow-rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--P", type=int, default=6_000_000)
    ap.add_argument("--n", type=int, default=80000)
    ap.add_argument("--K", type=int, default=8192)
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vq_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "vq_bench needs the MI355X"
    dev = "cuda:0"
    base = syn.scene_bicycle_scale(P=a.P)
    table = vectree.feature_table(base)[:, 6:54].to(dev)
    del base
    imp = torch.rand(a.P, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) ** 3
    result = {"device": torch.cuda.get_device_name(0), "scene": "S-6M" if a.P == 6_000_000 else f"scene_bicycle_scale(P={a.P})",
              "rounds": a.rounds, "slow_rounds": a.slow_rounds, "warmup": a.warmup, "peak_tflops_f32_matrix": PEAK_TFLOPS,
              "protocol": "one process, the two forms alternate round by round; device events around each call"}
    for D in (48, 27):
        result[f"D{D}"] = one_dim(table[:, :D].contiguous(), imp, a, dev)
        print(json.dumps({f"D{D}": result[f"D{D}"]}), flush=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
