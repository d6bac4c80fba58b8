"""LightGaussian's VecTree SH vector quantisation on the HIP library (csrc/vq.hip): the step that turns a pruned model into
something small enough to ship -- the most significant rows keep their SH coefficients at fp16, the SH vectors of the others
become log2(K)-bit indices into a K-entry codebook.

Drops in for (LightGaussian/vectree/)
  vq.VectorQuantize                          vq.py:308-442 with EuclideanCodebook :179-304, in the ONE configuration vectree.py:44-51
                                             uses: one head, no projection, decay EMA, kmeans_init=False, threshold_ema_dead_code=0,
                                             sample_codebook_temp=0, no orthogonal regularisation. Anything else raises ValueError.
  Quantization.quantize                      vectree.py:166-204 -> select_non_vq, train_codebook
  Quantization.calc_vector_quantized_feature vectree.py:80-97   -> assign_all
  Quantization.fully_vq_reformat             vectree.py:100-146 -> save_vq (without the zip of :150)
  utils.load_vqgaussian                      utils.py:5-65      -> load_vq
  quantize_model ties them together for a GaussianCloud or a PLY file (model_io's column order).

What the kernels do instead of cdist / argmax / one_hot / einsum / topk is described in csrc/vq.hip. A training iteration is enqueued
without a host synchronisation: sum w, sum cluster_size and both selections stay on the device.

Where torch leaves an order unspecified, it is fixed here:
  * the assignment: an exact tie of two scores goes to the LOWER code index (torch.argmax of -cdist: unspecified on the GPU);
  * torch.topk (vectree.py:176, :202, :203): among equal values the LOWEST index is taken first -- for the k codes of smallest
    cluster_size, for the k sampled rows of largest weight (a row drawn twice is two entries: the earlier position first) and for the
    non-VQ mask (select_non_vq: the order of torch.sort(-importance, stable=True));
  * the sums per code run in ascending row position, one rounding per term, and the scalars in double in a fixed order: same
    bits on every run.
In train() mode the reference returns quantize = x + (embed[ind] - x) (the straight-through expression, rounded twice) and takes the
loss from it; here quantize = embed[ind] exactly and the loss comes from the differences x - embed[ind].

The search, the step and the replacement need GPU tensors: there is no CPU fallback. The bit packing, select_non_vq and the
container functions also take CPU tensors (plain numpy / torch)."""
import math
import os

import numpy as np
import torch
from torch import nn

from . import _native, pruning
from .pruning import _check, _require_gpu, _stream

MAX_D, MAX_K, MAX_EXPIRE = 64, 65536, 64
_workspaces = {}


def _workspace(lib, n, K, D, training, device):
    need = max(int(lib.fr_vq_workspace_bytes(n, K, D, int(training))), 16)
    ws = _workspaces.get(device)
    if ws is None or ws.numel() < need:  # (grow-only, one per device: use it from one stream at a time)
        ws = _workspaces[device] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def _table(x, what, D=None):
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"{what}: expected a float32 [rows, D] tensor, got {x.dtype} {list(x.shape)}")
    if not 1 <= x.shape[1] <= MAX_D or (D is not None and x.shape[1] != D):
        raise ValueError(f"{what}: D = {x.shape[1]}" + (f", the codebook has D = {D}" if D is not None else f" is not in 1..{MAX_D}"))
    return x.detach().contiguous()


def _rows(rows, device):
    if rows is None:
        return None, 0, None
    if rows.dim() != 1 or rows.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"rows must be an int32 or int64 vector, got {rows.dtype} {list(rows.shape)}")
    if rows.device != device:
        raise RuntimeError(f"rows on {rows.device}, the table on {device}")
    rows = rows.contiguous()
    return rows, int(rows.dtype == torch.int64), rows.data_ptr()


def _codebook2d(codebook):
    cb = codebook[0] if codebook.dim() == 3 and codebook.shape[0] == 1 else codebook
    cb = _table(cb, "codebook")
    if not 1 <= cb.shape[0] <= MAX_K:
        raise ValueError(f"codebook: K = {cb.shape[0]} is not in 1..{MAX_K}")
    return cb


@torch.no_grad()
def _nearest(feats, cb, rows=None, out=None):
    """int32 [n]: the nearest code of feats[rows] (feats [N,D], cb [K,D]: float32, contiguous, on the GPU). No synchronisation."""
    K, D = cb.shape
    r, r64, rp = _rows(rows, feats.device)
    n = feats.shape[0] if r is None else r.shape[0]
    ind = torch.empty(n, dtype=torch.int32, device=feats.device) if out is None else out
    if n == 0:
        return ind
    if feats.shape[0] == 0:
        raise ValueError("rows index an empty table")
    lib = _native.load()
    with torch.cuda.device(feats.device):
        ws = _workspace(lib, n, K, D, False, feats.device)
        rc = lib.fr_vq_nearest(n, K, D, feats.data_ptr(), feats.shape[0], rp, r64, cb.data_ptr(), ind.data_ptr(), ws.data_ptr(),
                               _stream(feats.device))
    _check(rc, "vq_nearest")
    return ind


@torch.no_grad()
def _gather(feats, cb, ind, rows=None, quantize=False, to_half=False, dist2=False, loss_weight=None):
    """-> (quantize [n,D] or None, dist2 [n] or None, loss [1] or None) of feats[rows] against cb[ind]"""
    K, D = cb.shape
    r, r64, rp = _rows(rows, feats.device)
    n = ind.shape[0]
    dev = feats.device
    q = torch.empty((n, D), dtype=torch.float32, device=dev) if quantize else None
    d2 = torch.empty(n, dtype=torch.float32, device=dev) if dist2 else None
    loss = torch.zeros(1, dtype=torch.float32, device=dev) if loss_weight is not None else None
    if n == 0:
        return q, d2, loss
    lib = _native.load()
    with torch.cuda.device(dev):
        ws = _workspace(lib, n, K, D, False, dev)
        rc = lib.fr_vq_gather(n, K, D, feats.data_ptr(), feats.shape[0], rp, r64, cb.data_ptr(), ind.data_ptr(), int(bool(to_half)),
                              None if q is None else q.data_ptr(), None if d2 is None else d2.data_ptr(),
                              None if loss is None else loss.data_ptr(), 0.0 if loss_weight is None else float(loss_weight),
                              ws.data_ptr(), _stream(dev))
    _check(rc, "vq_gather")
    return q, d2, loss


@torch.no_grad()
def nearest_code(x, codebook, rows=None, return_distance=False):
    """ind[i] = argmin_c ||x_i - codebook_c|| (vq.py:276-277), int32 [n]; an exact tie goes to the lower code. x: float32 [N,D],
    codebook: [K,D] or [1,K,D]; rows (int32 / int64 [n]): assign x[rows] without materialising the gather (an index outside
    0..N-1 is clamped, not followed). return_distance: -> (ind, ||x_i - codebook[ind_i]||), the distance taken from the differences.
    No host synchronisation."""
    _require_gpu("nearest_code", x, codebook)
    cb = _codebook2d(codebook)
    feats = _table(x, "nearest_code", cb.shape[1])
    ind = _nearest(feats, cb, rows)
    if not return_distance:
        return ind
    return ind, torch.sqrt(_gather(feats, cb, ind, rows, dist2=True)[1])


def _uniform_init(*shape):
    t = torch.empty(shape)
    nn.init.kaiming_uniform_(t)  # vq.py:25-28
    return t


class EuclideanCodebook(nn.Module):
    """The state of vq.py's EuclideanCodebook: embed [1,K,D], cluster_size [1,K] (and embed_avg, initted: kept for state_dict parity)"""

    def __init__(self, dim, codebook_size, decay=0.8, eps=1e-5, embed=None):
        super().__init__()
        self.decay, self.eps, self.codebook_size, self.num_codebooks = decay, eps, codebook_size, 1
        if embed is None:
            embed = _uniform_init(1, codebook_size, dim)
        else:
            embed = embed.detach().float().reshape(1, codebook_size, dim).clone()
        self.register_buffer("initted", torch.Tensor([True]))
        self.register_buffer("cluster_size", torch.zeros(1, codebook_size))
        self.register_buffer("embed_avg", embed.clone())
        self.register_buffer("embed", embed)


class VectorQuantize(nn.Module):
    """vq.VectorQuantize in the configuration vectree.py:44-51 uses. forward(x, weight=None) -> (quantize, embed_ind, loss) with x
    [1,n,D] (or [n,D]), weight [1,n,1] (any shape with n elements). train(): the EMA step of vq.py:282-299 on the codebook as it
    stood when the rows were assigned, loss = commitment_weight * mse(embed[ind], x) as a 1-element tensor; eval(): nothing is
    updated, the loss is [0.]. codebook=: a [K,D] tensor to start from instead of the reference's kaiming_uniform_."""

    def __init__(self, dim, codebook_size, codebook_dim=None, heads=1, separate_codebook_per_head=False, decay=0.8, eps=1e-5,
                 kmeans_init=False, kmeans_iters=10, use_cosine_sim=False, threshold_ema_dead_code=0, channel_last=True,
                 accept_image_fmap=False, commitment_weight=1.0, orthogonal_reg_weight=0.0, orthogonal_reg_active_codes_only=False,
                 orthogonal_reg_max_codes=None, sample_codebook_temp=0.0, sync_codebook=False, codebook=None):
        super().__init__()
        refused = (("use_cosine_sim", use_cosine_sim, False), ("heads", heads, 1), ("kmeans_init", kmeans_init, False),
                   ("codebook_dim", dim if codebook_dim is None else codebook_dim, dim),
                   ("threshold_ema_dead_code", threshold_ema_dead_code, 0), ("sample_codebook_temp", sample_codebook_temp, 0),
                   ("orthogonal_reg_weight", orthogonal_reg_weight, 0), ("separate_codebook_per_head", separate_codebook_per_head, False),
                   ("channel_last", channel_last, True), ("accept_image_fmap", accept_image_fmap, False), ("sync_codebook", sync_codebook, False))
        for name, got, only in refused:
            if got != only:
                raise ValueError(f"VectorQuantize: {name}={got!r} is not supported (only {only!r}: the configuration of "
                                 "LightGaussian/vectree/vectree.py:44-51)")
        if not 1 <= int(dim) <= MAX_D:
            raise ValueError(f"VectorQuantize: dim = {dim} is not in 1..{MAX_D}")
        if not 1 <= int(codebook_size) <= MAX_K:
            raise ValueError(f"VectorQuantize: codebook_size = {codebook_size} is not in 1..{MAX_K}")
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"VectorQuantize: decay = {decay} is not in 0..1")
        if codebook is not None and tuple(codebook.shape[-2:]) != (codebook_size, dim):
            raise ValueError(f"VectorQuantize: codebook of shape {list(codebook.shape)}, expected [{codebook_size}, {dim}]")
        self.dim, self.codebook_size, self.heads = int(dim), int(codebook_size), 1
        self.eps, self.commitment_weight = eps, commitment_weight
        self._codebook = EuclideanCodebook(self.dim, self.codebook_size, decay, eps, codebook)

    @property
    def codebook(self):
        return self._codebook.embed[0]

    def _state(self):
        cbk = self._codebook
        e, cs = cbk.embed, cbk.cluster_size
        _require_gpu("VectorQuantize", e, cs)
        if e.dtype != torch.float32 or cs.dtype != torch.float32 or not e.is_contiguous() or not cs.is_contiguous():
            raise ValueError("VectorQuantize: embed and cluster_size must be contiguous float32 buffers (they are updated in place)")
        if tuple(e.shape) != (1, self.codebook_size, self.dim) or tuple(cs.shape) != (1, self.codebook_size):
            raise ValueError(f"VectorQuantize: embed {list(e.shape)} / cluster_size {list(cs.shape)} do not fit K = {self.codebook_size}, D = {self.dim}")
        return e, cs

    @torch.no_grad()
    def step(self, feats, weights=None, rows=None, k_expire=0, want_quantize=False):
        """One iteration on feats[rows] (feats [N,D], weights [N] indexed like feats; rows None: all rows): assignment, loss, the EMA step
        when training, then the replacement of the k_expire emptiest codes (vectree.py:202-204). -> (quantize or None, ind int32, loss).
        No host synchronisation."""
        e, cs = self._state()
        K, D = self.codebook_size, self.dim
        _require_gpu("VectorQuantize", e, feats, *(() if weights is None else (weights,)))
        feats = _table(feats, "VectorQuantize", D)
        N = feats.shape[0]
        if weights is not None:
            if weights.numel() != N or weights.dtype != torch.float32:
                raise ValueError(f"weight: expected {N} float32 values, got {weights.dtype} {list(weights.shape)}")
            weights = weights.detach().reshape(-1).contiguous()
        dev = feats.device
        r, r64, rp = _rows(rows, dev)
        n = N if r is None else r.shape[0]
        cb = e[0]
        ind = _nearest(feats, cb, r)
        q, _, loss = _gather(feats, cb, ind, r, quantize=want_quantize,
                             loss_weight=self.commitment_weight if self.training and self.commitment_weight > 0 else None)
        if loss is None:
            loss = torch.zeros(1, dtype=torch.float32, device=dev)
        if not self.training or n == 0:
            return q, ind, loss
        k = int(k_expire)
        if k < 0 or k > MAX_EXPIRE or k > n:
            raise ValueError(f"k_expire = {k} is not in 0..min({MAX_EXPIRE}, n = {n})")
        lib = _native.load()
        wp = None if weights is None else weights.data_ptr()
        with torch.cuda.device(dev):
            ws = _workspace(lib, n, K, D, True, dev)
            s = _stream(dev)
            _check(lib.fr_vq_update(n, K, D, feats.data_ptr(), N, rp, r64, wp, ind.data_ptr(), float(self._codebook.decay), float(self.eps),
                                    e.data_ptr(), cs.data_ptr(), ws.data_ptr(), s), "vq_update")
            if k > 0:
                _check(lib.fr_vq_replace(n, K, D, k, feats.data_ptr(), N, rp, r64, wp, e.data_ptr(), cs.data_ptr(), ws.data_ptr(), s), "vq_replace")
        return q, ind, loss

    def forward(self, x, weight=None, verbose=False):
        if x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[0] != 1) or x.shape[-1] != self.dim:
            raise ValueError(f"VectorQuantize: expected x of shape [1, n, {self.dim}] or [n, {self.dim}], got {list(x.shape)}")
        flat = x.detach().float().reshape(-1, self.dim)
        q, ind, loss = self.step(flat, None if weight is None else weight.detach().float().reshape(-1), want_quantize=True)
        return q.reshape(x.shape), ind.to(torch.int64).reshape(x.shape[:-1]), loss


@torch.no_grad()
def select_non_vq(importance, vq_ratio):
    """non_vq_mask (bool [N]) of vectree.py:175-179: the int(N * (1 - vq_ratio)) rows of largest importance keep their SH vectors.
    Among equal importances the lowest index goes first (torch.topk leaves it open). float64 scores are compared as float32."""
    imp = importance if torch.is_tensor(importance) else torch.as_tensor(np.asarray(importance))
    imp = imp.detach().reshape(-1)
    N = imp.shape[0]
    k = int(N * (1 - vq_ratio))
    if not 0 <= k <= N:
        raise ValueError(f"vq_ratio = {vq_ratio} is not in 0..1")
    neg = -imp.float()
    if neg.is_cuda:
        return pruning.lowest_k_mask(neg, k)
    mask = torch.zeros(N, dtype=torch.bool)
    mask[torch.sort(neg, stable=True)[1][:k]] = True
    return mask


@torch.no_grad()
def train_codebook(feats, importance, vq, iterations=1000, chunk=80000, k_expire=10, indexes=None, generator=None):
    """The loop of vectree.py:187-204 on the pool `feats` [N,D] (the rows that will be quantised) and their importances [N] (None: no
    weights, --no_IS): each iteration draws `chunk` rows with replacement, runs the weighted step and overwrites the k_expire codes
    of smallest cluster_size with the drawn rows of largest weight (k_expire > codebook_size: none, as :194-195). indexes: an int
    [iterations, chunk] tensor on the device that replaces the draws (an index outside 0..N-1 is clamped, not followed). The rows
    are read in place -- no gather is materialised -- and nothing synchronises with the host. -> losses float32 [iterations]."""
    _require_gpu("train_codebook", feats)
    feats = _table(feats, "train_codebook", vq.dim)
    N = feats.shape[0]
    if N == 0:
        raise ValueError("train_codebook: no rows to quantise")
    w = None
    if importance is not None:
        _require_gpu("train_codebook", feats, importance)
        w = importance.detach().float().reshape(-1).contiguous()
        if w.shape[0] != N:
            raise ValueError(f"train_codebook: {N} rows, {w.shape[0]} importances")
    if indexes is not None:
        if indexes.dim() != 2 or indexes.dtype not in (torch.int32, torch.int64) or indexes.device != feats.device:
            raise ValueError("train_codebook: indexes must be an int32 / int64 [iterations, chunk] tensor on the rows' device")
        indexes = indexes.contiguous()
        iterations, chunk = indexes.shape
    iterations, chunk = int(iterations), int(chunk)
    k = int(k_expire)
    if k > vq.codebook_size:
        k = 0
    was_training = vq.training
    vq.train()
    losses = torch.zeros(iterations, dtype=torch.float32, device=feats.device)
    for it in range(iterations):
        rows = indexes[it] if indexes is not None else torch.randint(0, N, (chunk,), device=feats.device, generator=generator)
        losses[it:it + 1] = vq.step(feats, w, rows, k_expire=k)[2]
    vq.train(was_training)
    return losses


@torch.no_grad()
def assign_all(feats, vq):
    """calc_vector_quantized_feature (vectree.py:80-97): every row against the fp32 codebook (the .half().float() of :89 discards its
    result), in one launch instead of 8192-row chunks. -> (all_feat = embed[ind] rounded through fp16, float32 [N,D]; all_indice int64 [N])"""
    e, _ = vq._state()
    _require_gpu("assign_all", e, feats)
    feats = _table(feats, "assign_all", vq.dim)
    ind = _nearest(feats, e[0])
    all_feat = _gather(feats, e[0], ind, quantize=True, to_half=True)[0]
    return all_feat, ind.to(torch.int64)


# ---- bits ------------------------------------------------------------------------------------------------------------------
def _bits_arg(bits):
    bits = int(bits)
    if not 1 <= bits <= 16:
        raise ValueError(f"bits = {bits} is not in 1..16")
    return bits


@torch.no_grad()
def pack_bits(values, bits):
    """uint8 [(count * bits + 7) // 8]: the low `bits` of every value, MSB first, back to back -- np.packbits of the reference's dec2bin
    matrix (vectree.py:120-126). values: an integer vector; on the GPU one kernel, on the CPU numpy."""
    bits = _bits_arg(bits)
    v = values.detach().reshape(-1)
    if v.is_cuda:
        v = v.to(torch.int32).contiguous()
        out = torch.empty((v.shape[0] * bits + 7) // 8, dtype=torch.uint8, device=v.device)
        if v.shape[0]:
            with torch.cuda.device(v.device):
                _check(_native.load().fr_pack_bits(v.shape[0], bits, v.data_ptr(), out.data_ptr(), _stream(v.device)), "pack_bits")
        return out
    a = v.numpy().astype(np.int64)
    m = (a[:, None] >> np.arange(bits - 1, -1, -1)[None, :]) & 1
    return torch.from_numpy(np.packbits(m.astype(np.uint8).reshape(-1)))


@torch.no_grad()
def unpack_bits(packed, count, bits):
    """The inverse of pack_bits: int32 [count] (utils.py:33-38: np.unpackbits, bin2dec)"""
    bits, count = _bits_arg(bits), int(count)
    p = packed.detach().reshape(-1)
    if p.dtype != torch.uint8 or p.shape[0] < (count * bits + 7) // 8:
        raise ValueError(f"unpack_bits: {count} values of {bits} bits need {(count * bits + 7) // 8} uint8, got {p.dtype} {list(p.shape)}")
    if p.is_cuda:
        p = p.contiguous()
        out = torch.empty(count, dtype=torch.int32, device=p.device)
        if count:
            with torch.cuda.device(p.device):
                _check(_native.load().fr_unpack_bits(count, bits, p.data_ptr(), out.data_ptr(), _stream(p.device)), "unpack_bits")
        return out
    m = np.unpackbits(p.numpy())[:count * bits].reshape(count, bits).astype(np.int64)
    return torch.from_numpy((m << np.arange(bits - 1, -1, -1)[None, :]).sum(axis=1).astype(np.int32))


# ---- the container -----------------------------------------------------------------------------------------------------------
FILES = ("metadata.npz", "vq_indexs.npz", "codebook.npz", "non_vq_mask.npz", "non_vq_feats.npz", "other_attribute.npz", "xyz.npz")


def _wage(t, vq_way):
    t = t.detach().cpu()
    return (t.half() if vq_way == "half" else t).numpy()


@torch.no_grad()
def save_vq(folder, feats_full, non_vq_mask, all_indice, codebook, sh_dim, vq_way="half"):
    """The extreme_saving directory of vectree.py:106-146 (np.savez_compressed files; not the zip of :150). feats_full: the
    [N, 6 + ... + 8] table (x y z nx ny nz f_dc f_rest opacity scale rot), of which columns 6 .. 6 + sh_dim are the quantised
    vectors; all_indice: the code of EVERY row (only those outside non_vq_mask are stored, log2(K) bits each); codebook [K, sh_dim]
    or [1, K, sh_dim], K a power of two. -> folder"""
    cb = codebook[0] if codebook.dim() == 3 else codebook
    K = cb.shape[0]
    if K < 2 or K & (K - 1):
        raise ValueError(f"save_vq: the container needs a power-of-two codebook size >= 2 (log2(K) bits per index), got {K}")
    if cb.shape[1] != sh_dim or feats_full.dim() != 2 or feats_full.shape[1] < 6 + sh_dim + 8:
        raise ValueError(f"save_vq: codebook {list(cb.shape)}, table {list(feats_full.shape)}, sh_dim {sh_dim}")
    N = feats_full.shape[0]
    mask = non_vq_mask.detach().reshape(-1).bool()
    ind = all_indice.detach().reshape(-1)
    if mask.shape[0] != N or ind.shape[0] != N:
        raise ValueError(f"save_vq: {N} rows, {mask.shape[0]} mask entries, {ind.shape[0]} indices")
    os.makedirs(folder, exist_ok=True)
    metadata = dict(input_pc_num=int(N), input_pc_dim=int(feats_full.shape[1]), codebook_size=int(K), codebook_dim=int(sh_dim))
    np.savez_compressed(os.path.join(folder, "metadata.npz"), metadata=metadata)
    vq_index = ind[~mask.to(ind.device)]
    np.savez_compressed(os.path.join(folder, "vq_indexs.npz"), pack_bits(vq_index, int(math.log2(K))).cpu().numpy())
    np.savez_compressed(os.path.join(folder, "codebook.npz"), cb.detach().cpu().half().numpy())
    np.savez_compressed(os.path.join(folder, "non_vq_mask.npz"), np.packbits(mask.cpu().numpy()))
    full = feats_full.detach()
    np.savez_compressed(os.path.join(folder, "non_vq_feats.npz"), _wage(full[mask.to(full.device), 6:6 + sh_dim], vq_way))
    np.savez_compressed(os.path.join(folder, "other_attribute.npz"), _wage(full[:, -8:], vq_way))
    np.savez_compressed(os.path.join(folder, "xyz.npz"), full[:, 0:3].cpu().numpy())
    return folder


@torch.no_grad()
def load_vq(folder, device="cpu"):
    """load_vqgaussian (utils.py:5-65): -> the [N, input_pc_dim] float32 table; normals (and any column between the quantised
    vectors and the last eight) are zero."""
    def load_f(name, allow_pickle=False, array_name="arr_0"):
        return np.load(os.path.join(folder, name), allow_pickle=allow_pickle)[array_name]
    metadata = load_f("metadata.npz", True, "metadata").item()
    K, D = int(metadata["codebook_size"]), int(metadata["codebook_dim"])
    N, width = int(metadata["input_pc_num"]), int(metadata["input_pc_dim"])
    bits = int(math.log2(K))
    non_vq_mask = torch.from_numpy(np.unpackbits(load_f("non_vq_mask.npz"))[:N].astype(bool)).to(device)
    codebook = torch.from_numpy(load_f("codebook.npz")).float().to(device)
    vq_mask = ~non_vq_mask
    n_vq = int(vq_mask.sum())
    ind = unpack_bits(torch.from_numpy(load_f("vq_indexs.npz")).to(device), n_vq, bits).long()
    full = torch.zeros(N, width, device=device)
    full[:, 0:3] = torch.from_numpy(load_f("xyz.npz")).float().to(device)
    full[:, -8:] = torch.from_numpy(load_f("other_attribute.npz")).float().to(device)
    full[vq_mask, 6:6 + D] = codebook[ind]
    full[non_vq_mask, 6:6 + D] = torch.from_numpy(load_f("non_vq_feats.npz")).float().to(device)
    return full


# ---- whole models ------------------------------------------------------------------------------------------------------------
def feature_table(cloud):
    """-> float32 [P, 6 + 3 (n_rest + 1) + 8]: the PLY's columns in its order (model_io.save_ply: x y z nx ny nz f_dc_* f_rest_*
    opacity scale_* rot_*, f_dc / f_rest channel-major), as LightGaussian's read_ply_data returns them"""
    xyz = cloud._xyz.detach().float()
    return torch.cat([xyz, torch.zeros_like(xyz),
                      cloud._features_dc.detach().float().transpose(1, 2).flatten(start_dim=1),
                      cloud._features_rest.detach().float().transpose(1, 2).flatten(start_dim=1),
                      cloud._opacity.detach().float().reshape(-1, 1), cloud._scaling.detach().float(), cloud._rotation.detach().float()], dim=1)


def cloud_from_table(table, sh_degree=3):
    """The inverse of feature_table (GaussianModel.load_ply's reshapes, model_io.load_ply)"""
    from .synthetic import GaussianCloud
    P, n_rest = table.shape[0], (sh_degree + 1) ** 2 - 1
    if table.shape[1] != 6 + 3 * (n_rest + 1) + 8:
        raise ValueError(f"cloud_from_table: {table.shape[1]} columns, SH degree {sh_degree} has {6 + 3 * (n_rest + 1) + 8}")
    f_dc = table[:, 6:9].reshape(P, 1, 3).contiguous()
    f_rest = table[:, 9:9 + 3 * n_rest].reshape(P, 3, n_rest).transpose(1, 2).contiguous()
    return GaussianCloud(table[:, 0:3].contiguous(), f_dc, f_rest, table[:, -7:-4].contiguous(), table[:, -4:].contiguous(),
                         table[:, -8:-7].contiguous(), sh_degree=sh_degree)


@torch.no_grad()
def quantize_model(cloud_or_ply, importance, folder=None, codebook_size=8192, vq_ratio=0.6, iterations=1000, chunk=80000, k_expire=10,
                   sh_degree=3, sh_dim=None, vq_way="half", indexes=None, generator=None, codebook=None, device="cuda"):
    """vectree.py's whole run: cloud_or_ply (a GaussianCloud-like model or a PLY path) and its importance scores [P] (what
    lightgaussian.calculate_v_imp_score returns / imp_score.npz holds; None: all ones, --no_IS) -> the non-VQ mask, a codebook
    trained on the other rows, every row's code, and -- with `folder` -- the container load_vq reads. sh_dim: the leading SH
    columns that are quantised (default: all of them; the reference's --sh_degree 2 takes 27). -> dict(vq, non_vq_mask, all_feat,
    all_indice, losses, table, folder)"""
    if isinstance(cloud_or_ply, (str, os.PathLike)):
        from .model_io import load_ply
        cloud_or_ply = load_ply(cloud_or_ply, sh_degree)[0]
    table = feature_table(cloud_or_ply).to(device)
    P = table.shape[0]
    if sh_dim is None:
        sh_dim = table.shape[1] - 14
    if not 1 <= sh_dim <= min(MAX_D, table.shape[1] - 14):
        raise ValueError(f"quantize_model: sh_dim = {sh_dim} for a table of {table.shape[1]} columns")
    imp = torch.ones(P, device=device) if importance is None else torch.as_tensor(importance).detach().reshape(-1).float().to(device)
    if imp.shape[0] != P:
        raise ValueError(f"quantize_model: {P} Gaussians, {imp.shape[0]} importance scores")
    feats = table[:, 6:6 + sh_dim].contiguous()
    non_vq_mask = select_non_vq(imp, vq_ratio)
    vq_mask = ~non_vq_mask
    vq = VectorQuantize(dim=sh_dim, codebook_size=codebook_size, decay=0.8, commitment_weight=1.0, use_cosine_sim=False,
                        threshold_ema_dead_code=0, codebook=codebook).to(device)
    losses = train_codebook(feats[vq_mask].contiguous(), None if importance is None else imp[vq_mask], vq, iterations, chunk, k_expire,
                            indexes, generator)
    all_feat, all_indice = assign_all(feats, vq)
    if folder is not None:
        save_vq(folder, table, non_vq_mask, all_indice, vq._codebook.embed, sh_dim, vq_way)
    return dict(vq=vq, non_vq_mask=non_vq_mask, all_feat=all_feat, all_indice=all_indice, losses=losses, table=table, folder=folder)
