"""VecTree vector quantisation restated in float64 numpy (LightGaussian/vectree/vq.py:262-299, :405-407; vectree.py:196-204), and the
acceptance rule of the assignment. Not a port: every formula is written from the reference's lines as the issue lists them."""
import numpy as np

DECAY, EPS = 0.8, 1e-5


def sq_dists(x, e, chunk=256):
    """float64 [n, K]: ||x_i - e_c||^2 from the differences"""
    x, e = np.asarray(x, np.float64), np.asarray(e, np.float64)
    out = np.empty((x.shape[0], e.shape[0]))
    for lo in range(0, x.shape[0], chunk):
        d = x[lo:lo + chunk, None, :] - e[None, :, :]
        out[lo:lo + chunk] = np.einsum("nkd,nkd->nk", d, d)
    return out


def bound(x, e):
    """B_i = 2 (D + 2) 2^-24 (||x_i|| + max_c ||e_c||)^2: what a (D+1)-term fp32 fmaf chain can do to the difference of two scores"""
    x, e = np.asarray(x, np.float64), np.asarray(e, np.float64)
    D = x.shape[1]
    return 2.0 * (D + 2) * 2.0 ** -24 * (np.linalg.norm(x, axis=1) + np.linalg.norm(e, axis=1).max()) ** 2


def assignment(x, e):
    """-> (ind: the float64 argmin, lowest index on a tie; ambiguous bool [n]: the second-best d^2 lies within B_i of the best;
    allowed bool [n, K]: the codes within B_i of the best; d2)"""
    d2 = sq_dists(x, e)
    ind = d2.argmin(axis=1)
    best = d2[np.arange(d2.shape[0]), ind]
    B = bound(x, e)
    allowed = d2 <= (best + B)[:, None]
    return ind, allowed.sum(axis=1) > 1, allowed, d2


def check_assignment(got, x, e, cap):
    """The rule: equal to the float64 argmin on every non-ambiguous row, one of the codes within B_i on an ambiguous one; the
    ambiguous share is at most `cap` (so the test cannot pass vacuously). -> the share"""
    got = np.asarray(got).astype(np.int64)
    ind, amb, allowed, _ = assignment(x, e)
    share = float(amb.mean())
    assert share <= cap, f"ambiguous share {share} > {cap}"
    bad = np.nonzero(~amb & (got != ind))[0]
    assert bad.size == 0, f"{bad.size} non-ambiguous rows differ, first {bad[:5]}: got {got[bad[:5]]}, float64 {ind[bad[:5]]}"
    assert (got >= 0).all() and (got < e.shape[0]).all()
    assert allowed[np.arange(got.shape[0]), got].all(), "an ambiguous row took a code outside its bound"
    return share


def train_step(x, w, embed, cluster_size, ind=None, decay=DECAY, eps=EPS, commitment_weight=1.0):
    """One training step in float64 -> dict(ind, quantize, loss, embed, cluster_size). ind: the assignment to use (else the float64 argmin)"""
    x, embed, cs = np.asarray(x, np.float64), np.asarray(embed, np.float64), np.asarray(cluster_size, np.float64)
    n, K = x.shape[0], embed.shape[0]
    if ind is None:
        ind = sq_dists(x, embed).argmin(axis=1)
    ind = np.asarray(ind).astype(np.int64)
    wp = np.ones(n) if w is None else np.asarray(w, np.float64) * n / np.asarray(w, np.float64).sum()
    quantize = embed[ind]
    batch = np.bincount(ind, weights=wp, minlength=K)
    cs = decay * cs + (1 - decay) * batch
    esum = np.zeros_like(embed)
    np.add.at(esum, ind, wp[:, None] * x)
    smoothed = (cs + eps) / (cs.sum() + K * eps) * cs.sum()
    new_embed = decay * embed + (1 - decay) * esum / smoothed[:, None]
    loss = commitment_weight * np.mean((quantize - x) ** 2)
    return dict(ind=ind, quantize=quantize, loss=loss, embed=new_embed, cluster_size=cs)


def stable_smallest(v, k):
    return np.argsort(np.asarray(v), kind="stable")[:k]


def replace(embed, cluster_size, x, w, k):
    """vectree.py:202-204 with ties to the lowest index: -> (embed, codes, rows)"""
    K = embed.shape[0]
    if k > K:
        k = 0
    codes = stable_smallest(cluster_size, k)
    rows = stable_smallest(-np.asarray(w), k)
    embed = np.array(embed, copy=True)
    embed[codes] = np.asarray(x)[rows]
    return embed, codes, rows


def pack_bits(values, bits):
    v = np.asarray(values).astype(np.int64).reshape(-1)
    m = (v[:, None] >> np.arange(bits - 1, -1, -1)[None, :]) & 1
    return np.packbits(m.astype(bool).reshape(-1))


# ---- the codebook step as csrc/vq.hip performs it, operation for operation (float32) ---------------------------------------------
U = 2.0 ** -24
TILE = 1024  # rows per counting-sort tile (VQ_TILE), and the width of k_vq_sum's / k_vq_select's one workgroup


def fixed_order_sum(v):
    """k_vq_sum: thread t adds elements t, t + 1024, ... in double, then the 512 ... 1 tree. -> the double (the kernel rounds it to float once)"""
    v = np.asarray(v, np.float32).astype(np.float64)
    pad = np.zeros((v.shape[0] + TILE - 1) // TILE * TILE)
    pad[:v.shape[0]] = v
    sh = np.zeros(TILE)
    for stride in pad.reshape(-1, TILE):
        sh = sh + stride
    m = TILE // 2
    while m >= 1:
        sh[:m] = sh[:m] + sh[m:2 * m]
        m //= 2
    return sh[0]


def sort_rows(ind, K):
    """The stable counting sort: -> (perm int64 [n]: rows by code, ascending row position inside a code; seg int64 [K + 1])"""
    ind = np.asarray(ind).astype(np.int64)
    seg = np.concatenate([[0], np.cumsum(np.bincount(ind, minlength=K))])
    return np.argsort(ind, kind="stable"), seg


def emulate_update(x, w, ind, embed, cs, decay=DECAY, eps=EPS, perm=None, seg=None, defect=None):
    """fr_vq_update in numpy float32, one rounding per operation in the kernels' order. x [n, D] and w [n] (or None) are the rows of
    the call (already gathered through `rows`). perm / seg: another sort than sort_rows' and defect="ema" (decay and 1 - decay
    exchanged in the cluster-size EMA) exist for the tests that show a judge rejecting a defective restatement.
    -> dict(embed, cluster_size, embed_sum, batch, smoothed, wp), float32"""
    f = np.float32
    x, embed, cs = np.asarray(x, f), np.asarray(embed, f), np.asarray(cs, f)
    n, K = x.shape[0], embed.shape[0]
    decay, eps = f(decay), f(eps)
    omd = f(1.0 - float(decay))
    if perm is None:
        perm, seg = sort_rows(ind, K)
    if w is None:
        wp = np.ones(n, f)
    else:
        w = np.asarray(w, f)
        wp = (w * f(n)) / f(fixed_order_sum(w))
    seg = np.minimum(np.asarray(seg, np.int64), n)
    length = np.maximum(seg[1:] - seg[:-1], 0)
    acc, bs = np.zeros(embed.shape, f), np.zeros(K, f)
    for j in range(int(length.max())):  # the j-th member of every code that has one: acc = fl(acc + fl(w' x)), bs = fl(bs + w')
        c = np.nonzero(length > j)[0]
        i = perm[seg[c] + j]
        acc[c] = acc[c] + wp[i][:, None] * x[i]
        bs[c] = bs[c] + wp[i]
    if defect == "ema":
        new_cs = cs * omd + decay * bs
    else:
        new_cs = cs * decay + omd * bs
    S = f(fixed_order_sum(new_cs))
    k_eps = f(float(K) * float(eps))
    with np.errstate(all="ignore"):  # (a state that sums to nothing divides by zero here as it does on the device)
        smoothed = ((new_cs + eps) / (S + k_eps)) * S
        new_embed = embed * decay + omd * (acc / smoothed[:, None])
    for a in (wp, acc, bs, new_cs, smoothed, new_embed):
        assert a.dtype == f
    return dict(embed=new_embed, cluster_size=new_cs, embed_sum=acc, batch=bs, smoothed=smoothed, wp=wp)


def update_bounds(x, w, ind, embed, cs, decay=DECAY, eps=EPS):
    """First-order bounds of emulate_update's arithmetic against train_step's float64 values (derived, not measured; u = 2^-24, m_c the
    members of code c, sums of magnitudes in float64). A sum of m terms, each a rounded product of a w' that itself carries two
    roundings, added one at a time: (m - 1) + 1 + 2 = m + 2 roundings on sum w', one more for the product w' x.
      batch         (m_c + 2) u sum w'
      cluster_size  (1 - decay) bound(batch) + 3 u |cs_new|                         (two products and a sum)
      embed_sum     E = (m_c + 3) u sum w' |x|
      smoothed      relative: bound(cs) / (cs + eps) + 6 u                          (S carries the relative error of its terms at most)
      embed         (1 - decay) / smoothed (E + |esum| rel(smoothed)) + 3 u (decay |e| + (1 - decay) |esum| / smoothed)
    -> dict(batch [K], cluster_size [K], embed_sum [K, D], smoothed_rel [K], embed [K, D])"""
    x, embed, cs = np.asarray(x, np.float64), np.asarray(embed, np.float64), np.asarray(cs, np.float64)
    n, K = x.shape[0], embed.shape[0]
    ind = np.asarray(ind).astype(np.int64)
    wp = np.ones(n) if w is None else np.asarray(w, np.float64) * n / np.asarray(w, np.float64).sum()
    m = np.bincount(ind, minlength=K)
    sum_wp = np.bincount(ind, weights=wp, minlength=K)
    batch = (m + 2) * U * sum_wp
    new_cs = decay * cs + (1 - decay) * sum_wp
    b_cs = (1 - decay) * batch + 3 * U * np.abs(new_cs)
    mag, esum = np.zeros_like(embed), np.zeros_like(embed)
    np.add.at(mag, ind, wp[:, None] * np.abs(x))
    np.add.at(esum, ind, wp[:, None] * x)
    E = (m + 3)[:, None] * U * mag
    rel = b_cs / (new_cs + eps) + 6 * U
    smoothed = (new_cs + eps) / (new_cs.sum() + K * eps) * new_cs.sum()
    b_embed = ((1 - decay) / smoothed[:, None] * (E + np.abs(esum) * rel[:, None])
               + 3 * U * (decay * np.abs(embed) + (1 - decay) * np.abs(esum) / smoothed[:, None]))
    return dict(batch=batch, cluster_size=b_cs, embed_sum=E, smoothed_rel=rel, embed=b_embed)
