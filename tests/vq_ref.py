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
