"""Reference for the counting render (LightGaussian's global significance): the oracle's ORIGINAL blend replayed per pixel in
numpy, in the oracle's dtype and operation order (oracle/fovraster_oracle.c render_plain, the R0 branch), over the oracle's own
ranges / point_list / means2D / conic -- with one thing added, the two statements of renderCUDA_count (compress-diff-gaussian-
rasterization cuda_rasterizer/forward.cu:473-474) executed one pixel at a time: hits[g] += 1 for every (pixel, Gaussian) pair
that is accumulated.

All pixels of all tiles advance together, one list position per step. The replay validates itself against the oracle it
replays: n_contrib must be equal, final_T equal to 1e-6 (numpy's exp against libm's)."""
import numpy as np

from oracle import oracle as orc

TILE = 16


def replay(scene, cam, dtype=np.float32, fwd=None):
    """-> dict(hits int64 [P], n_contrib uint32 [H,W], final_T [H,W], saturated = pixels that finished early, longest = the longest
    tile list, fwd = the oracle's forward dict)."""
    real = np.dtype(dtype).type
    if fwd is None:
        fwd = orc.forward("original", scene, cam, dtype=dtype)
    W, H = int(cam["image_width"]), int(cam["image_height"])
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    T = gx * gy
    ranges = fwd["ranges"].astype(np.int64).reshape(T, 2)
    n = ranges[:, 1] - ranges[:, 0]
    plist = fwd["point_list"].astype(np.int64)
    mx, my = fwd["means2D"][:, 0].astype(dtype), fwd["means2D"][:, 1].astype(dtype)
    ca, cb, cc = (fwd["conic"][:, i].astype(dtype) for i in range(3))
    op = np.asarray(scene["opacities"], dtype=dtype).reshape(-1)
    P = op.shape[0]
    tiles = np.arange(T)
    lx, ly = np.meshgrid(np.arange(TILE), np.arange(TILE))
    pxi = (tiles % gx)[:, None] * TILE + lx.reshape(-1)[None, :]
    pyi = (tiles // gx)[:, None] * TILE + ly.reshape(-1)[None, :]
    inside = (pxi < W) & (pyi < H)
    pxf, pyf = pxi.astype(dtype), pyi.astype(dtype)
    # the constants as the oracle's C spells them: float literals widened to `real`, 1 / 255 divided in `real`
    half, c099, c1e4, inv255 = real(np.float32(-0.5)), real(np.float32(0.99)), real(np.float32(0.0001)), real(1.0) / real(255.0)
    Tr = np.ones((T, TILE * TILE), dtype=dtype)
    done = ~inside
    last = np.zeros((T, TILE * TILE), dtype=np.uint32)
    hits = np.zeros(P, dtype=np.int64)
    longest = int(n.max()) if T else 0
    with np.errstate(over="ignore", under="ignore"):
        for j in range(longest):
            act = np.nonzero(n > j)[0]
            g = plist[ranges[act, 0] + j]
            dx = mx[g][:, None] - pxf[act]
            dy = my[g][:, None] - pyf[act]
            power = half * (ca[g][:, None] * dx * dx + cc[g][:, None] * dy * dy) - cb[g][:, None] * dx * dy
            alpha = np.minimum(c099, op[g][:, None] * np.exp(power)).astype(dtype)
            live = ~done[act] & ~(power > 0) & ~(alpha < inv255)
            test_T = Tr[act] * (real(1.0) - alpha)
            sat = live & (test_T < c1e4)
            acc = live & ~sat
            done[act] |= sat
            Tr[act] = np.where(acc, test_T, Tr[act])
            last[act] = np.where(acc, np.uint32(j + 1), last[act])
            np.add.at(hits, g, acc.sum(axis=1))
    final_T = np.zeros((H, W), dtype=dtype)
    n_contrib = np.zeros((H, W), dtype=np.uint32)
    final_T[pyi[inside], pxi[inside]] = Tr[inside]
    n_contrib[pyi[inside], pxi[inside]] = last[inside]
    return dict(hits=hits, n_contrib=n_contrib, final_T=final_T, saturated=int((done & inside).sum()), longest=longest, fwd=fwd)


def validate(rep):
    """the replay against the oracle it replays"""
    fwd = rep["fwd"]
    assert np.array_equal(rep["n_contrib"], fwd["n_contrib"]), "replay: n_contrib differs from the oracle's"
    err = float(np.abs(rep["final_T"].astype(np.float64) - fwd["final_T"].astype(np.float64)).max())
    assert err <= 1e-6, f"replay: final_T differs from the oracle's by {err:.3g}"
    return err


def validated(scene, cam, dtype=np.float32):
    rep = replay(scene, cam, dtype)
    rep["final_T_err"] = validate(rep)
    return rep


def agreed_hits(scene, cam):
    """The hit counts on which the fp32 and the fp64 replay agree in every row (the edge scenes are chosen so that they do)."""
    r32, r64 = validated(scene, cam, np.float32), validated(scene, cam, np.float64)
    assert np.array_equal(r32["hits"], r64["hits"]), "fp32 and fp64 replays disagree: choose other scene parameters"
    return r32


def serial_fp32_score(hits, opacity):
    """important_score as ONE thread would accumulate it (forward.cu:474): opacity added hits[i] times in fp32"""
    hits = np.asarray(hits, dtype=np.int64)
    op = np.asarray(opacity, dtype=np.float32).reshape(-1)
    s = np.zeros_like(op)
    for k in range(int(hits.max()) if hits.size else 0):
        s = np.where(hits > k, (s + op).astype(np.float32), s)
    return s
