"""References for the nearest-neighbour tests (test_knn_cpu.py, test_knn_gpu.py): the exact k-d tree in knn_exact.c and
an all-pairs numpy restatement, both in fp32 with the contract's operation order (include/fovraster.h, fr_knn_mean_dist2)."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FLT_MAX = np.float32(np.finfo(np.float32).max)


def build_exact(tmpdir):
    """Compile knn_exact.c into `tmpdir`; -> path of the program."""
    exe = os.path.join(str(tmpdir), "knn_exact")
    subprocess.check_call(["gcc", "-O2", "-fopenmp", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "knn_exact.c"), "-lm"])
    return exe


def run_exact(exe, points, tmpdir):
    """points float32 [P,3] (finite) -> float32 [P] of the k-d tree reference."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    assert np.isfinite(pts).all()
    src, dst = os.path.join(str(tmpdir), "knn_in.bin"), os.path.join(str(tmpdir), "knn_out.bin")
    with open(src, "wb") as f:
        f.write(np.int32(pts.shape[0]).tobytes())
        f.write(pts.tobytes())
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", str(min(16, os.cpu_count() or 1)))
    subprocess.check_call([exe, src, dst], env=env)
    out = np.fromfile(dst, dtype=np.float32)
    os.remove(src)
    os.remove(dst)
    assert out.shape == (pts.shape[0],)
    return out


def brute_force(points):
    """All pairs in numpy fp32, same order: d = (dx*dx + dy*dy) + dz*dz, three smallest over j != i padded with FLT_MAX."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    P = p.shape[0]
    out = np.empty(P, np.float32)
    for s in range(0, P, 512):
        q = p[s:s + 512]
        dx = p[None, :, 0] - q[:, None, 0]
        dy = p[None, :, 1] - q[:, None, 1]
        dz = p[None, :, 2] - q[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        rows = np.arange(q.shape[0])
        d[rows, s + rows] = FLT_MAX  # self: one more missing neighbour, which the FLT_MAX padding already stands for
        d = np.concatenate([d, np.full((q.shape[0], 3), FLT_MAX, np.float32)], axis=1)
        b = np.sort(d, axis=1)[:, :3]
        with np.errstate(over="ignore"):  # P <= 2: FLT_MAX + FLT_MAX = inf, as in the contract
            out[s:s + 512] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3.0)
    return out


def uniform_cloud(P, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=(P, 3)).astype(np.float32)


def degenerate_clouds(P=5000, seed=7):
    """name -> float32 [P,3]: the sets on which a spatial search most easily goes wrong."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, size=(P, 3)).astype(np.float32)
    dup = base.copy()
    k = P // 10
    dup[rng.choice(P, k, replace=False)] = base[rng.choice(P, k, replace=False)]
    plane = base.copy()
    plane[:, 2] = np.float32(0.25)
    t = rng.uniform(-1, 1, size=(P, 1)).astype(np.float32)
    line = (t * np.array([[0.3, -0.7, 0.2]], np.float32) + np.array([[0.1, 0.2, 0.3]], np.float32)).astype(np.float32)
    thin = np.stack([rng.uniform(0, 1e3, P), rng.uniform(0, 1e-6, P), rng.uniform(0, 1e3, P)], 1).astype(np.float32)
    offset = (base + np.float32(1e4)).astype(np.float32)
    return {"identical": np.tile(np.array([[0.5, -2.0, 3.0]], np.float32), (P, 1)), "duplicates_10pct": dup,
            "z_const": plane, "collinear": line, "thin_axis_1e-6": thin, "offset_1e4": offset}
