"""Reference runs for fov3dgs_amd.optim.Adam, built from torch.optim.Adam alone (test infrastructure, not a test).

The contract of tests/test_optim_gpu.py: the truth is torch.optim.Adam in float64 from the same float32 inputs, the
yardstick is torch's own float32 Adam (foreach=False) against that truth, the metric is the relative L2 distance per tensor
(exp_avg, exp_avg_sq; the parameters relative to the distance they moved), and the HIP optimizer may be at most
CONTRACT (2) times torch-float32's distance away, on each of the three.

Rules for a row-sparse gradient:
  exact  Adam on grad.to_dense()
  lazy   take the Adam step, then put back p, exp_avg, exp_avg_sq of the rows that had no entry
"""
import math
from types import SimpleNamespace

import torch

from tests import parity_report

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ROW_SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
ATTRS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
         "rotation": "_rotation"}
# the reference's learning rates (fov3dgs/arguments/__init__.py, OptimizationParams)
TRAINING_ARGS = SimpleNamespace(position_lr_init=0.00016, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
LRS = {"xyz": TRAINING_ARGS.position_lr_init, "f_dc": TRAINING_ARGS.feature_lr, "f_rest": TRAINING_ARGS.feature_lr / 20.0,
       "opacity": TRAINING_ARGS.opacity_lr, "scaling": TRAINING_ARGS.scaling_lr, "rotation": TRAINING_ARGS.rotation_lr}
CONTRACT = 2.0


def make_params(P, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {n: torch.randn((P,) + ROW_SHAPES[n], generator=g, dtype=torch.float32) for n in NAMES}


def make_grads(P, steps, seed=1, visible=0.17):
    """Per step: (rows, {name: dense float32 gradient}). g = randn * exp(3 randn - 8) on a random `visible` fraction of the
    rows, zero elsewhere; |g| >= 1e-9 where it is not zero, so that g * g is a normal float32."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        rows = torch.nonzero(torch.rand(P, generator=g) < visible).flatten()
        grads = {}
        for n in NAMES:
            shape = (P,) + ROW_SHAPES[n]
            x = torch.randn(shape, generator=g) * torch.exp(3.0 * torch.randn(shape, generator=g) - 8.0)
            x = torch.where(x.abs() < 1e-9, torch.where(x < 0, -1e-9, 1e-9).to(x.dtype), x).float()
            d = torch.zeros(shape, dtype=torch.float32)
            d[rows] = x[rows]
            grads[n] = d
        out.append((rows, grads))
    return out


def to_row_sparse(dense, rows):
    """The rasterizer's gradient layout: torch.sparse_coo, one sparse dimension, coalesced."""
    return torch.sparse_coo_tensor(rows.unsqueeze(0), dense[rows], dense.shape, is_coalesced=True)


def groups_of(params, lrs=LRS):
    return [{"params": [params[n]], "lr": lrs[n], "name": n} for n in params]


def param_of(opt, name):
    for g in opt.param_groups:
        if g["name"] == name:
            return g["params"][0]
    raise KeyError(name)


def state_of(opt, device="cpu"):
    """{name: (p, exp_avg, exp_avg_sq)} as float64 copies on `device` (None moments before the first step of a parameter)."""
    out = {}
    for g in opt.param_groups:
        p = g["params"][0]
        st = opt.state.get(p, {})
        out[g["name"]] = tuple(None if t is None else t.detach().to(device, torch.float64)
                               for t in (p, st.get("exp_avg"), st.get("exp_avg_sq")))
    return out


class RefAdam:
    """torch.optim.Adam (foreach=False) over copies of `params` in `dtype` on `device`, constructed as the reference does:
    Adam(groups, lr=0.0, eps=1e-15)."""

    def __init__(self, params, dtype, device="cpu", lrs=LRS, eps=1e-15, betas=(0.9, 0.999)):
        self.dtype, self.device = dtype, device
        ps = {n: torch.nn.Parameter(p.detach().to(device, dtype).clone()) for n, p in params.items()}
        self.opt = torch.optim.Adam(groups_of(ps, lrs), lr=0.0, eps=eps, betas=betas, foreach=False)

    def step(self, grads, rule="dense"):
        """grads: {name: float32 dense or row-sparse tensor, or None}. rule: dense | exact | lazy."""
        saved = {}
        for n, g in grads.items():
            p = param_of(self.opt, n)
            if g is None:
                p.grad = None
                continue
            sparse = g.layout == torch.sparse_coo
            assert sparse or rule == "dense"
            if sparse and rule == "lazy":
                keep = torch.ones(p.shape[0], dtype=torch.bool, device=self.device)
                keep[g.coalesce().indices()[0].to(self.device)] = False
                st = self.opt.state.get(p, {})
                saved[n] = (keep, p.detach()[keep].clone(),
                            None if "exp_avg" not in st else st["exp_avg"][keep].clone(),
                            None if "exp_avg_sq" not in st else st["exp_avg_sq"][keep].clone())
            p.grad = (g.to_dense() if sparse else g).to(self.device, self.dtype)
        self.opt.step()
        with torch.no_grad():
            for n, (keep, p0, m0, v0) in saved.items():
                p = param_of(self.opt, n)
                st = self.opt.state[p]
                p[keep] = p0
                st["exp_avg"][keep] = 0 if m0 is None else m0
                st["exp_avg_sq"][keep] = 0 if v0 is None else v0
        for n in grads:
            param_of(self.opt, n).grad = None

    def state(self, device="cpu"):
        return state_of(self.opt, device)


def _rel(a, truth, ref=None):
    """|a - truth|_2 / |truth - ref|_2 (ref = 0 when None); absolute when the denominator is zero."""
    a, truth = a.double().flatten(), truth.double().flatten()
    den = torch.linalg.vector_norm(truth if ref is None else truth - ref.double().flatten()).item()
    num = torch.linalg.vector_norm(a - truth).item()
    return num / den if den > 0 else num


def distances(got, truth, start):
    """{name: (param, exp_avg, exp_avg_sq) distances to the float64 run}; the parameters relative to what they moved from
    `start` ({name: tensor})."""
    return {n: (_rel(got[n][0], truth[n][0], start[n]), _rel(got[n][1], truth[n][1]), _rel(got[n][2], truth[n][2]))
            for n in truth}


def check_contract(label, hip, f32, f64, start):
    """Records every ratio (the session's parity_report_gpu.json), prints it, then asserts the 2x contract on each of the three."""
    dh, dt = distances(hip, f64, start), distances(f32, f64, start)
    bad = []
    for n in f64:
        for k, what in enumerate(("param", "exp_avg", "exp_avg_sq")):
            h, t = dh[n][k], dt[n][k]
            ratio = h / t if t > 0 else (0.0 if h == 0 else math.inf)
            print(f"adam {label} {n}.{what}: hip {h:.3e} torch32 {t:.3e} ratio {ratio:.3f}")
            parity_report.record("adam", f"{label}/{n}.{what}", hip_dist=h, torch32_dist=t, ratio=ratio if math.isfinite(ratio) else -1.0)
            if not h <= CONTRACT * t:
                bad.append((n, what, h, t))
    assert not bad, f"{label}: farther than {CONTRACT}x torch-float32 from the float64 run: {bad}"
