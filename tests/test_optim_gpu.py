"""fov3dgs_amd.optim.Adam on the MI355X against torch.optim.Adam (tests/adam_ref.py).

The contract: the truth is torch.optim.Adam in float64 from the same float32 inputs, the yardstick torch's own float32 Adam
(foreach=False) against that truth; relative L2 per tensor for exp_avg and exp_avg_sq, for the parameters relative to the
distance they moved; the HIP optimizer may be at most 2x torch-float32's distance away on each of the three. Where the library
is compared with itself (vector tails, exact vs dense, streams) the comparison is bit for bit. Every measured ratio goes to
the session's parity_report_gpu.json through tests/parity_report.record (one session's: profiles/optim_parity.json).

Measured on the MI355X (162 comparisons): parameters and exp_avg at 1.00x everywhere (exp_avg has torch's bits on CPU and GPU);
exp_avg_sq at 1.00x against torch's GPU Adam (S-6M: the same roundings) and 0.5x - 1.46x against torch's CPU Adam, whose
addcmul places one rounding differently: with gradients spanning eleven decades a moment tensor's relative L2 is the rounding
error of its few largest elements."""
import math

import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import optim
from fov3dgs_amd import synthetic as syn
from fov3dgs_amd.gaussian_renderer import render
from fov3dgs_amd.loss_utils import l1_ssim_loss
from tests import adam_ref
from tests.adam_ref import ATTRS, LRS, NAMES, RefAdam, check_contract, make_grads, make_params, state_of, to_row_sparse

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Pipe:
    debug = False


def _need_gpu():
    assert torch.cuda.is_available(), "this test needs the MI355X"


def _hip(params, lrs=LRS, eps=1e-15, sparse="exact"):
    ps = {n: torch.nn.Parameter(p.detach().to(DEV).clone()) for n, p in params.items()}
    return optim.Adam(adam_ref.groups_of(ps, lrs), lr=0.0, eps=eps, sparse=sparse)


def _hip_step(opt, grads):
    for n, g in grads.items():
        adam_ref.param_of(opt, n).grad = None if g is None else g.to(DEV)
    opt.step()


def _same_bits(a, b, what=""):
    for n in a:
        for k, f in enumerate(("param", "exp_avg", "exp_avg_sq")):
            assert torch.equal(a[n][k], b[n][k]), f"{what} {n}.{f}"


def _head(state, P):
    return {n: tuple(t[:P] for t in s) for n, s in state.items()}


def test_dense_parity_determinism_and_vector_tails():
    _need_gpu()
    P, steps = 20_000, 30
    ps, grads = make_params(P), make_grads(P, steps)
    hip, again = _hip(ps), _hip(ps)
    f32, f64 = RefAdam(ps, torch.float32), RefAdam(ps, torch.float64)
    for _, g in grads:
        _hip_step(hip, g)
        _hip_step(again, g)
        f32.step(g)
        f64.step(g)
    full = state_of(hip)
    check_contract("dense P=20000", full, f32.state(), f64.state(), ps)
    _same_bits(full, state_of(again), "second run")  # no atomics
    assert float(hip.state[adam_ref.param_of(hip, "xyz")]["step"]) == steps
    # vector tails, single-wave tensors: the arithmetic of an element does not depend on where it sits
    for Q in (1, 3, 63, 64, 65, 1000):
        sub = _hip({n: p[:Q] for n, p in ps.items()})
        for _, g in grads:
            _hip_step(sub, {n: x[:Q].contiguous() for n, x in g.items()})
        _same_bits(state_of(sub), _head(full, Q), f"first {Q} rows")


def test_learning_rate_schedule_zero_lr_group_and_eps():
    _need_gpu()
    P, steps = 3000, 12
    ps, grads = make_params(P, seed=3), make_grads(P, steps, seed=4)

    def build(make):
        groups = adam_ref.groups_of(make, LRS)
        for g in groups:
            if g["name"] == "opacity":
                del g["lr"]  # left at the constructor's lr = 0.0
        return groups
    hp = {n: torch.nn.Parameter(p.to(DEV).clone()) for n, p in ps.items()}
    hip = optim.Adam(build(hp), lr=0.0, eps=1e-15)
    refs = []
    for dt in (torch.float32, torch.float64):
        r = RefAdam(ps, dt)
        for g in r.opt.param_groups:
            if g["name"] == "opacity":
                g["lr"] = 0.0
        refs.append(r)
    assert hip.param_groups[3]["name"] == "opacity" and hip.param_groups[3]["lr"] == 0.0
    for it, (_, g) in enumerate(grads):
        lr = 0.00016 * math.exp(-0.3 * it)  # update_learning_rate writes group["lr"] of xyz every iteration
        for o in (hip, refs[0].opt, refs[1].opt):
            for grp in o.param_groups:
                if grp["name"] == "xyz":
                    grp["lr"] = lr
        _hip_step(hip, g)
        for r in refs:
            r.step(g)
    got = state_of(hip)
    check_contract("schedule", got, refs[0].state(), refs[1].state(), ps)
    assert torch.equal(got["opacity"][0], ps["opacity"].double())  # lr = 0: bit for bit
    assert got["opacity"][1].abs().max() > 0 and got["opacity"][2].abs().max() > 0  # while its moments advance
    # eps is honoured: p = 0, |g| = 1e-9, step 1 -> m / (1-b1) = g, sqrt(v / (1-b2)) = |g|: every element moves by lr
    # (with eps = 1e-8 hard-coded it would move by about lr / 11)
    lr = 0.01
    z = torch.nn.Parameter(torch.zeros(1000, 3, device=DEV))
    o = optim.Adam([{"params": [z], "lr": lr, "name": "xyz"}], lr=0.0, eps=1e-15)
    sign = torch.where(torch.arange(3000, device=DEV).reshape(1000, 3) % 2 == 0, 1.0, -1.0)
    z.grad = 1e-9 * sign
    o.step()
    move = (z.detach() * -sign).double().cpu()
    assert ((move - lr).abs() <= 1e-5 * lr).all(), (move.min().item(), move.max().item())


def test_zero_gradient_rows():
    _need_gpu()
    P = 1000
    ps = make_params(P, seed=5)
    rows, g = make_grads(P, 1, seed=6)[0]
    zero = torch.ones(P, dtype=torch.bool)
    zero[rows] = False
    assert zero.any() and (~zero).any()
    hip = _hip(ps)
    _hip_step(hip, g)
    got = state_of(hip)
    for n in NAMES:
        assert torch.equal(got[n][0][zero], ps[n][zero].double()), n  # bit-unchanged at step 1
        assert not got[n][1][zero].any() and not got[n][2][zero].any(), n  # moments exactly zero
        assert not torch.equal(got[n][0][~zero], ps[n][~zero].double()), n
    for _ in range(3):
        _hip_step(hip, {n: torch.zeros_like(x) for n, x in g.items()})
    assert all(torch.isfinite(t).all() for s in state_of(hip).values() for t in s)


def _cloud(P, seed=1, opacity_shift=0.0):
    c = syn.scene_bicycle_scale(P=P, seed=seed, scale_log_mean=math.log(0.05))
    c._opacity = c._opacity + opacity_shift
    c = c.to(DEV).requires_grad_(True)
    c.fuse_activations = True   # raw parameters: every rasterizer input is a leaf
    return c


def _cloud_params(c):
    return {n: getattr(c, ATTRS[n]) for n in NAMES}


def _backward(cloud, cam, bg, target):
    for p in cloud.parameters():
        p.grad = None
    out = render(cam, cloud, Pipe(), bg, cuda_type="pcheck_obb_sum")
    loss = l1_ssim_loss(out["render"], target, 0.2)
    loss.backward()
    return loss


def _uncoalesced(g):
    """The same gradient as unsorted entries plus entries of zeros for some rows (sums are exact: v + 0)."""
    g = g.coalesce()
    rows, vals = g.indices()[0], g.values()
    perm = torch.randperm(rows.numel(), device=rows.device)
    extra = rows[:: 7]
    u = torch.sparse_coo_tensor(torch.cat((rows[perm], extra)).unsqueeze(0), torch.cat((vals[perm], torch.zeros_like(vals[:: 7]))), g.shape)
    assert not u.is_coalesced()
    return u


def test_exact_is_the_dense_step_on_to_dense_bit_for_bit():
    _need_gpu()
    torch.manual_seed(0)
    P = 50_000
    cloud = _cloud(P)
    cloud.row_sparse_grads = True
    bg = torch.zeros(3, device=DEV)
    a = optim.Adam(optim.reference_param_groups(cloud, adam_ref.TRAINING_ARGS), lr=0.0, eps=1e-15)  # sparse="exact" is the default
    start = {n: p.detach().cpu().clone() for n, p in _cloud_params(cloud).items()}
    b, c, d = _hip(start), _hip(start), _hip(start)
    assert a.exact_lookup == "map"
    d.exact_lookup = "search"  # the lookup without scratch: a binary search in the rows
    for it in range(5):
        cam = syn.camera_ring(it, width=192, height=128).to(DEV)
        _backward(cloud, cam, bg, torch.rand(3, 128, 192, device=DEV))
        grads = {n: p.grad for n, p in _cloud_params(cloud).items()}
        assert all(g.is_sparse and g.is_coalesced() for g in grads.values())  # the rasterizer's flag survives autograd
        n_rows = grads["xyz"].coalesce().indices().shape[1]
        assert 100 < n_rows < P
        _hip_step(b, {n: g.to_dense() for n, g in grads.items()})
        _hip_step(c, {n: _uncoalesced(g) for n, g in grads.items()})
        _hip_step(d, {n: g.coalesce() for n, g in grads.items()})
        a.step()
        sa = state_of(a)
        _same_bits(sa, state_of(b), f"exact vs dense, step {it}")
        _same_bits(sa, state_of(c), f"uncoalesced input, step {it}")
        _same_bits(sa, state_of(d), f"binary search, step {it}")
    assert not torch.equal(sa["xyz"][0], start["xyz"].double())


def test_lazy_mode():
    _need_gpu()
    P, steps = 20_000, 30
    ps, grads = make_params(P), make_grads(P, steps)
    hip = _hip(ps, sparse="lazy")
    f32, f64 = RefAdam(ps, torch.float32), RefAdam(ps, torch.float64)
    for rows, g in grads:
        sp = {n: to_row_sparse(x, rows) for n, x in g.items()}
        before = state_of(hip)
        _hip_step(hip, sp)
        after = state_of(hip)
        keep = torch.ones(P, dtype=torch.bool)
        keep[rows] = False
        for n in NAMES:  # rows not listed keep their bits (before the first step there are no moments: zeros)
            assert torch.equal(after[n][0][keep], before[n][0][keep]), n
            for k in (1, 2):
                assert torch.equal(after[n][k][keep], before[n][k][keep] if before[n][k] is not None else torch.zeros_like(after[n][k][keep])), n
        f32.step(sp, rule="lazy")
        f64.step(sp, rule="lazy")
    check_contract("lazy P=20000", state_of(hip), f32.state(), f64.state(), ps)
    # every row listed: the dense step, bit for bit
    Q = 1000
    sub = {n: p[:Q] for n, p in ps.items()}
    lazy_all, dense = _hip(sub, sparse="lazy"), _hip(sub)
    every = torch.arange(Q)
    for _, g in grads[:5]:
        gq = {n: x[:Q].contiguous() for n, x in g.items()}
        _hip_step(lazy_all, {n: to_row_sparse(x, every) for n, x in gq.items()})
        _hip_step(dense, gq)
    _same_bits(state_of(lazy_all), state_of(dense), "lazy with every row listed")


# ---- the reference's model surgery (GaussianModel.replace_tensor_to_optimizer / _prune_optimizer / cat_tensors_to_optimizer,
# gaussian_model.py:609-686), restated: they reach into optimizer.state and group["params"][0]

def _install(opt, group, tensor, state):
    opt.state.pop(group["params"][0], None)
    group["params"][0] = torch.nn.Parameter(tensor.requires_grad_(True))
    if state is not None:
        opt.state[group["params"][0]] = state


def prune_optimizer(opt, keep):
    for group in opt.param_groups:
        old = group["params"][0]
        m = keep.to(old.device)
        st = opt.state.get(old)
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][m], st["exp_avg_sq"][m]
        _install(opt, group, old.detach()[m], st)


def cat_tensors_to_optimizer(opt, new):
    for group in opt.param_groups:
        assert len(group["params"]) == 1
        old = group["params"][0]
        ext = new[group["name"]].to(old.device, old.dtype)
        st = opt.state.get(old)
        if st is not None:
            st["exp_avg"] = torch.cat((st["exp_avg"], torch.zeros_like(ext)), dim=0)
            st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
        _install(opt, group, torch.cat((old.detach(), ext), dim=0), st)


def replace_tensor_to_optimizer(opt, tensor, name):
    for group in opt.param_groups:
        if group["name"] == name:
            old = group["params"][0]
            t = tensor.to(old.device, old.dtype)
            st = opt.state.get(old)
            st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(t), torch.zeros_like(t)
            _install(opt, group, t, st)


def test_model_surgery_between_steps():
    _need_gpu()
    P = 5000
    ps = make_params(P, seed=7)
    hip = _hip(ps)
    f32, f64 = RefAdam(ps, torch.float32), RefAdam(ps, torch.float64)
    opts = (hip, f32.opt, f64.opt)
    start = {n: p.clone() for n, p in ps.items()}
    g = torch.Generator().manual_seed(8)

    def step(seed):
        Pn = adam_ref.param_of(hip, "xyz").shape[0]
        _, grads = make_grads(Pn, 1, seed=seed)[0]
        _hip_step(hip, grads)
        f32.step(grads)
        f64.step(grads)
    step(10)
    keep = torch.rand(P, generator=g) >= 0.3
    for o in opts:
        prune_optimizer(o, keep)
    start = {n: p[keep] for n, p in start.items()}
    step(11)
    new = make_params(P // 10, seed=9)
    for o in opts:
        cat_tensors_to_optimizer(o, new)
    start = {n: torch.cat((start[n], new[n])) for n in start}
    assert adam_ref.param_of(hip, "f_rest").shape == (int(keep.sum()) + P // 10, 15, 3)
    step(12)
    # reset_opacity: min(opacity, logit(0.01)), moments cleared -- every optimizer gets the same float32 tensor
    reset = torch.minimum(adam_ref.param_of(hip, "opacity").detach().cpu(), torch.full((1,), math.log(0.01 / 0.99)))
    for o in opts:
        replace_tensor_to_optimizer(o, reset.clone(), "opacity")
    start["opacity"] = reset.clone()
    step(13)
    for n in NAMES:
        assert float(hip.state[adam_ref.param_of(hip, n)]["step"]) == 4
    check_contract("surgery", state_of(hip), f32.state(), f64.state(), start)


@pytest.mark.parametrize("mode", ("dense", "exact", "lazy"))
def test_training_loop(mode):
    _need_gpu()
    torch.manual_seed(1)
    P, W, H, iters = 50_000, 192, 128, 20
    bg = torch.zeros(3, device=DEV)
    cams = [syn.camera_ring(i, width=W, height=H).to(DEV) for i in range(8)]
    truth = _cloud(P)
    with torch.no_grad():
        targets = [render(c, truth, Pipe(), bg, cuda_type="pcheck_obb_sum")["render"].clone() for c in cams]
    del truth
    cloud = _cloud(P, opacity_shift=-2.0)  # the same scene, far too transparent: the opacities have to come back up
    cloud.row_sparse_grads = mode != "dense"
    opt = optim.Adam(optim.reference_param_groups(cloud, adam_ref.TRAINING_ARGS), lr=0.0, eps=1e-15,
                     sparse="lazy" if mode == "lazy" else "exact")
    assert [g["name"] for g in opt.param_groups] == list(NAMES)
    start = {n: p.detach().cpu().clone() for n, p in _cloud_params(cloud).items()}
    f32, f64 = RefAdam(start, torch.float32), RefAdam(start, torch.float64)
    losses = []
    for it in range(iters):
        loss = _backward(cloud, cams[it % 8], bg, targets[it % 8])
        if it == 3:
            cloud._rotation.grad = None  # skipped: its step does not advance
        grads = {n: (None if p.grad is None else p.grad.detach().cpu()) for n, p in _cloud_params(cloud).items()}
        assert all(g is None or g.is_sparse == (mode != "dense") for g in grads.values())
        opt.step()
        losses.append(float(loss.detach()))
        # the reference runs are fed the same gradient tensors: never re-rendered, so no discrete blend decision can diverge
        rule = "dense" if mode == "dense" else mode
        f32.step(grads, rule=rule)
        f64.step(grads, rule=rule)
    steps = {n: float(opt.state[getattr(cloud, ATTRS[n])]["step"]) for n in NAMES}
    assert steps == {n: (iters - 1 if n == "rotation" else iters) for n in NAMES}, steps
    print(f"adam train[{mode}] loss first5 {sum(losses[:5]) / 5:.5f} last5 {sum(losses[-5:]) / 5:.5f}")
    check_contract(f"train {mode}", state_of(opt), f32.state(), f64.state(), start)
    assert sum(losses[-5:]) / 5 < sum(losses[:5]) / 5, losses


def test_streams_and_no_synchronisation():
    _need_gpu()
    P = 4000
    ps, grads = make_params(P, seed=11), make_grads(P, 4, seed=12)
    a, b = _hip(ps), _hip(ps)
    s = torch.cuda.Stream(device=DEV)
    for _, g in grads:
        _hip_step(a, g)
        for n, x in g.items():
            adam_ref.param_of(b, n).grad = x.to(DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            b.step()
        s.synchronize()
    _same_bits(state_of(a), state_of(b), "side stream")
    # a warmed-up step: no device synchronisation, no host <-> device copy
    dev_grads = {n: x.to(DEV) for n, x in grads[0][1].items()}
    sparse = _hip(ps, sparse="lazy")
    rows = grads[0][0]
    sp = {n: to_row_sparse(x, rows).to(DEV) for n, x in grads[0][1].items()}
    _hip_step(sparse, sp)
    torch.cuda.synchronize()
    for n in NAMES:
        adam_ref.param_of(a, n).grad = dev_grads[n]
        adam_ref.param_of(sparse, n).grad = sp[n]
    torch.cuda.set_sync_debug_mode("error")
    try:
        a.step()
        sparse.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ("dense", "lazy"))
def test_full_size_s6m(mode):
    """6 M x 59 floats: the size at which grid capping and 64-bit element offsets matter. Truth and yardstick are
    torch.optim.Adam in float64 / float32 on the GPU. Three steps: dense gradients of the ring cameras 0..2, or lazy on the
    rows of camera_ring(0)'s backward."""
    _need_gpu()
    torch.manual_seed(2)
    W, H = 1920, 1080
    bg = torch.zeros(3, device=DEV)
    cloud = syn.scene_bicycle_scale().to(DEV).requires_grad_(True)
    cloud.fuse_activations = True
    cloud.row_sparse_grads = mode == "lazy"
    P = len(cloud)
    assert P == 6_000_000
    opt = optim.Adam(optim.reference_param_groups(cloud, adam_ref.TRAINING_ARGS), lr=0.0, eps=1e-15, sparse="lazy")
    start = {n: p.detach().clone() for n, p in _cloud_params(cloud).items()}
    f32, f64 = RefAdam(start, torch.float32, device=DEV), RefAdam(start, torch.float64, device=DEV)
    for it in range(3):
        cam = syn.camera_ring(0 if mode == "lazy" else it, width=W, height=H).to(DEV)
        _backward(cloud, cam, bg, torch.rand(3, H, W, device=DEV))
        grads = {n: p.grad for n, p in _cloud_params(cloud).items()}
        if mode == "lazy":
            n_rows = grads["xyz"].coalesce().indices().shape[1]
            assert 10_000 < n_rows < P
        opt.step()
        f32.step(grads, rule=mode)
        f64.step(grads, rule=mode)
    check_contract(f"S-6M {mode}", state_of(opt, device=DEV), f32.state(device=DEV), f64.state(device=DEV), start)
