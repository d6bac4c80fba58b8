"""The scale-decay loss and the opacity cap of the pruning loop on the MI355X (csrc/prune_step.hip).

Sizes: one thread per row in workgroups of 256 = four waves of 64, so P = 1, 63, 64, 65 (a wave's edge), 257 (a second workgroup
of one row) and 4097 (seventeen per-workgroup sums for the one-workgroup finish).

scale_decay_loss is held to the reference's expression (prune.py:257-261) under torch.autograd in float64 on the CPU, from the
same fp32 inputs, at rtol 1e-6 for the value and for every gradient element: the terms are non-negative (no cancellation) and
each carries a few fp32 ulps, the exp included. The cap is held to bits: float32(logit(max)) evaluated in float64 within 1 ulp on
the capped rows, the input's bits elsewhere."""
import math

import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import optim, pruning
from fov3dgs_amd import synthetic as syn
from fov3dgs_amd.gaussian_renderer import render
from tests import prune_ref
from tests.adam_ref import ATTRS, NAMES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 63, 64, 65, 257, 4097)
RTOL = 1e-6


class Pipe:
    debug = False


def _need_gpu():
    assert torch.cuda.is_available(), "this test needs the MI355X"


# ---- scale decay -----------------------------------------------------------------------------------------------------
def scale_inputs(P, low_counts=False):
    """-> (log-scales fp32 [P,3], counts int32 [P]) on the CPU. Counts: 5, 0, 4 and 2^20 first, then 0..40; rows 10..12 (when
    there are that many) are a two-way tie in columns 0 and 1, a two-way tie in columns 1 and 2 above column 0, and a three-way
    tie, each with a count above the threshold. low_counts: every count is 0..4."""
    g = torch.Generator().manual_seed(100 + P)
    raw = 0.7 * torch.randn(P, 3, generator=g) - 3.0
    counts = torch.randint(0, 41, (P,), generator=g, dtype=torch.int32)
    special = torch.tensor([5, 0, 4, 2 ** 20], dtype=torch.int32)
    counts[:min(P, 4)] = special[:min(P, 4)]
    if P > 12:
        raw[10] = torch.tensor([-2.5, -2.5, -4.0])
        raw[11] = torch.tensor([-4.0, -2.25, -2.25])
        raw[12] = torch.tensor([-3.0, -3.0, -3.0])
        counts[10:13] = torch.tensor([9, 17, 6], dtype=torch.int32)
    if low_counts:
        counts = counts % 5
    return raw, counts


def reference(x32, counts, raw, factor=1.0):
    """prune.py:258-260 in float64 under torch.autograd -> (value, gradient [P,3]) as numpy float64"""
    x = x32.double().requires_grad_(True)
    scale = torch.exp(x) if raw else x
    gs_count = counts.long()
    scale_max, _ = torch.max(scale, dim=1)
    scale_loss = (scale_max * (gs_count - 4) * (gs_count > 4)).mean()
    (scale_loss * factor).backward()
    return scale_loss.item(), x.grad.numpy()


def fused(x32, counts, raw, factor=None, **kw):
    x = x32.to(DEV).requires_grad_(True)
    loss = pruning.scale_decay_loss(x, counts.to(DEV), raw=raw, **kw)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.device == x.device
    (loss if factor is None else loss * factor).backward()
    return loss.detach().cpu(), x.grad.cpu()


@pytest.mark.parametrize("raw", (False, True), ids=("activated", "raw"))
@pytest.mark.parametrize("P", SIZES)
def test_scale_decay_matches_the_reference_expression(P, raw):
    _need_gpu()
    logs, counts = scale_inputs(P)
    x32 = logs if raw else torch.exp(logs)
    assert int(counts[0]) == 5 and (P < 4 or counts[:4].tolist() == [5, 0, 4, 2 ** 20])
    want, want_grad = reference(x32, counts, raw)
    got, grad = fused(x32, counts, raw)
    print(f"P={P} raw={raw}: value {got.item()!r} (float64 {want!r}), relative {abs(got.item() / want - 1):.3g}; "
          f"worst gradient element {np.max(np.abs(grad.double().numpy() - want_grad) / np.maximum(np.abs(want_grad), 1e-300)):.3g}")
    assert want > 0
    np.testing.assert_allclose(got.item(), want, rtol=RTOL, atol=0)
    assert grad.shape == (P, 3) and grad.dtype == torch.float32
    np.testing.assert_allclose(grad.double().numpy(), want_grad, rtol=RTOL, atol=0)
    # rows at or under the threshold: exactly 0; the others: one non-zero column
    low = counts <= 4
    assert (grad[low] == 0).all() and ((grad[~low] != 0).sum(1) == 1).all()
    if P > 12:  # ties go to the lowest column, torch.max's documented index
        assert grad[10, 0] > 0 and grad[10, 1] == 0 and grad[10, 2] == 0
        assert grad[11, 0] == 0 and grad[11, 1] > 0 and grad[11, 2] == 0
        assert grad[12, 0] > 0 and grad[12, 1] == 0 and grad[12, 2] == 0
    # an upstream factor scales the gradient (it is read on the device), the value stays
    want3, want_grad3 = reference(x32, counts, raw, 3.0)
    got3, grad3 = fused(x32, counts, raw, 3.0)
    assert torch.equal(got3, got) and want3 == want
    np.testing.assert_allclose(grad3.double().numpy(), want_grad3, rtol=RTOL, atol=0)
    np.testing.assert_allclose(grad3.double().numpy(), 3.0 * grad.double().numpy(), rtol=2e-7, atol=0)
    # two runs: the same bits; and gs_count as a [P,1] column is the same call
    got_b, grad_b = fused(x32, counts.unsqueeze(1), raw)
    assert torch.equal(got_b, got) and prune_ref.same_bits(grad_b, grad)


@pytest.mark.parametrize("raw", (False, True), ids=("activated", "raw"))
@pytest.mark.parametrize("P", SIZES)
def test_scale_decay_is_exactly_zero_when_no_count_exceeds_the_threshold(P, raw):
    _need_gpu()
    logs, counts = scale_inputs(P, low_counts=True)
    assert int(counts.max()) <= 4
    x32 = logs if raw else torch.exp(logs)
    got, grad = fused(x32, counts, raw, 3.0)
    want, want_grad = reference(x32, counts, raw, 3.0)
    assert want == 0 and not want_grad.any()
    assert got.item() == 0 and prune_ref.same_bits(grad, torch.zeros(P, 3))


def test_scale_decay_threshold_and_the_training_step_without_synchronisation():
    _need_gpu()
    P = 4097
    logs, counts = scale_inputs(P)
    # another threshold
    x = logs.double().requires_grad_(True)
    c = counts.long()
    want = (torch.exp(x).max(dim=1)[0] * (c - 9) * (c > 9)).mean()
    want.backward()
    got, grad = fused(logs, counts, True, threshold=9)
    np.testing.assert_allclose(got.item(), want.item(), rtol=RTOL, atol=0)
    np.testing.assert_allclose(grad.double().numpy(), x.grad.numpy(), rtol=RTOL, atol=0)
    assert (grad[10] == 0).all() and grad[11, 1] > 0  # counts 9 and 17
    # prune.py:253-261, :270: `loss += scale_loss * scale_weight` and loss.backward() enqueue, nothing waits for the device
    xs, cd = logs.to(DEV).requires_grad_(True), counts.to(DEV)
    other = torch.ones((), device=DEV)
    pruning.scale_decay_loss(xs, cd, raw=True).backward()  # (the library is loaded)
    xs.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = other * 2.0
        loss = loss + pruning.scale_decay_loss(xs, cd, raw=True) * 1e-3
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _, want_grad = reference(logs, counts, True, 1e-3)
    np.testing.assert_allclose(xs.grad.cpu().double().numpy(), want_grad, rtol=RTOL, atol=0)
    # no gradient asked for: the value alone
    want_value = fused(logs, counts, True)[0]
    with torch.no_grad():
        value = pruning.scale_decay_loss(logs.to(DEV), cd, raw=True)
    assert not value.requires_grad and torch.equal(value.cpu(), want_value)


# ---- opacity cap -----------------------------------------------------------------------------------------------------
def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def opacity_values(P, cap):
    """raw opacities fp32 [P,1]: -30, 0, logit(cap) itself, +30, +inf and NaN first (as many as fit), then 3 * randn"""
    g = torch.Generator().manual_seed(200 + P)
    v = 3.0 * torch.randn(P, 1, generator=g)
    special = torch.tensor([30.0, -30.0, 0.0, math.log(cap / (1 - cap)), float("inf"), float("nan")])
    v[:min(P, 6), 0] = special[:min(P, 6)]
    return v


def stepped_model(P, optimizer_cls, stepped=NAMES):
    model = prune_ref.Model(syn.scene_1k(P=P), optimizer_cls, device=DEV)
    g = torch.Generator().manual_seed(P)
    for n in stepped:
        p = getattr(model, ATTRS[n])
        p.grad = (1e-3 * torch.randn(p.shape, generator=g)).to(DEV)
    if stepped:
        model.optimizer.step()
        model.optimizer.step()
        model.optimizer.zero_grad(set_to_none=True)
    return model


def check_cap(model, call, cap, values):
    """Run `call` on `model` whose _opacity holds `values`, and check the kernel's three outputs and the host surgery."""
    opt = model.optimizer
    with torch.no_grad():
        model._opacity.copy_(values.to(DEV))
    old = model._opacity
    had_state = old in opt.state
    st_before = opt.state.get(old, None)
    step_before = None if not had_state else float(st_before["step"])
    before = {k: v.clone() for k, v in prune_ref.state_tensors(model).items()}
    others = {n: getattr(model, ATTRS[n]) for n in NAMES if n != "opacity"}
    new = call(model)
    # the surgery of replace_tensor_to_optimizer
    group = [g for g in opt.param_groups if g["name"] == "opacity"][0]
    assert new is model._opacity and new is group["params"][0] and new is not old and len(group["params"]) == 1
    assert isinstance(new, torch.nn.Parameter) and new.requires_grad and new.is_leaf and new.shape == old.shape and new.grad is None
    assert new.data_ptr() != old.data_ptr() and old not in opt.state
    assert (new in opt.state) == had_state and len(opt.state) == len([k for k in before if k.endswith(".exp_avg")])
    if had_state:
        st = opt.state[new]
        assert st is st_before and set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == step_before == 2
        for k in ("exp_avg", "exp_avg_sq"):
            assert st[k].shape == new.shape and st[k].dtype == torch.float32 and prune_ref.same_bits(st[k], torch.zeros_like(st[k])), k
    after = prune_ref.state_tensors(model)
    assert after.keys() == before.keys()
    for k in before:
        if not k.startswith("opacity"):
            assert prune_ref.same_bits(before[k], after[k]), k
    assert all(getattr(model, ATTRS[n]) is p for n, p in others.items())
    # the values
    x = values.reshape(-1).numpy()
    out = new.detach().cpu().reshape(-1).numpy()
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    target = np.float32(math.log(cap / (1.0 - cap)))
    n_capped = 0
    for i in range(len(x)):
        same = x[i:i + 1].view(np.int32)[0] == out[i:i + 1].view(np.int32)[0]
        if np.isnan(x[i]):
            assert same, (i, out[i])  # NaN stays NaN, payload and all
        elif abs(sig[i] - cap) < 1e-6:  # on the threshold, logit(cap) itself: capped or kept, the value is logit(cap) either way
            assert same or _ulps(out[i], target) <= 1, (i, x[i], out[i])
        elif sig[i] > cap:
            n_capped += 1
            assert _ulps(out[i], target) <= 1, (i, x[i], out[i], target)
        else:
            assert same, (i, x[i], out[i])
    return n_capped


@pytest.mark.parametrize("optimizer_cls", (optim.Adam, torch.optim.Adam), ids=("fused", "torch"))
@pytest.mark.parametrize("cap", (0.01, 0.1, 0.99))
@pytest.mark.parametrize("P", SIZES)
def test_reset_opacity_max_caps_and_replaces_the_parameter(P, cap, optimizer_cls):
    _need_gpu()
    model = stepped_model(P, optimizer_cls)
    st = model.optimizer.state[model._opacity]
    assert st["exp_avg"].abs().max() > 0 and st["exp_avg_sq"].abs().max() > 0  # (there is something to zero)
    n = check_cap(model, lambda m: pruning.reset_opacity_max(m, max=cap), cap, opacity_values(P, cap))
    assert n >= 1 and (P < 6 or n >= 2)  # +30, and +inf when it fits
    # one further step works on the new parameter
    model._opacity.grad = torch.ones_like(model._opacity)
    model.optimizer.step()
    assert float(model.optimizer.state[model._opacity]["step"]) == 3


def test_the_siblings_and_a_group_without_state():
    _need_gpu()
    P = 257
    model = stepped_model(P, optim.Adam)
    check_cap(model, pruning.reset_opacity, 0.01, opacity_values(P, 0.01))
    check_cap(model, lambda m: pruning.reset_opacity_upper_bound(m, 0.3), 0.3, opacity_values(P, 0.3))
    check_cap(model, pruning.reset_opacity_max, 0.99, opacity_values(P, 0.99))  # the default
    for cls in (optim.Adam, torch.optim.Adam):
        # no state at all, and state for other groups only: the parameter alone is replaced
        for stepped in ((), ("xyz", "scaling")):
            model = stepped_model(P, cls, stepped)
            assert check_cap(model, lambda m: pruning.reset_opacity_max(m, max=0.1), 0.1, opacity_values(P, 0.1)) > 10
            assert len(model.optimizer.state) == len(stepped) and model._opacity not in model.optimizer.state
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        pruning.reset_opacity_max(model, max=1.0)


def test_a_render_after_the_cap_sees_the_new_opacities():
    _need_gpu()
    model = stepped_model(3000, optim.Adam)
    cam, bg = syn.camera_1k(96, 64).to(DEV), torch.zeros(3, device=DEV)
    with torch.no_grad():
        before = render(cam, model, Pipe(), bg, cuda_type="pcheck_obb")["render"].clone()  # (the renderer has seen the old tensor)
        assert int((torch.sigmoid(model._opacity) > 0.1).sum()) > 100
        pruning.reset_opacity_max(model, max=0.1)
        assert float(torch.sigmoid(model._opacity).max()) <= 0.1 + 1e-6
        after = render(cam, model, Pipe(), bg, cuda_type="pcheck_obb")["render"].clone()
        fresh = prune_ref.clone_model(model)
        want = render(cam, fresh, Pipe(), bg, cuda_type="pcheck_obb")["render"]
    assert torch.equal(after, want) and not torch.equal(after, before) and before.max() > 0.1
