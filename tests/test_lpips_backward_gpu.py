"""LPIPS as a training loss on the MI355X (csrc/lpips.hip: fr_lpips_forward_keep, fr_lpips_backward) against torch.autograd in
float64 on the cases of tests/lpips_cases.py.

A gradient through ReLU and max pool is discontinuous in the decisions, so the float64 gradient is taken with x's decisions frozen
to the maps the GPU kept (tests/lpips_grad_ref.py; LPIPSLoss.activations()), and that the GPU's decisions are right is checked on
its own: all 13 kept maps elementwise against float64. Bounds are measured, not guessed (tests/lpips_grad_cases.py): 4 x the
float32 torch.autograd gradient's own largest distance from float64, 1.352e-4 of |g64| + rms(g64) per element and 3.2e-5 relative
L2, and 4 x the float32 restatement's largest distance over the 13 maps, 1.496e-5."""
import functools

import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import lpipsPyTorch, optim
from fov3dgs_amd import synthetic as syn
from fov3dgs_amd.gaussian_renderer import render
from fov3dgs_amd.loss_utils import l1_ssim_loss
from tests import adam_ref, lpips_cases, lpips_grad_cases, lpips_grad_ref, parity_report, prune_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = list(lpips_cases.CASES)


class Pipe:
    debug = False


def _need_gpu():
    assert torch.cuda.is_available(), "this test needs the MI355X"


@functools.lru_cache(maxsize=None)
def loss():
    return lpipsPyTorch.LPIPSLoss("vgg", weights=lpips_cases.weights())


@functools.lru_cache(maxsize=None)
def metric():
    return lpipsPyTorch.LPIPS("vgg", weights=lpips_cases.weights())


def _grad(x, y, crit=None, want_maps=False):
    """one differentiable call -> (value, x.grad, the kept maps if asked for)"""
    x = x.detach().clone().requires_grad_(True)
    v = (crit or loss())(x, y)
    assert v.shape == (1, 1, 1, 1) and v.dtype == torch.float32 and v.grad_fn is not None
    maps = (crit or loss()).activations() if want_maps else None
    v.backward()
    return v.detach(), x.grad, maps


@functools.lru_cache(maxsize=None)
def run(name):
    """the case's value, gradient and kept maps from the GPU, once per session (left unchanged by the tests)"""
    c = lpips_cases.case(name)
    x, y = c["x"].to(DEV), c["y"].to(DEV)
    v, g, maps = _grad(x, y, want_maps=True)
    return dict(x=x, y=y, value=v, grad=g, maps=maps)


@pytest.mark.parametrize("name", NAMES)
def test_the_kept_maps_match_float64_elementwise(name):
    _need_gpu()
    got, want = run(name)["maps"], lpips_grad_cases.case(name)["maps64"]
    assert len(got) == 13
    ratios = []
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == torch.float32 and a.device.type == "cuda"
        a = a.cpu()
        assert torch.isfinite(a).all() and float(a.min()) >= 0.0
        ratios.append(lpips_cases.feature_ratio(a, b))
    print(f"{name}: ratios of the 13 maps {ratios} (bound {lpips_grad_cases.ACT_RTOL}, float32's own {lpips_grad_cases.ACT_YARDSTICK})")
    parity_report.record("lpips_kept_maps", name, worst_ratio=max(ratios), bound=lpips_grad_cases.ACT_RTOL, yardstick=lpips_grad_cases.ACT_YARDSTICK)
    assert max(ratios) <= lpips_grad_cases.ACT_RTOL, ratios


@pytest.mark.parametrize("name", NAMES)
def test_the_gradient_matches_float64_frozen_to_the_kept_decisions(name):
    _need_gpu()
    r = run(name)
    g = r["grad"]
    assert g.shape == r["x"].shape and g.dtype == torch.float32 and g.device == r["x"].device and torch.isfinite(g).all()
    v64, g64 = lpips_grad_cases.frozen64(r["x"].cpu(), r["y"].cpu(), r["maps"], name)
    ratio, l2 = lpips_grad_cases.grad_ratio(g.cpu(), g64), lpips_grad_cases.grad_l2(g.cpu(), g64)
    free = lpips_grad_cases.grad_ratio(g64, lpips_grad_cases.case(name)["grad64"])  # 0 when the GPU decided as float64 did
    print(f"{name}: ratio {ratio!r} (bound {lpips_grad_cases.GRAD_RTOL}), relative L2 {l2!r} (bound {lpips_grad_cases.GRAD_L2_RTOL}), "
          f"frozen float64 against free float64 {free!r}, |g64| {float(g64.norm())!r}")
    parity_report.record("lpips_gradient", name, ratio=ratio, bound=lpips_grad_cases.GRAD_RTOL, rel_l2=l2, l2_bound=lpips_grad_cases.GRAD_L2_RTOL,
                         frozen_vs_free=free)
    assert float(g64.norm()) > 0 and abs(float(v64) - r["value"].item()) <= lpips_cases.VALUE_RTOL * float(v64)
    assert ratio <= lpips_grad_cases.GRAD_RTOL and l2 <= lpips_grad_cases.GRAD_L2_RTOL, (ratio, l2)


def test_the_value_is_the_metrics_and_nothing_is_kept_without_grad():
    _need_gpu()
    for name in ("35x50", "64x48n2"):
        r = run(name)
        assert torch.equal(r["value"], metric()(r["x"], r["y"]))
    fresh = lpipsPyTorch.LPIPSLoss("vgg", weights=lpips_cases.weights())
    r = run("17x16")
    v = fresh(r["x"], r["y"])
    assert v.grad_fn is None and not v.requires_grad and fresh._last is None and fresh._packed_backward == {}
    assert torch.equal(v, r["value"])
    with torch.no_grad():  # nothing to differentiate: the plain call
        v = fresh(r["x"].clone().requires_grad_(True), r["y"])
    assert v.grad_fn is None and fresh._last is None and torch.equal(v, r["value"])
    with pytest.raises(RuntimeError, match="differentiable forward first"):
        fresh.activations()
    with pytest.raises(RuntimeError, match=r"y requires grad.*detach\(\)"):
        fresh(r["x"], r["y"].clone().requires_grad_(True))


def test_equal_pictures_give_exactly_zero_everywhere():
    _need_gpu()
    for name in ("35x50", "64x48n2"):
        x = run(name)["x"]
        v, g, _ = _grad(x, x.clone())
        assert v.item() == 0.0 and g.shape == x.shape and torch.equal(g, torch.zeros_like(g))


def test_ties_in_the_pool_windows_go_to_the_first_maximum():
    _need_gpu()
    x = torch.tensor([0.2, 0.5, 0.7], device=DEV)[None, :, None, None].expand(1, 3, 20, 22).contiguous()
    y = torch.tensor([0.6, 0.3, 0.4], device=DEV)[None, :, None, None].expand(1, 3, 20, 22).contiguous()
    v, g, maps = _grad(x, y, want_maps=True)
    win = maps[1][0, :, 4:6, 4:6].reshape(64, 4)  # an interior window of relu1_2: the same chain at all four pixels
    tied = (win.min(1).values == win.max(1).values) & (win.max(1).values > 0)
    assert int(tied.sum()) >= 8, int(tied.sum())
    v64, g64 = lpips_grad_cases.frozen64(x.cpu(), y.cpu(), maps)
    ratio, l2 = lpips_grad_cases.grad_ratio(g.cpu(), g64), lpips_grad_cases.grad_l2(g.cpu(), g64)
    print(f"ties: value {v.item()!r} (float64 {float(v64)!r}), ratio {ratio!r}, relative L2 {l2!r}, tied channels {int(tied.sum())}")
    parity_report.record("lpips_gradient", "ties 20x22", ratio=ratio, bound=lpips_grad_cases.GRAD_RTOL, rel_l2=l2, l2_bound=lpips_grad_cases.GRAD_L2_RTOL)
    assert torch.isfinite(g).all() and float(g64.norm()) > 0
    assert ratio <= lpips_grad_cases.GRAD_RTOL and l2 <= lpips_grad_cases.GRAD_L2_RTOL, (ratio, l2)


def test_a_dead_tap_gives_finite_zeros_where_the_float32_restatement_gives_nan():
    _need_gpu()
    w = lpips_cases.weights()
    feats = dict(w["features"])
    feats["2.bias"] = torch.full((64,), -100.0)  # relu1_2 is zero everywhere; every later map is its biases' for both pictures
    dead = dict(features=feats, lin=w["lin"])
    c = lpips_cases.case("17x16")
    # the float32 restatement: normalize_activation's sqrt backward gives 0 / 0 = NaN at every pixel of the dead tap. Written with
    # a mask product (the frozen form) the NaN reaches x; F.relu's backward is a selection and happens to drop it again, as the
    # kernels do by rule
    _, free32, m32 = lpips_grad_ref.lpips_grad(c["x"], c["y"], dead, torch.float32)
    _, g32, _ = lpips_grad_ref.lpips_grad(c["x"], c["y"], dead, torch.float32, x_maps=m32)
    assert float(m32[1].max()) == 0.0 and torch.isnan(g32).any() and torch.equal(free32, torch.zeros_like(free32))
    v, g, maps = _grad(c["x"].to(DEV), c["y"].to(DEV), lpipsPyTorch.LPIPSLoss("vgg", weights=dead), want_maps=True)
    assert float(maps[1].max()) == 0.0 and float(maps[0].max()) > 0.0
    assert torch.isfinite(v).all() and torch.isfinite(g).all() and torch.equal(g, torch.zeros_like(g))


def test_the_upstream_gradient_is_applied_on_the_device():
    _need_gpu()
    r = run("33x130")
    wgt = torch.randn(r["x"].shape, generator=torch.Generator().manual_seed(11)).to(DEV)
    x = r["x"].clone().requires_grad_(True)
    (0.37 * loss()(x, r["y"]).sum() + (x * x * wgt).sum()).backward()  # the value is never read back in between
    want = 0.37 * r["grad"].double() + (2 * r["x"] * wgt).double()
    err = float((x.grad.double() - want).abs().max())
    print(f"upstream: largest distance {err!r}, largest |0.37 g| {0.37 * float(r['grad'].abs().max())!r}")
    assert err <= 4 * 2.0 ** -24 * float(want.abs().max())  # three float32 roundings (0.37, the product, the sum) and one to spare
    g2 = torch.autograd.grad((loss()(x, r["y"]) * 0.0).sum(), x)[0]
    assert torch.equal(g2, torch.zeros_like(g2))


def test_each_picture_of_a_batch_has_the_gradient_it_has_alone():
    _need_gpu()
    r = run("64x48n2")
    for i in range(2):
        v, g, _ = _grad(r["x"][i:i + 1], r["y"][i:i + 1])
        assert torch.equal(g[0], r["grad"][i]) and float(g.abs().max()) > 0
    assert not torch.equal(r["grad"][0], r["grad"][1])


def test_two_forwards_keep_their_own_state_and_a_second_backward_raises():
    _need_gpu()
    a, b = run("35x50"), run("33x130")
    xa, xb = a["x"].clone().requires_grad_(True), b["x"].clone().requires_grad_(True)
    va, vb = loss()(xa, a["y"]), loss()(xb, b["y"])
    vb.backward()
    va.backward()
    assert torch.equal(xa.grad, a["grad"]) and torch.equal(xb.grad, b["grad"])
    assert torch.equal(va.detach(), a["value"]) and torch.equal(vb.detach(), b["value"])
    with pytest.raises(RuntimeError, match="second time"):
        va.backward()
    xa.grad = None
    va = loss()(xa, a["y"])
    va.backward(retain_graph=True)
    va.backward()
    assert torch.equal(xa.grad, 2 * a["grad"])


def test_two_runs_and_a_side_stream_give_the_same_bits():
    _need_gpu()
    r = run("seams")
    v, g, maps = _grad(r["x"], r["y"], want_maps=True)
    assert torch.equal(v, r["value"]) and torch.equal(g, r["grad"]) and all(torch.equal(p, q) for p, q in zip(maps, r["maps"]))
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        junk = torch.randn(512, 512, device=DEV) @ torch.randn(512, 512, device=DEV)  # other work directly in front
        v2, g2, _ = _grad(r["x"], r["y"])
    s.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(s)
    assert torch.equal(v2, r["value"]) and torch.equal(g2, r["grad"]) and torch.isfinite(junk).all()


def test_the_functional_form_is_the_class():
    _need_gpu()
    r = run("17x16")
    w = lpips_cases.weights()
    lpipsPyTorch._loss_cache.clear()
    try:
        x = r["x"].clone().requires_grad_(True)
        v = lpipsPyTorch.lpips_loss(x, r["y"], weights=w)
        v.backward()
        assert torch.equal(v.detach(), r["value"]) and torch.equal(x.grad, r["grad"])
        assert len(lpipsPyTorch._loss_cache) == 1 and torch.equal(lpipsPyTorch.lpips_loss(r["x"], r["y"], net_type="vgg", weights=w), r["value"])
        assert len(lpipsPyTorch._loss_cache) == 1
    finally:
        lpipsPyTorch._loss_cache.clear()


def test_one_training_step_with_the_perceptual_term():
    """render (pcheck_obb_sum) -> l1_ssim_loss + 0.1 lpips_loss -> backward on 20 000 Gaussians at 64 x 48"""
    _need_gpu()
    torch.manual_seed(0)
    model = prune_ref.Model(syn.scene_1k(P=20_000), optim.Adam, device=DEV)
    cam, bg = syn.camera_1k(64, 48).to(DEV), torch.zeros(3, device=DEV)
    target = torch.rand(3, 48, 64, generator=torch.Generator().manual_seed(3)).to(DEV)

    def grads(lam):
        model.optimizer.zero_grad(set_to_none=True)
        image = render(cam, model, Pipe(), bg, cuda_type="pcheck_obb_sum")["render"]
        assert image.shape == target.shape
        total = l1_ssim_loss(image, target, 0.2)
        if lam:
            total = total + lam * loss()(image[None], target[None]).sum()
        total.backward()
        out = {n: getattr(model, adam_ref.ATTRS[n]).grad for n in ("xyz", "f_dc", "opacity")}
        return {n: (g.to_dense() if g.is_sparse else g).clone() for n, g in out.items()}
    plain, again, with_term = grads(0.0), grads(0.0), grads(0.1)
    for n in plain:
        assert torch.isfinite(with_term[n]).all() and float(with_term[n].abs().max()) > 0
        noise = float((again[n] - plain[n]).norm() / plain[n].norm())  # the rasterizer's backward sums with float atomics
        moved = float((with_term[n] - plain[n]).norm() / plain[n].norm())
        print(f"{n}: the perceptual term moves the gradient by {moved!r} of its norm (two plain runs differ by {noise!r})")
        assert moved > 1e-3 and moved > 10 * noise
