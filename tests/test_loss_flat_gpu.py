"""The fused L1 + SSIM loss (csrc/loss.hip) and the quality meter's copy of its arithmetic (csrc/quality.hip) on the MI355X, on the
flat, dark and stepped pictures of tests/loss_cases.py: black background, constant areas, x == y regions, edges on and off the tile
seams -- where SSIM's stabilisers and the cancellation E[x^2] - mu^2 decide the result, and where white noise never looks.

Every value and every gradient element is compared with the float64 oracle inside the allowance of its case: four times the largest
distance of a float32 family of the reference's own formula from float64 (loss_cases.case; the L1 value's allowance is derived
there). tests/test_loss_flat_cpu.py shows that those allowances still catch a stabiliser off by 1 %. Every measured figure is printed
and recorded beside its yardstick and allowance (parity report, kind "loss"; one MI355X session is kept in profiles/loss_parity.json).
Beyond the allowances: the L1 term bit for bit, x == y, run-to-run bits, float16 and non-contiguous inputs."""
import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import loss_utils as lu
from fov3dgs_amd import quality
from tests import loss_cases as lc
from tests import parity_report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MSE_RTOL, PSNR_TOL = 1e-6, 1e-5  # tests/test_quality_gpu.py's float64 rule


def _need_gpu():
    assert torch.cuda.is_available(), "this test needs the MI355X"


def _pair(c, grad_x=False, grad_y=False):
    return c["x"].to(DEV).requires_grad_(grad_x), c["y"].to(DEV).requires_grad_(grad_y)


def _judge(c, label, measured):
    """print and record every figure beside its yardstick and allowance, then assert all of them"""
    bad = []
    for k, v in measured.items():
        yard, allow = c["yardstick"][k], c["allowance"][k]
        print(f"{c['name']} / {label} / {k}: measured {v:.3e}, yardstick {yard:.3e}, allowance {allow:.3e}")
        parity_report.record("loss", f"{c['name']}/{label}/{k}", measured=v, yardstick=yard, allowance=allow)
        if not v <= allow:
            bad.append((c["name"], label, k, v, allow))
    assert not bad, bad


@pytest.mark.parametrize("name", [n for n in lc.NAMES if n != "equal"])
def test_values_and_gradients_stay_inside_the_family_allowance(name):
    _need_gpu()
    c = lc.case(name)
    x, y = _pair(c, grad_x=True)
    loss = lu.l1_ssim_loss(x, y, lc.LAM)
    loss.backward()
    x2 = c["x"].to(DEV).requires_grad_(True)
    ss = lu.ssim(x2, y)
    ss.backward()
    assert x.grad.shape == x2.grad.shape == c["x"].shape and loss.dtype == ss.dtype == torch.float32
    got = dict(l1=lu.l1_loss(x.detach(), y).item(), ssim=ss.item(), loss=loss.item(), grad_loss=x.grad, grad_ssim=x2.grad)
    _judge(c, "loss_utils", lc.statistics(c, got))
    # the kernel's own L1 sum (loss_utils.l1_loss is a torch expression): with lam = 0 the loss IS its float32 l1
    _judge(c, "kernel", lc.statistics(c, dict(l1=lu.l1_ssim_loss(x.detach(), y, 0.0).item())))


@pytest.mark.parametrize("name", lc.GT_GRAD)
def test_the_gradient_with_respect_to_gt(name):
    _need_gpu()
    c = lc.case(name)
    x, y = _pair(c, grad_y=True)
    lu.l1_ssim_loss(x, y, lc.LAM).backward()
    assert x.grad is None and y.grad.shape == c["y"].shape
    _judge(c, "gt alone", lc.statistics(c, dict(grad_gt=y.grad)))
    x, y = _pair(c, grad_x=True, grad_y=True)
    lu.l1_ssim_loss(x, y, lc.LAM).backward()
    _judge(c, "both", lc.statistics(c, dict(grad_loss=x.grad, grad_gt=y.grad)))


@pytest.mark.parametrize("name", ["blob", "flat"])
def test_the_l1_term_bit_for_bit(name):
    """lam = 0: the gradient is exactly 0.0 wherever x == y (the reference's torch.abs convention, which tests/test_loss.py leaves
    unpinned), exactly +-float32(1 / n) elsewhere, and with an upstream factor of -2.5 that times -2.5 in one float32 rounding."""
    _need_gpu()
    c = lc.case(name)
    xn, yn = c["x"].numpy(), c["y"].numpy()
    w = np.float32(1.0 / c["n"])
    want = np.where(xn > yn, w, np.where(xn < yn, -w, np.float32(0.0))).astype(np.float32)
    assert 0.3 < float((want == 0).mean()) < 0.9
    x, y = _pair(c, grad_x=True)
    lu.l1_ssim_loss(x, y, 0.0).backward()
    got = x.grad.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want), float(np.abs(got - want).max())
    x, y = _pair(c, grad_x=True)
    (lu.l1_ssim_loss(x, y, 0.0) * -2.5).backward()
    got = x.grad.cpu().numpy()
    assert np.array_equal(got, (want * np.float32(-2.5)).astype(np.float32)), float(np.abs(got - want * np.float32(-2.5)).max())


def test_equal_pictures():
    """x == y bit for bit: the five moments of x and y are bit-equal, so a1 == b1 and a2 == b2 exactly and every map value is a product
    times the reciprocal of the same product: |ssim - 1| <= 2 eps32. l1 is exactly 0. SSIM's true gradient is 0: n max |g| is judged
    against the family's own."""
    _need_gpu()
    c = lc.case("equal")
    x, y = _pair(c, grad_x=True)
    loss = lu.l1_ssim_loss(x, y, lc.LAM)
    loss.backward()
    x2 = c["x"].to(DEV).requires_grad_(True)
    ss = lu.ssim(x2, y)
    ss.backward()
    l1 = lu.l1_ssim_loss(x.detach(), y, 0.0).item()
    print(f"equal: ssim - 1 = {ss.item() - 1.0:.3e} (allowed {2 * lc.EPS32:.3e}), loss {loss.item():.3e}, l1 {l1!r}")
    parity_report.record("loss", "equal/loss_utils/ssim_minus_1", measured=abs(ss.item() - 1.0), allowance=2 * lc.EPS32)
    assert abs(ss.item() - 1.0) <= 2 * lc.EPS32
    assert l1 == 0.0 and lu.l1_loss(x.detach(), y).item() == 0.0
    assert abs(loss.item()) <= lc.LAM * 2 * lc.EPS32 * (1 + lc.EPS32)  # 0.8 * 0 + 0.2 * (1 - ssim)
    _judge(c, "loss_utils", lc.statistics(c, dict(grad_loss=x.grad, grad_ssim=x2.grad)))


@pytest.mark.parametrize("name", ["blob", "steps"])
def test_two_runs_give_the_same_bits(name):
    _need_gpu()
    c = lc.case(name)
    runs = []
    for _ in range(2):
        x, y = _pair(c, grad_x=True, grad_y=True)
        out = lu.l1_ssim_loss(x, y, lc.LAM)
        out.backward()
        runs.append((out.detach().clone(), lu.ssim(x.detach(), y), x.grad, y.grad))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("name", ["blob", "smooth"])
def test_a_float16_render(name):
    """The value is the loss of the ROUNDED picture (judged against the oracle on it, inside the family's allowance there); the
    gradient comes back as float16, within one float16 rounding of the float32 path's."""
    _need_gpu()
    c, h = lc.case(name), lc.half_case(name)
    y = c["y"].to(DEV)
    x16 = h["x16"].to(DEV).requires_grad_(True)
    out = lu.l1_ssim_loss(x16, y, lc.LAM)
    out.backward()
    d = abs(out.item() - h["loss64"])
    print(f"{name} / float16 / loss: measured {d:.3e}, yardstick {h['yardstick']:.3e}, allowance {h['allowance']:.3e}")
    parity_report.record("loss", f"{name}/float16/loss", measured=d, yardstick=h["yardstick"], allowance=h["allowance"])
    assert h["yardstick"] > 0 and d <= h["allowance"]
    x32 = h["x16"].float().to(DEV).requires_grad_(True)
    out32 = lu.l1_ssim_loss(x32, y, lc.LAM)
    out32.backward()
    assert x16.grad.dtype == torch.float16 and x16.grad.shape == x32.grad.shape and torch.equal(out, out32)
    g16, g32 = x16.grad.double().cpu(), x32.grad.double().cpu()
    # one rounding to float16: half an ulp, 2^-11 relative for normal numbers, 2^-25 absolute below 2^-14
    assert bool(((g16 - g32).abs() <= torch.maximum(g32.abs() * 2.0 ** -11, torch.tensor(2.0 ** -25, dtype=torch.float64))).all())
    assert float(g32.abs().max()) > 2.0 ** -14  # (not all of it in the subnormal range)


def test_non_contiguous_renders_give_the_bits_of_the_contiguous_copy():
    _need_gpu()
    c = lc.case("blob")
    x, y = _pair(c, grad_x=True)
    want = lu.l1_ssim_loss(x, y, lc.LAM)
    want.backward()
    wide = torch.full((lc.C, lc.H, 64), 0.25, device=DEV)
    wide[:, :, :lc.W] = c["x"].to(DEV)
    hwc = c["x"].to(DEV).permute(1, 2, 0).contiguous()
    for view in (wide[:, :, :lc.W], hwc.permute(2, 0, 1)):
        v = view.detach().requires_grad_(True)
        assert not v.is_contiguous() and v.shape == x.shape
        out = lu.l1_ssim_loss(v, y, lc.LAM)
        out.backward()
        assert torch.equal(out, want) and v.grad.shape == v.shape and torch.equal(v.grad, x.grad)
        assert torch.equal(lu.ssim(v.detach(), y), lu.ssim(x.detach(), y))


def test_the_quality_meter_on_the_same_pictures():
    """QualityMeter.add (csrc/quality.hip restates k_l1_ssim_fwd's arithmetic): per-view ssim and l1 inside the same value allowances,
    mse / psnr by the float64 rule of tests/test_quality_gpu.py, and per_view["ssim"] within 1e-6 of loss_utils.ssim here too."""
    _need_gpu()
    names = ("blob", "flat", "steps", "dark")
    meter = quality.QualityMeter(DEV, len(names))
    for name in names:
        meter.add(*_pair(lc.case(name)))
    r = meter.result()
    assert r["n"] == len(names)
    for v, name in enumerate(names):
        c = lc.case(name)
        pv = {k: float(r["per_view"][k][v]) for k in r["per_view"]}
        _judge(c, "QualityMeter", lc.statistics(c, dict(ssim=pv["ssim"], l1=pv["l1"])))
        mse_rel, psnr_d = abs(pv["mse"] / c["mse64"] - 1), abs(pv["psnr"] - c["psnr64"])
        twin = abs(pv["ssim"] - lu.ssim(*_pair(c)).item())
        print(f"{name} / QualityMeter: mse off by {mse_rel:.3e} relative (allowed {MSE_RTOL}), psnr {pv['psnr']!r} off by {psnr_d:.3e} dB (allowed {PSNR_TOL}), "
              f"ssim {twin:.3e} from loss_utils.ssim (allowed 1e-6)")
        parity_report.record("loss", f"{name}/QualityMeter/others", mse_rel=mse_rel, psnr_abs=psnr_d, ssim_vs_loss_utils=twin)
        assert mse_rel <= MSE_RTOL and psnr_d <= PSNR_TOL and twin <= 1e-6
