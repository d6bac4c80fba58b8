"""The quality gate on the MI355X (csrc/quality.hip): image_utils.mse / psnr, quality.QualityMeter and quality.evaluate_views
against tests/golden/ref_quality.npz -- the reference's own loss_utils.ssim, l1_loss and image_utils.psnr, mse on four pictures,
none a multiple of the kernels' 16x32 tile but the last, with the same expressions evaluated in float64 beside them.

Tolerances: SSIM and L1 within 2e-6 absolute of the reference's fp32 value on THESE pictures: noise, and one smooth pair with
noise of sigma 0.03 (what tests/test_loss.py holds the same arithmetic to, on the same kind of picture). It is no general bound: on flat, dark and stepped pictures the
reference's fp32 SSIM is itself up to 2.2e-4 from float64, and tests/test_loss_flat_gpu.py judges the meter there against float64 by
the spread of a float32 family of the reference's formula (measured: 9.9e-7 blob, 9.3e-6 flat, 3.7e-7 steps, 3.3e-8 dark, each with
the bits of loss_utils.ssim; profiles/loss_parity.json); MSE within 1e-6 relative of the float64 evaluation (non-negative terms, accumulated in double); PSNR within 1e-5 dB of
it (10 / ln 10 times the MSE bound, and an fp32 rounding of a value below 64 dB is under 4e-6), and within 1e-5 dB plus the
reference's own fp32-to-float64 distance (stored by the generator) of the reference's fp32 value."""
import os

import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import image_utils, loss_utils, optim, quality
from fov3dgs_amd import synthetic as syn
from fov3dgs_amd.gaussian_renderer import render
from fov3dgs_amd.odak_perception import MetamericLossUniform
from tests import hvs_cases, prune_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "ref_quality.npz"))
FINITE = (0, 1, 2)
SSIM_TOL = L1_TOL = 2e-6
MSE_RTOL = 1e-6
PSNR_TOL = 1e-5


class Pipe:
    debug = False


def _need_gpu():
    assert torch.cuda.is_available(), "this test needs the MI355X"


def _pair(i):
    return torch.from_numpy(Z[f"a{i}"]).to(DEV), torch.from_numpy(Z[f"b{i}"]).to(DEV)


def _check_view(i, ssim, psnr, l1, what=""):
    assert abs(ssim - float(Z[f"ssim_{i}"])) <= SSIM_TOL, (what, i, ssim, Z[f"ssim_{i}"])
    assert abs(l1 - float(Z[f"l1_{i}"])) <= L1_TOL, (what, i, l1, Z[f"l1_{i}"])
    assert abs(psnr - float(Z[f"psnr64_{i}"])) <= PSNR_TOL, (what, i, psnr, Z[f"psnr64_{i}"])
    assert abs(psnr - float(Z[f"psnr_{i}"])) <= PSNR_TOL + float(Z[f"psnr_gap_{i}"]), (what, i, psnr, Z[f"psnr_{i}"])


@pytest.mark.parametrize("i", FINITE)
def test_metrics_match_the_reference(i):
    _need_gpu()
    a, b = _pair(i)
    C = a.shape[0]
    m, p = image_utils.mse(a[None], b[None]), image_utils.psnr(a[None], b[None])
    assert m.shape == p.shape == (1, 1) and m.dtype == p.dtype == torch.float32 and m.device == a.device
    print(f"case {i}: mse {m.item()!r} (float64 {float(Z[f'mse64_{i}'])!r}), psnr {p.item()!r} (float64 {float(Z[f'psnr64_{i}'])!r}, "
          f"reference {float(Z[f'psnr_{i}'])!r})")
    assert abs(m.item() / float(Z[f"mse64_{i}"]) - 1) <= MSE_RTOL
    assert abs(p.item() - float(Z[f"psnr64_{i}"])) <= PSNR_TOL
    assert abs(p.item() - float(Z[f"psnr_{i}"])) <= PSNR_TOL + float(Z[f"psnr_gap_{i}"])
    # a [C,H,W] input: one value per channel, as the reference's view(shape[0], -1)
    mc, pc = image_utils.mse(a, b), image_utils.psnr(a, b)
    assert mc.shape == pc.shape == (C, 1)
    mc, pc = mc.cpu().double().numpy()[:, 0], pc.cpu().double().numpy()[:, 0]
    print(f"case {i}: per channel mse {mc}, psnr {pc} (float64 {Z[f'psnr_ch64_{i}']})")
    assert (np.abs(mc / Z[f"mse_ch64_{i}"] - 1) <= MSE_RTOL).all()
    assert (np.abs(pc - Z[f"psnr_ch64_{i}"]) <= PSNR_TOL).all()
    assert (np.abs(pc - Z[f"psnr_ch_{i}"].astype(np.float64)) <= PSNR_TOL + Z[f"psnr_ch_gap_{i}"]).all()
    # the meter's view: SSIM and L1 too, and the same PSNR bits as image_utils.psnr (one kernel, one order)
    meter = quality.QualityMeter(DEV, 1)
    meter.add(a, b)
    r = meter.result()
    print(f"case {i}: ssim {r['ssim']!r} (reference {float(Z[f'ssim_{i}'])!r}), l1 {r['l1']!r} (reference {float(Z[f'l1_{i}'])!r})")
    _check_view(i, r["ssim"], r["psnr"], r["l1"])
    assert r["n"] == 1 and torch.equal(r["per_view"]["psnr"], p.cpu()[:, 0]) and torch.equal(r["per_view"]["mse"], m.cpu()[:, 0])
    # non-contiguous and fp64 inputs are converted, [1,C,H,W] is the same picture
    meter.reset()
    meter.add(a.double()[None], b.permute(1, 2, 0).contiguous().permute(2, 0, 1)[None])
    r2 = meter.result()
    assert all(torch.equal(r["per_view"][k], r2["per_view"][k]) for k in r["per_view"]) and r2["n"] == 1
    assert torch.equal(image_utils.psnr(a.double(), b.permute(1, 2, 0).contiguous().permute(2, 0, 1)), image_utils.psnr(a, b))


def test_equal_pictures_give_infinite_psnr_and_ssim_one():
    _need_gpu()
    a, b = _pair(3)
    assert torch.equal(a, b)
    p, m = image_utils.psnr(a[None], b[None]), image_utils.mse(a[None], b[None])
    assert p.shape == (1, 1) and torch.isposinf(p).all() and (m == 0).all()
    assert torch.isposinf(image_utils.psnr(a, b)).all() and image_utils.psnr(a, b).shape == (3, 1)
    meter = quality.QualityMeter(DEV, 2)
    meter.add(a, b)
    r = meter.result()
    assert r["psnr"] == float("inf") and abs(r["ssim"] - 1) <= 1e-6 and r["l1"] == 0 and r["n"] == 1
    assert meter.passes(1e9, 0.999)


def _fill(meter):
    for i in FINITE:
        meter.add(*_pair(i))
    return meter


def test_meter_means_slots_and_determinism():
    _need_gpu()
    meter = _fill(quality.QualityMeter(DEV, 3))
    assert len(meter) == 3
    r = meter.result()
    assert r["n"] == 3 and set(r) == {"ssim", "psnr", "l1", "n", "per_view"} and set(r["per_view"]) == {"ssim", "psnr", "l1", "mse"}
    for v, i in enumerate(FINITE):
        pv = {k: float(r["per_view"][k][v]) for k in r["per_view"]}
        _check_view(i, pv["ssim"], pv["psnr"], pv["l1"], "slot")
        assert abs(pv["mse"] / float(Z[f"mse64_{i}"]) - 1) <= MSE_RTOL
        # ... and each slot holds the bits of that view measured alone
        alone = quality.QualityMeter(DEV, 1)
        alone.add(*_pair(i))
        ra = alone.result()
        assert all(torch.equal(ra["per_view"][k][0], r["per_view"][k][v]) for k in ra["per_view"]), i
    # the means are means over the views of the per-view values (prune.py:144-154, :163-174), to the per-view tolerances
    for k, tol in (("ssim", SSIM_TOL), ("l1", L1_TOL)):
        assert abs(r[k] - np.mean([float(Z[f"{k}_{i}"]) for i in FINITE])) <= tol, k
        assert abs(r[k] - float(r["per_view"][k].double().mean())) < 1e-13
    assert abs(r["psnr"] - np.mean([float(Z[f"psnr64_{i}"]) for i in FINITE])) <= PSNR_TOL
    assert abs(r["psnr"] - float(r["per_view"]["psnr"].double().mean())) < 1e-13
    # a second identical run, on a new meter and on this one after reset()
    again = _fill(quality.QualityMeter(DEV, 3)).result()
    meter.reset()
    assert len(meter) == 0 and meter.result()["n"] == 0
    third = _fill(meter).result()
    for other in (again, third):
        assert all(other[k] == r[k] for k in ("ssim", "psnr", "l1", "n"))
        assert all(torch.equal(other["per_view"][k], r["per_view"][k]) for k in r["per_view"])


def test_meter_adds_enqueue_without_synchronisation():
    _need_gpu()
    pairs = [_pair(i) for i in FINITE]
    meter = quality.QualityMeter(DEV, 8)
    want = _fill(quality.QualityMeter(DEV, 3)).result()  # (the library is loaded)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for a, b in pairs:
            meter.add(a, b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = meter.result()
    assert got["n"] == 3 and all(got[k] == want[k] for k in ("ssim", "psnr", "l1"))
    assert all(torch.equal(got["per_view"][k], want["per_view"][k]) for k in want["per_view"])


def test_meter_capacity_and_gate():
    _need_gpu()
    a, b = _pair(1)
    meter = quality.QualityMeter(DEV, 2)
    meter.add(a, b)
    meter.add(a, b)
    with pytest.raises(RuntimeError, match="capacity"):
        meter.add(a, b)
    r = meter.result()
    assert r["n"] == 2 and r["per_view"]["ssim"].shape == (2,)  # the refused view left nothing behind
    with pytest.raises(ValueError):
        meter.add(a, b[:, :-1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meter.add(a.cpu(), b.cpu())
    psnr, ssim = r["psnr"], r["ssim"]
    assert 30 < psnr < 31 and 0.86 < ssim < 0.87
    assert meter.passes(psnr, ssim) is True                # both thresholds are met with equality (prune.py:288-289: >=)
    assert meter.passes(psnr - 1e-3, ssim - 1e-4) is True
    assert meter.passes(psnr + 1e-3, ssim - 1e-4) is False  # PSNR alone fails
    assert meter.passes(psnr - 1e-3, ssim + 1e-4) is False  # SSIM alone fails
    assert meter.passes(psnr + 1e-3, ssim + 1e-4) is False


class _Cam:
    def __init__(self, gt):
        self.original_image = gt
        self.image_height, self.image_width = gt.shape[1], gt.shape[2]


def _recording(pictures, seen):
    it = iter(pictures)

    def stub(cam, pc, pipe, bg, **kw):
        assert not torch.is_grad_enabled()
        seen.append((cam, kw))
        return {"render": next(it)}
    return stub


def test_evaluate_views_renders_each_camera_once_with_pcheck_obb():
    _need_gpu()
    model = prune_ref.Model(syn.scene_1k(P=100), optim.Adam, device=DEV)
    g = torch.Generator().manual_seed(4)
    gts = [torch.rand(3, 40, 50, generator=g).to(DEV) for _ in range(3)]
    pics = [(gt + 0.05 * torch.randn(3, 40, 50, generator=g).to(DEV)).clamp(0, 1) for gt in gts]
    pics[1] = gts[1].clone()  # one perfect view: its PSNR, and so the mean, is inf, as in the reference
    cams, seen = [_Cam(gt) for gt in gts], []
    out = quality.evaluate_views(model, cams, Pipe(), torch.zeros(3, device=DEV), render=_recording(pics, seen))
    assert [c for c, _ in seen] == cams and all(kw == {"cuda_type": "pcheck_obb"} for _, kw in seen)
    assert out["n"] == 3 and "hvs" not in out and out["psnr"] == float("inf")
    for v in range(3):
        assert float(out["per_view"]["psnr"][v]) == image_utils.psnr(pics[v][None], gts[v][None]).item()
        assert abs(float(out["per_view"]["ssim"][v]) - loss_utils.ssim(pics[v], gts[v]).item()) <= 1e-6
        assert abs(float(out["per_view"]["l1"][v]) - loss_utils.l1_loss(pics[v], gts[v]).item()) <= 1e-6
    assert abs(out["ssim"] - float(out["per_view"]["ssim"].double().mean())) < 1e-13


def test_evaluate_views_with_the_real_renderer():
    _need_gpu()
    torch.manual_seed(0)
    model = prune_ref.Model(syn.scene_1k(P=3000), optim.Adam, device=DEV)
    cams = [syn.camera_1k(96, 64).to(DEV)] + [syn.camera_ring(i, width=96, height=64).to(DEV) for i in (1, 2)]
    bg = torch.zeros(3, device=DEV)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        renders = [render(c, model, Pipe(), bg, cuda_type="pcheck_obb")["render"].clone() for c in cams]
    for c, r in zip(cams, renders):
        c.original_image = (r + 0.03 * torch.randn(r.shape, generator=g).to(DEV)).clamp(0, 1)
    print("real renders: max", [float(r.max()) for r in renders])
    assert all(r.shape == (3, 64, 96) for r in renders) and max(float(r.max()) for r in renders) > 0.1
    out = quality.evaluate_views(model, cams, Pipe(), bg)
    assert out["n"] == 3
    for v, (c, r) in enumerate(zip(cams, renders)):
        assert float(out["per_view"]["psnr"][v]) == image_utils.psnr(r[None], c.original_image[None]).item()
        assert abs(float(out["per_view"]["ssim"][v]) - loss_utils.ssim(r, c.original_image).item()) <= 1e-6
    print("real renders:", {k: out[k] for k in ("ssim", "psnr", "l1")})
    assert 25 < out["psnr"] < 45 and 0 < out["ssim"] < 1  # noise of sigma 0.03, partly clamped away on the black background
    assert abs(out["psnr"] - float(out["per_view"]["psnr"].double().mean())) < 1e-12
    assert model._xyz.grad is None


def test_evaluate_views_accumulates_the_hvs_loss_with_the_resize_inside():
    _need_gpu()
    model = prune_ref.Model(syn.scene_1k(P=100), optim.Adam, device=DEV)
    H, W = 62, 90  # no multiple of 2 ** 2: the loss runs at 64 x 92
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand(3, H, W, generator=g).to(DEV) for _ in range(2)]
    pics = [(gt + 0.1 * torch.randn(3, H, W, generator=g).to(DEV)).clamp(0, 1) for gt in gts]
    hvs = MetamericLossUniform(device=DEV, pooling_size=4, n_pyramid_levels=2, n_orientations=2, loss_type="L1", bilinear_downsampling=True,
                               filters=hvs_cases.filters(2))
    seen = []
    out = quality.evaluate_views(model, [_Cam(gt) for gt in gts], Pipe(), torch.zeros(3, device=DEV), render=_recording(pics, seen), hvs=hvs)
    assert len(seen) == 2 and out["n"] == 2
    want = [hvs(p[None], gt[None], resize="pyramid").item() for p, gt in zip(pics, gts)]
    assert want[0] > 0 and want[0] != want[1]
    assert [float(x) for x in out["per_view"]["hvs"]] == want
    assert abs(out["hvs"] - (want[0] + want[1]) / 2) < 1e-9
    assert float(out["per_view"]["psnr"][1]) == image_utils.psnr(pics[1][None], gts[1][None]).item()
    with pytest.raises(ValueError):  # without the resize the size is refused, as by the loss itself
        quality.evaluate_views(model, [_Cam(gt) for gt in gts], Pipe(), torch.zeros(3, device=DEV), render=_recording(pics, []), hvs=hvs, resize=None)
