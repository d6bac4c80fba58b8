"""LPIPS on the MI355X (csrc/lpips.hip) against tests/lpips_ref.py in float64 on the cases of tests/lpips_cases.py.

Tolerances are measured, not guessed: the yardsticks are the float32 restatement's own largest distances from float64 over the
six cases (lpips_cases.FEAT_YARDSTICK: 3.18e-6 of |f64| + rms(map) per feature-map element; VALUE_YARDSTICK: 3.53e-6 relative per
tap value and total), and the HIP path gets 4 times that (FEAT_RTOL 1.272e-5, VALUE_RTOL 1.412e-5): its sums run in another order
than torch's CPU kernels. Tests 1 and 2 judge the kernels; the elementwise feature test is the one that sees a wrong halo, padding,
pool floor or tile seam, which the spatial mean of the final value would hide."""
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import lpipsPyTorch, optim, quality
from fov3dgs_amd import synthetic as syn
from fov3dgs_amd.gaussian_renderer import render
from tests import lpips_cases, parity_report, prune_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = list(lpips_cases.CASES)


class Pipe:
    debug = False


def _need_gpu():
    assert torch.cuda.is_available(), "this test needs the MI355X"


_crit = None


def crit():
    global _crit
    if _crit is None:
        _crit = lpipsPyTorch.LPIPS("vgg", weights=lpips_cases.weights())
    return _crit


def _pair(name):
    c = lpips_cases.case(name)
    return c, c["x"].to(DEV), c["y"].to(DEV)


@pytest.mark.parametrize("name", NAMES)
def test_feature_maps_match_float64_elementwise(name):
    _need_gpu()
    c, x, _ = _pair(name)
    feats = crit().features(x)
    assert len(feats) == 5
    ratios = []
    for k, (got, want) in enumerate(zip(feats, c["feats64"])):
        assert got.shape == want.shape and got.dtype == torch.float32 and got.device.type == "cuda"
        got = got.cpu()
        assert torch.isfinite(got).all() and float(got.min()) >= 0.0
        ratios.append(lpips_cases.feature_ratio(got, want))
    print(f"{name}: feature ratios {ratios} (bound {lpips_cases.FEAT_RTOL}, the float32 restatement's own {lpips_cases.FEAT_YARDSTICK})")
    parity_report.record("lpips_features", name, worst_ratio=max(ratios), bound=lpips_cases.FEAT_RTOL, yardstick=lpips_cases.FEAT_YARDSTICK)
    assert max(ratios) <= lpips_cases.FEAT_RTOL, ratios


@pytest.mark.parametrize("name", NAMES)
def test_tap_values_and_total_match_float64(name):
    _need_gpu()
    c, x, y = _pair(name)
    taps = crit().taps(x, y)
    value = crit()(x, y)
    assert value.shape == (1, 1, 1, 1) and value.dtype == torch.float32 and taps.shape == (5,)
    r = lpips_cases.value_ratios(taps.cpu(), value.item(), c)
    print(f"{name}: value {value.item()!r} (float64 {c['value64']!r}), relative distances {r} (bound {lpips_cases.VALUE_RTOL})")
    parity_report.record("lpips_values", name, worst_ratio=max(r), bound=lpips_cases.VALUE_RTOL, yardstick=lpips_cases.VALUE_YARDSTICK,
                         value=value.item(), value64=c["value64"])
    assert max(r) <= lpips_cases.VALUE_RTOL, r
    assert abs(float(taps.double().sum()) - value.item()) <= 1e-6 * value.item()


def test_equal_pictures_give_exactly_zero():
    _need_gpu()
    for name in ("35x50", "64x48n2"):
        _, x, _ = _pair(name)
        v = crit()(x, x.clone())
        assert v.shape == (1, 1, 1, 1) and v.item() == 0.0
        assert torch.equal(crit().taps(x, x), torch.zeros(5, device=DEV))


def test_two_runs_and_a_side_stream_give_the_same_bits():
    _need_gpu()
    _, x, y = _pair("33x130")
    a, ta, fa = crit()(x, y), crit().taps(x, y), crit().features(x)
    b, tb, fb = crit()(x, y), crit().taps(x, y), crit().features(x)
    assert torch.equal(a, b) and torch.equal(ta, tb) and all(torch.equal(p, q) for p, q in zip(fa, fb)) and a.item() > 0
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        junk = torch.randn(512, 512, device=DEV) @ torch.randn(512, 512, device=DEV)  # other work directly in front
        c = crit()(x, y)
        tc = crit().taps(x, y)
    s.synchronize()
    assert torch.equal(a, c) and torch.equal(ta, tc) and torch.isfinite(junk).all()


def test_a_batch_is_the_sum_of_its_pictures():
    _need_gpu()
    c, x, y = _pair("64x48n2")
    both = crit()(x, y)
    assert both.shape == (1, 1, 1, 1)
    singles = [crit()(x[i:i + 1], y[i:i + 1]).item() for i in range(2)]
    print(f"batch {both.item()!r}, singles {singles}, float64 {c['value64']!r}")
    assert min(singles) > 0 and singles[0] != singles[1]
    assert abs(both.item() - (singles[0] + singles[1])) <= lpips_cases.VALUE_RTOL * both.item()
    # a non-contiguous input is made contiguous: the same bits
    xt = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not xt.is_contiguous() and torch.equal(crit()(xt, y), both)


def test_the_functional_form_equals_the_class_and_packs_once():
    _need_gpu()
    w = lpips_cases.weights()
    _, x, y = _pair("17x16")
    want = crit()(x, y)
    lpipsPyTorch._cache.clear()
    lpipsPyTorch.set_default_weights(w)
    try:
        before = lpipsPyTorch.PACK_COUNT
        got = lpipsPyTorch.lpips(x, y, net_type="vgg")
        assert lpipsPyTorch.PACK_COUNT == before + 1
        again = lpipsPyTorch.lpips(x, y, net_type="vgg")
        explicit = lpipsPyTorch.lpips(x, y, net_type="vgg", weights=w)
        assert lpipsPyTorch.PACK_COUNT == before + 1  # the same weights object: no repack
        assert got.shape == (1, 1, 1, 1) and torch.equal(got, want) and torch.equal(again, want) and torch.equal(explicit, want)
    finally:
        lpipsPyTorch.set_default_weights(None)
        lpipsPyTorch._cache.clear()


def test_evaluate_views_adds_lpips_per_view_and_its_mean():
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
    plain = quality.evaluate_views(model, cams, Pipe(), bg)
    out = quality.evaluate_views(model, cams, Pipe(), bg, lpips=crit())
    assert "lpips" not in plain and "lpips" not in plain["per_view"]
    assert set(out) == set(plain) | {"lpips"} and set(out["per_view"]) == set(plain["per_view"]) | {"lpips"}
    for k in ("ssim", "psnr", "l1"):
        assert out[k] == plain[k] and torch.equal(out["per_view"][k], plain["per_view"][k])
    want = [crit()(r[None], c.original_image[None]).item() for c, r in zip(cams, renders)]
    print("lpips per view", want)
    assert out["per_view"]["lpips"].shape == (3,) and [float(v) for v in out["per_view"]["lpips"]] == want
    assert min(want) > 0 and abs(out["lpips"] - sum(want) / 3) <= 1e-9
