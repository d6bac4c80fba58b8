"""The fused HVS loss (fov3dgs_amd.odak_perception.MetamericLossUniform, csrc/hvs.hip) on the GPU against the float64
restatement (tests/hvs_ref.py). The allowance of every figure is 3 x the distance of the reference's OWN float32 run
(tests/golden/ref_hvs.npz) from that yardstick, with a floor of 16 fp32 epsilons (tests/hvs_cases.py); every measured figure,
the library's and the reference's, is printed and recorded through tests/parity_report.py (kind "hvs").
The test_edge_* tests run the second fixture (tests/golden/ref_hvs_edges.npz, E0 .. E7) under the same rule, each case against
its own reference vector: E0, E1 pooled maps larger than the band (ph > h: k_hvs_pool, k_hvs_bwd_up's footprints, hvs_g_at's
window gather), E2 one orientation, E3 pooling 0.75 on a picture smaller than a tile with two levels, E4 tile remainders 8, 8
and 12, 4, E5 one pooled row (hvs_lerp with n_in = 1) in RGB and YCrCb, E6 one pooled column, E7 six levels and eight
orientations with a 4x4 identity level. E2 .. E7 use asymmetric filters: a tap index swapped or mirrored in k_hvs_level or
hvs_convT, which the reference's own symmetric filters hide from the seven cases, moves these results."""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd.odak_perception import MetamericLossUniform, _native_hvs
from tests import hvs_cases as hc
from tests import hvs_ref, parity_report

pytestmark = pytest.mark.gpu
CASES = list(range(7))
DEV = "cuda:0"


def _loss_fn(c, **kw):
    return MetamericLossUniform(device=DEV, pooling_size=c.pooling, n_pyramid_levels=c.levels, n_orientations=c.orientations,
                                loss_type=c.loss_type, bilinear_downsampling=True, filters=hc.filters_of(c), **kw)


def _run(fn, img_np, tgt_np, colorspace="RGB", upstream=None, dtype=torch.float32):
    img = torch.tensor(img_np, device=DEV).to(dtype).requires_grad_(True)
    tgt = torch.tensor(tgt_np, device=DEV)
    loss = fn(img, tgt, image_colorspace=colorspace)
    (loss if upstream is None else loss * upstream).backward()
    return loss.detach(), img.grad


def _check(name, got_loss, got_grad, y, ref_loss, ref_grad):
    """library vs yardstick within 3 x (reference vs yardstick), floor 16 eps: loss, gradient rel L2, gradient max/max"""
    ref_rel = abs(ref_loss - y["loss"]) / abs(y["loss"])
    ref_l2, ref_mx = hc.distances(ref_grad, y["grad"])
    rel = abs(got_loss - y["loss"]) / abs(y["loss"])
    l2, mx = hc.distances(got_grad, y["grad"])
    parity_report.record("hvs", name, rel_loss=rel, ref_rel_loss=ref_rel, grad_rel_l2=l2, ref_grad_rel_l2=ref_l2,
                         grad_max_over_max=mx, ref_grad_max_over_max=ref_mx)
    print(f"{name}: rel loss {rel:.3e} (reference {ref_rel:.3e}) grad rel L2 {l2:.3e} (reference {ref_l2:.3e}) "
          f"max/max {mx:.3e} (reference {ref_mx:.3e})")
    assert np.isfinite(got_grad).all()
    assert rel <= hc.allowance(ref_rel), (rel, ref_rel)
    assert l2 <= hc.allowance(ref_l2), (l2, ref_l2)
    assert mx <= hc.allowance(ref_mx), (mx, ref_mx)


@pytest.mark.parametrize("i", CASES)
def test_loss_and_gradient_match_the_float64_restatement(i):
    c, z, y = hc.case(i), hc.golden(), hc.yardstick(i)
    loss, grad = _run(_loss_fn(c), c.img, c.tgt)
    assert loss.dim() == 0 and loss.device.type == "cuda" and grad.shape == (1, 3, c.H, c.W)
    _check(f"case{i}", float(loss), grad.cpu().numpy(), y, float(z[f"loss_{i}"]), z[f"grad_{i}"])


def _library_statistics(c, want):
    """the statistics `want` (indices in the reference's list) of the image, rebuilt from the state the kernels keep: the
    pooled mean / mean-square are bilinearly up-sampled here in float64, as the comparison kernel samples them"""
    fn = _loss_fn(c)
    img = torch.tensor(c.img, device=DEV)
    st = fn._settings(c.H, c.W, True)
    state = torch.empty(_native_hvs.floats(st, 0), dtype=torch.float32, device=DEV)
    state_t, fresh = fn._target_state(img, img.reshape(3, c.H, c.W), st)
    # one forward with the image as its own target: the image's state is what is looked at
    loss = _native_hvs.HvsLoss.apply(img, img.reshape(3, c.H, c.W), state_t, fn._filters_on(img.device), st)
    assert float(loss) == 0.0
    s = state_t.cpu().double()
    lv = _native_hvs.layout(st)
    out = {}
    for k in want:
        if k == hvs_ref.n_stats(c.levels, c.orientations) - 1:
            o, h, w = lv[-1]["low_out"], lv[-1]["h"] // 2, lv[-1]["w"] // 2
            out[k] = s[o:o + 3 * h * w].reshape(1, 3, h, w).numpy()
            continue
        m = k // 2                                   # map number: 0 = h, then the bands level by level
        l = 0 if m == 0 else (m - 1) // c.orientations
        mi = m if l == 0 else (m - 1) % c.orientations
        v = lv[l]
        h, w = v["h"], v["w"]
        if v["identity"]:
            band = s[v["maps"] + mi * 3 * h * w: v["maps"] + (mi + 1) * 3 * h * w].reshape(1, 3, h, w)
            out[k] = (band if k % 2 == 0 else torch.full_like(band, 1e-7).sqrt()).numpy()
            continue
        n = 3 * v["ph"] * v["pw"]
        mean = s[v["pool"] + mi * n: v["pool"] + (mi + 1) * n].reshape(1, 3, v["ph"], v["pw"])
        msq = s[v["pool"] + (v["nm"] + mi) * n: v["pool"] + (v["nm"] + mi + 1) * n].reshape(1, 3, v["ph"], v["pw"])
        mean_up = F.interpolate(mean, size=(h, w), mode="bilinear")
        var = F.interpolate(msq, size=(h, w), mode="bilinear") - mean_up * mean_up
        out[k] = (mean_up if k % 2 == 0 else torch.sqrt(torch.clamp(var, min=1e-7))).numpy()
    return out


@pytest.mark.parametrize("i", CASES)
def test_stored_statistic_maps(i):
    c, z, y = hc.case(i), hc.golden(), hc.yardstick(i)
    idx = [int(v) for v in z[f"mapidx_{i}"]]
    got = _library_statistics(c, idx)
    for name, k in zip(("map0", "mapmid", "mapstd", "maplow"), idx):
        _, ref_mx = hc.distances(z[f"{name}_{i}"], y["maps"][k])
        _, mx = hc.distances(got[k], y["maps"][k])
        parity_report.record("hvs", f"case{i}/{name}", max_over_max=mx, ref_max_over_max=ref_mx)
        print(f"case{i}/{name} (statistic {k}): max/max {mx:.3e} (reference {ref_mx:.3e})")
        assert got[k].shape == y["maps"][k].shape
        assert mx <= hc.allowance(ref_mx), (name, mx, ref_mx)


def test_upstream_gradient_other_than_one():
    c = hc.case(0)
    _, g1 = _run(_loss_fn(c), c.img, c.tgt)
    _, g2 = _run(_loss_fn(c), c.img, c.tgt, upstream=-2.5)
    assert torch.equal(g2, g1 * -2.5)  # one exact scaling of every element


def test_half_precision_image_gets_a_half_gradient():
    c, y = hc.case(2), hc.yardstick(2)
    loss, grad = _run(_loss_fn(c), c.img, c.tgt, dtype=torch.float16)
    assert grad.dtype == torch.float16 and grad.shape == (1, 3, c.H, c.W)
    # the image was rounded to half before the call: compare with the fp32 call on that rounded image
    img16 = torch.tensor(c.img).half().float().numpy()
    loss32, grad32 = _run(_loss_fn(c), img16, c.tgt)
    assert float(loss) == float(loss32)
    assert torch.equal(grad, grad32.half())


@pytest.mark.parametrize("i", [1, 3])
def test_two_calls_are_bit_identical(i):
    c = hc.case(i)
    a = _run(_loss_fn(c), c.img, c.tgt)
    b = _run(_loss_fn(c), c.img, c.tgt)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_target_state_reuse_never_decides_a_result():
    c = hc.case(1)
    fn = _loss_fn(c)
    img = torch.tensor(c.img, device=DEV)
    tgt = torch.tensor(c.tgt, device=DEV)

    def run(f, t):
        x = img.clone().requires_grad_(True)
        l = f(x, t)
        l.backward()
        return l.detach().clone(), x.grad.clone()

    first = run(fn, tgt)
    assert fn._target is not None and fn._target[0]() is tgt
    state = fn._target[2]
    again = run(fn, tgt)                       # the same object, unchanged: its state is reused ...
    assert fn._target[2] is state
    fresh = run(_loss_fn(c), tgt.clone())      # ... and gives what a fresh object gives
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert torch.equal(first[0], fresh[0]) and torch.equal(first[1], fresh[1])
    # modified in place: the new target's loss
    other = torch.tensor(hc.case(1).img[:, [2, 0, 1]], device=DEV)
    tgt.copy_(other)
    changed = run(fn, tgt)
    assert fn._target[2] is not state
    want = run(_loss_fn(c), other.clone())
    assert torch.equal(changed[0], want[0]) and torch.equal(changed[1], want[1])
    assert not torch.equal(changed[0], first[0])
    # a new tensor at a freed target's address: its own loss
    t1 = torch.tensor(c.tgt, device=DEV)
    r1 = run(fn, t1)
    addr = t1.data_ptr()
    del t1
    gc.collect()
    t2 = torch.empty_like(other)
    t2.copy_(other)
    r2 = run(fn, t2)
    print("new target at the freed address:", t2.data_ptr() == addr)
    assert torch.equal(r2[0], want[0]) and torch.equal(r2[1], want[1]) and torch.equal(r1[0], first[0])


def test_ycrcb_path():
    i = 6
    c, z = hc.case(i), hc.golden()
    y = hc.yardstick(i, "YCrCb")
    loss, grad = _run(_loss_fn(c), c.img, c.tgt, colorspace="YCrCb")
    # the reference's float32 distance of this case (measured on its RGB run) is the allowance's base
    y_rgb = hc.yardstick(i)
    ref_rel = abs(float(z[f"loss_{i}"]) - y_rgb["loss"]) / y_rgb["loss"]
    ref_l2, ref_mx = hc.distances(z[f"grad_{i}"], y_rgb["grad"])
    rel = abs(float(loss) - y["loss"]) / y["loss"]
    l2, mx = hc.distances(grad.cpu().numpy(), y["grad"])
    parity_report.record("hvs", "case6/YCrCb", rel_loss=rel, ref_rel_loss=ref_rel, grad_rel_l2=l2, ref_grad_rel_l2=ref_l2,
                         grad_max_over_max=mx, ref_grad_max_over_max=ref_mx)
    print(f"YCrCb: rel loss {rel:.3e} ({ref_rel:.3e}) grad rel L2 {l2:.3e} ({ref_l2:.3e}) max/max {mx:.3e} ({ref_mx:.3e})")
    assert rel <= hc.allowance(ref_rel) and l2 <= hc.allowance(ref_l2) and mx <= hc.allowance(ref_mx)


# ---------------------------------------------------------------- the second fixture: ref_hvs_edges.npz (E0 .. E7)
EDGES = list(range(hc.EDGES))


def _edge_reference(i, colorspace="RGB"):
    z, tag = hc.edges(), "" if colorspace == "RGB" else "_ycrcb"
    return float(z[f"loss_{i}{tag}"]), z[f"grad_{i}{tag}"]


@pytest.mark.parametrize("i", EDGES)
def test_edge_loss_and_gradient_match_the_float64_restatement(i):
    c, y = hc.edge_case(i), hc.edge_yardstick(i)
    loss, grad = _run(_loss_fn(c), c.img, c.tgt)
    assert loss.dim() == 0 and loss.device.type == "cuda" and grad.shape == (1, 3, c.H, c.W)
    _check(f"E{i}", float(loss), grad.cpu().numpy(), y, *_edge_reference(i))


@pytest.mark.parametrize("i", EDGES)
def test_edge_stored_statistic_maps(i):
    """E0, E1, E2 (and E3) compare a pooled level with ph > h map against map, E5 and E6 a level of one row / one column"""
    c, z, y = hc.edge_case(i), hc.edges(), hc.edge_yardstick(i)
    idx = [int(v) for v in z[f"mapidx_{i}"]]
    got = _library_statistics(c, idx)
    for name, k in zip(("map0", "mapmid", "mapstd", "maplow"), idx):
        _, ref_mx = hc.distances(z[f"{name}_{i}"], y["maps"][k])
        _, mx = hc.distances(got[k], y["maps"][k])
        parity_report.record("hvs", f"E{i}/{name}", max_over_max=mx, ref_max_over_max=ref_mx)
        print(f"E{i}/{name} (statistic {k}): max/max {mx:.3e} (reference {ref_mx:.3e})")
        assert got[k].shape == y["maps"][k].shape
        assert mx <= hc.allowance(ref_mx), (name, mx, ref_mx)


def test_edge_ycrcb_against_its_own_reference_vector():
    c, y = hc.edge_case(5), hc.edge_yardstick(5, "YCrCb")
    loss, grad = _run(_loss_fn(c), c.img, c.tgt, colorspace="YCrCb")
    _check("E5/YCrCb", float(loss), grad.cpu().numpy(), y, *_edge_reference(5, "YCrCb"))


@pytest.mark.parametrize("i", [1, 4])
def test_edge_two_calls_are_bit_identical(i):
    c = hc.edge_case(i)
    a = _run(_loss_fn(c), c.img, c.tgt)
    b = _run(_loss_fn(c), c.img, c.tgt)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_edge_target_state_reuse_never_decides_a_result():
    """test_target_state_reuse_never_decides_a_result's equalities where the kept state holds pooled maps larger than a band"""
    c = hc.edge_case(0)
    fn = _loss_fn(c)
    img = torch.tensor(c.img, device=DEV)
    tgt = torch.tensor(c.tgt, device=DEV)

    def run(f, t):
        x = img.clone().requires_grad_(True)
        l = f(x, t)
        l.backward()
        return l.detach().clone(), x.grad.clone()

    first = run(fn, tgt)
    assert fn._target is not None and fn._target[0]() is tgt
    state = fn._target[2]
    again = run(fn, tgt)
    assert fn._target[2] is state
    fresh = run(_loss_fn(c), tgt.clone())
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert torch.equal(first[0], fresh[0]) and torch.equal(first[1], fresh[1])
    other = torch.tensor(c.img[:, [2, 0, 1]], device=DEV)
    tgt.copy_(other)                           # modified in place: the new target's loss
    changed = run(fn, tgt)
    assert fn._target[2] is not state
    want = run(_loss_fn(c), other.clone())
    assert torch.equal(changed[0], want[0]) and torch.equal(changed[1], want[1])
    assert not torch.equal(changed[0], first[0])


def test_one_loss_object_with_several_settings():
    """one object (E3's: pooling 0.75, two levels, one orientation) called with E3's pictures (8x8), with E6's (36x20, where its
    pooled map is 48x26), with E3's again: every result is a fresh object's, bit for bit; the workspace is planned per size"""
    c3, c6 = hc.edge_case(3), hc.edge_case(6)
    fn = _loss_fn(c3)
    small = _run(fn, c3.img, c3.tgt)
    large = _run(fn, c6.img, c6.tgt)
    small_again = _run(fn, c3.img, c3.tgt)
    fresh_small, fresh_large = _run(_loss_fn(c3), c3.img, c3.tgt), _run(_loss_fn(c3), c6.img, c6.tgt)
    assert small[1].shape == (1, 3, c3.H, c3.W) and large[1].shape == (1, 3, c6.H, c6.W)
    for got, want in ((small, fresh_small), (large, fresh_large), (small_again, fresh_small)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(small[0], large[0])


def test_edge_half_precision_image_gets_a_half_gradient():
    c = hc.edge_case(2)
    loss, grad = _run(_loss_fn(c), c.img, c.tgt, dtype=torch.float16)
    assert grad.dtype == torch.float16 and grad.shape == (1, 3, c.H, c.W)
    img16 = torch.tensor(c.img).half().float().numpy()
    loss32, grad32 = _run(_loss_fn(c), img16, c.tgt)
    assert float(loss) == float(loss32)
    assert torch.equal(grad, grad32.half())


def test_three_dimensional_input_and_no_grad():
    c = hc.case(0)
    fn = _loss_fn(c)
    with torch.no_grad():
        a = fn(torch.tensor(c.img[0], device=DEV), torch.tensor(c.tgt[0], device=DEV))
    b, _ = _run(_loss_fn(c), c.img, c.tgt)
    assert torch.equal(a, b)
