"""The fused foveated HVS loss (fov3dgs_amd.odak_perception.MetamericLoss, csrc/hvs_fov.hip) on the GPU against the float64
restatement (tests/hvs_fov_ref.py). The allowance of every figure is tests/hvs_cases.py's rule, unchanged: 3 x the distance of the
reference's OWN float32 run (tests/golden/ref_hvs_fov.npz) from that yardstick, with a floor of 16 fp32 epsilons; every measured
figure, the library's and the reference's, is printed and recorded through tests/parity_report.py (kind "hvs_fov").
Cases (tests/golden/make_hvs_fov_golden.py): F0 HVSLoss's defaults, F1 a chain that ends 1x2 with the appended mean sampled, F2 LOD
up to 5 of a 7-level chain, F3 tall with two orientations and YCrCb input, F4 odd mip sizes and lod >= K, F5 lod = 0 everywhere
(L1 and MSE), F6 the gaze outside the picture."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd.hvs_loss_calc import HVSLoss
from fov3dgs_amd.odak_perception import MetamericLoss, MetamericLossUniform, _native_hvs_fov
from tests import hvs_cases as hc
from tests import hvs_fov_cases as fc
from tests import hvs_fov_ref, hvs_ref, parity_report

pytestmark = pytest.mark.gpu
CASES = list(range(8))
DEV = "cuda:0"


def _loss_fn(c, **kw):
    return MetamericLoss(device=DEV, alpha=c.alpha, real_image_width=c.width, real_viewing_distance=c.distance,
                         n_pyramid_levels=c.levels, mode=c.mode, n_orientations=c.orientations, use_l2_foveal_loss=False,
                         loss_type=c.loss_type, use_bilinear_downup=True, filters=hc.filters(c.orientations), **kw)


def _run(fn, c, img_np=None, tgt_np=None, gaze=None, upstream=None, **kw):
    img = torch.tensor(c.img if img_np is None else img_np, device=DEV).requires_grad_(True)
    tgt = torch.tensor(c.tgt if tgt_np is None else tgt_np, device=DEV)
    loss = fn(img, tgt, gaze=list(c.gaze if gaze is None else gaze), image_colorspace=c.colorspace, **kw)
    (loss if upstream is None else loss * upstream).backward()
    return loss.detach(), img.grad


def _check(name, got_loss, got_grad, y, ref_loss, ref_grad):
    """library vs yardstick within 3 x (reference vs yardstick), floor 16 eps: loss, gradient rel L2, gradient max/max"""
    ref_rel = abs(ref_loss - y["loss"]) / abs(y["loss"])
    ref_l2, ref_mx = hc.distances(ref_grad, y["grad"])
    rel = abs(got_loss - y["loss"]) / abs(y["loss"])
    l2, mx = hc.distances(got_grad, y["grad"])
    parity_report.record("hvs_fov", name, rel_loss=rel, ref_rel_loss=ref_rel, grad_rel_l2=l2, ref_grad_rel_l2=ref_l2,
                         grad_max_over_max=mx, ref_grad_max_over_max=ref_mx)
    print(f"{name}: rel loss {rel:.3e} (reference {ref_rel:.3e}) grad rel L2 {l2:.3e} (reference {ref_l2:.3e}) "
          f"max/max {mx:.3e} (reference {ref_mx:.3e})")
    assert np.isfinite(got_grad).all()
    assert rel <= hc.allowance(ref_rel), (rel, ref_rel)
    assert l2 <= hc.allowance(ref_l2), (l2, ref_l2)
    assert mx <= hc.allowance(ref_mx), (mx, ref_mx)


@pytest.mark.parametrize("i", CASES)
def test_loss_and_gradient_match_the_float64_restatement(i):
    c, z, y = fc.case(i), fc.golden(), fc.yardstick(i)
    loss, grad = _run(_loss_fn(c), c)
    assert loss.dim() == 0 and loss.device.type == "cuda" and grad.shape == (1, 3, c.H, c.W)
    _check(c.name, float(loss), grad.cpu().numpy(), y, float(z[f"loss_{i}"]), z[f"grad_{i}"])


@pytest.mark.parametrize("i", CASES)
def test_lod_maps_match_the_stored_ones(i):
    """the maps the kernels build against the float64 yardstick, within the rule's allowance of the reference's own float32
    maps (max absolute difference: a LOD map can be 0 everywhere)"""
    c, z, y = fc.case(i), fc.golden(), fc.yardstick(i)
    got = _loss_fn(c).lod_maps(c.H, c.W, gaze=list(c.gaze))
    assert len(got) == c.levels - 1
    for l, m in enumerate(got):
        assert m.dtype == torch.float64 and tuple(m.shape) == (c.H >> l, c.W >> l)
        ref_d, d = fc.max_abs(z[f"lod_{i}_{l}"], y["lods"][l]), fc.max_abs(m.cpu().numpy(), y["lods"][l])
        parity_report.record("hvs_fov", f"{c.name}/lod{l}", max_abs=d, ref_max_abs=ref_d)
        print(f"{c.name} level {l}: LOD map max |d| {d:.3e} (reference {ref_d:.3e})")
        assert d <= hc.allowance(ref_d), (l, d, ref_d)


def _blend(chain, lod):
    """the blur's blend (tests/hvs_fov_ref.blur) of a GIVEN chain [level 0 .. level K], float64"""
    K, x = len(chain) - 1, chain[0]
    up = [x] + [F.interpolate(m, size=x.shape[-2:], mode="bilinear", align_corners=False) for m in chain[1:K]] + [chain[K].expand_as(x)]
    frac, out = torch.fmod(lod, 1.0), torch.zeros_like(x)
    for l in range(K + 1):
        mask = (lod >= l) if l == K else ((lod < l + 1) if l == 0 else ((lod >= l) & (lod < l + 1)))
        out = torch.where(mask, up[l] if l == K else (1 - frac) * up[l] + frac * up[l + 1], out)
    return out


def _library_statistics(c, want):
    """the statistics `want` (indices in the reference's list) of the image, rebuilt from the state the kernels keep: the two
    mip chains are sampled and blended here in float64, with the library's own LOD maps, as k_fov_cmp does per pixel"""
    fn = _loss_fn(c)
    img = torch.tensor(c.img, device=DEV)
    loss = fn(img, img, gaze=list(c.gaze), image_colorspace=c.colorspace)  # the image as its own target: the kept state is the image's
    assert float(loss) == 0.0
    st = fn._target[1][-1]
    s, lods = fn._target[2].cpu().double(), fn._lod[2].cpu()
    lv = _native_hvs_fov.layout(st)
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
        lod = lods[v["lod"]:v["lod"] + h * w].reshape(h, w)

        def level(offsets, kk, hk, wk):
            o = offsets[kk] + mi * 3 * hk * wk
            return s[o:o + 3 * hk * wk].reshape(1, 3, hk, wk)
        band = s[v["maps"] + mi * 3 * h * w: v["maps"] + (mi + 1) * 3 * h * w].reshape(1, 3, h, w)
        mean = _blend([band] + [level(v["mean"], kk, *v["chain"][kk]) for kk in range(1, len(v["chain"]))], lod)
        if k % 2 == 0:
            out[k] = mean.numpy()
            continue
        msq = _blend([band * band] + [level(v["square"], kk, *v["chain"][kk]) for kk in range(1, len(v["chain"]))], lod)
        out[k] = torch.sqrt(torch.clamp(msq - mean * mean, min=1e-7)).numpy()
    return out


@pytest.mark.parametrize("i", CASES)
def test_stored_statistic_maps(i):
    c, z, y = fc.case(i), fc.golden(), fc.yardstick(i)
    idx = [int(v) for v in z[f"mapidx_{i}"]]
    got = _library_statistics(c, idx)
    for name, k in zip(("map0", "mapmid", "mapstd", "maplow"), idx):
        _, ref_mx = hc.distances(z[f"{name}_{i}"], y["maps"][k])
        _, mx = hc.distances(got[k], y["maps"][k])
        parity_report.record("hvs_fov", f"{c.name}/{name}", max_over_max=mx, ref_max_over_max=ref_mx)
        print(f"{c.name}/{name} (statistic {k}): max/max {mx:.3e} (reference {ref_mx:.3e})")
        assert got[k].shape == y["maps"][k].shape
        assert mx <= hc.allowance(ref_mx), (name, mx, ref_mx)


@pytest.mark.parametrize("i", [1, 4])
def test_two_calls_are_bit_identical(i):
    c = fc.case(i)
    a, b = _run(_loss_fn(c), c), _run(_loss_fn(c), c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_upstream_gradient_other_than_one():
    c = fc.case(2)
    _, g1 = _run(_loss_fn(c), c)
    _, g2 = _run(_loss_fn(c), c, upstream=-2.5)
    assert torch.equal(g2, g1 * -2.5)  # one exact scaling of every element


def test_kept_target_and_lod_maps_never_decide_a_result():
    c = fc.case(2)
    fn = _loss_fn(c)
    img = torch.tensor(c.img, device=DEV)
    tgt = torch.tensor(c.tgt, device=DEV)

    def run(f, t, gaze):
        x = img.clone().requires_grad_(True)
        l = f(x, t, gaze=gaze)
        l.backward()
        return l.detach().clone(), x.grad.clone()

    first = run(fn, tgt, [0.5, 0.5])
    assert fn._target is not None and fn._target[0]() is tgt and fn._lod[3]
    state, lod = fn._target[2], fn._lod[2]
    again = run(fn, tgt, [0.5, 0.5])               # the same object, unchanged, the same gaze: nothing is recomputed ...
    assert fn._target[2] is state and fn._lod[2] is lod
    fresh = run(_loss_fn(c), tgt.clone(), [0.5, 0.5])  # ... and the result is a fresh object's
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert torch.equal(first[0], fresh[0]) and torch.equal(first[1], fresh[1])
    # the same target with another gaze: recomputed (the reference would keep the first gaze's target statistics)
    moved = run(fn, tgt, [0.2, 0.7])
    assert fn._target[2] is not state and fn._lod[2] is not lod
    want = run(_loss_fn(c), tgt.clone(), [0.2, 0.7])
    assert torch.equal(moved[0], want[0]) and torch.equal(moved[1], want[1])
    assert not torch.equal(moved[0], first[0])
    y = fc.restate(c, torch.float64, gaze=(0.2, 0.7))
    assert abs(float(moved[0]) - y["loss"]) / y["loss"] < 1e-4   # and it is the loss AT that gaze
    # modified in place: the new target's loss
    other = torch.tensor(c.img[:, [2, 0, 1]], device=DEV)
    tgt.copy_(other)
    changed = run(fn, tgt, [0.2, 0.7])
    want = run(_loss_fn(c), other.clone(), [0.2, 0.7])
    assert torch.equal(changed[0], want[0]) and torch.equal(changed[1], want[1])
    assert not torch.equal(changed[0], moved[0])


def test_resize_to_the_pyramid_size_inside_the_kernels():
    """a 30x60 pair with resize="pyramid" (-> 32x64) equals the yardstick with F.interpolate in front; the allowance's base is
    the reference's float32 distance on F0 (the same settings and size, measured on its own pictures)"""
    i = 0
    c, z, y0 = fc.case(i), fc.golden(), fc.yardstick(i)
    img_np, tgt_np = np.ascontiguousarray(c.img[..., :30, :60]), np.ascontiguousarray(c.tgt[..., :30, :60])
    x = torch.tensor(img_np, dtype=torch.float64, requires_grad=True)
    up = lambda t: F.interpolate(t, size=(32, 64), mode="bilinear", align_corners=False)
    f64 = hvs_ref.filters_to(hc.filters(c.orientations), dtype=torch.float64)
    want = hvs_fov_ref.fov_loss(up(x), up(torch.tensor(tgt_np, dtype=torch.float64)), f64, c.gaze, c.alpha, c.width, c.distance,
                                c.levels, c.mode, c.loss_type)
    want.backward()
    want = want.detach()
    loss, grad = _run(_loss_fn(c), c, img_np, tgt_np, resize="pyramid")
    assert grad.shape == (1, 3, 30, 60)
    ref_rel = abs(float(z[f"loss_{i}"]) - y0["loss"]) / y0["loss"]
    ref_l2, ref_mx = hc.distances(z[f"grad_{i}"], y0["grad"])
    rel = abs(float(loss) - float(want)) / float(want)
    l2, mx = hc.distances(grad.cpu().numpy(), x.grad.numpy())
    parity_report.record("hvs_fov", "F0/resized30x60", rel_loss=rel, ref_rel_loss=ref_rel, grad_rel_l2=l2, ref_grad_rel_l2=ref_l2,
                         grad_max_over_max=mx, ref_grad_max_over_max=ref_mx)
    print(f"resized: rel loss {rel:.3e} ({ref_rel:.3e}) grad rel L2 {l2:.3e} ({ref_l2:.3e}) max/max {mx:.3e} ({ref_mx:.3e})")
    assert rel <= hc.allowance(ref_rel) and l2 <= hc.allowance(ref_l2) and mx <= hc.allowance(ref_mx)
    # resize to the pictures' own size is the plain call, bit for bit
    a, b = _run(_loss_fn(c), c, resize="pyramid"), _run(_loss_fn(c), c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_hvsloss_calls_equal_the_direct_calls():
    c = fc.case(0)   # HVSLoss's defaults
    hvs = HVSLoss(filters=hc.filters(6))
    img_np, tgt_np = np.ascontiguousarray(c.img[..., :30, :60]), np.ascontiguousarray(c.tgt[..., :30, :60])

    def run(f):
        x = torch.tensor(img_np, device=DEV).requires_grad_(True)
        l = f(x, torch.tensor(tgt_np, device=DEV))
        l.backward()
        return l.detach(), x.grad

    for gaze in ([0.5, 0.5], [0.1, 0.1]):
        a = run(lambda x, t: hvs.calc_fov_loss(x, t, gaze=gaze))
        b = run(lambda x, t: _loss_fn(c)(x, t, gaze=gaze, resize="pyramid"))
        assert a[1].shape == (1, 3, 30, 60) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for pooling in (1, 9):   # assigned per call
        a = run(lambda x, t: hvs.calc_uniform_loss(x, t, pooling_size=pooling))
        direct = MetamericLossUniform(device=DEV, pooling_size=pooling, n_pyramid_levels=5, n_orientations=6, loss_type="MSE",
                                      bilinear_downsampling=True, filters=hc.filters(6))
        b = run(lambda x, t: direct(x, t, resize="pyramid"))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert hvs.uniform_loss.pooling_size == 9


def test_three_dimensional_input_no_grad_and_half_precision():
    c = fc.case(4)
    fn = _loss_fn(c)
    with torch.no_grad():
        a = fn(torch.tensor(c.img[0], device=DEV), torch.tensor(c.tgt[0], device=DEV), gaze=list(c.gaze))
    b, _ = _run(_loss_fn(c), c)
    assert torch.equal(a, b)
    img16 = torch.tensor(c.img, device=DEV).half().requires_grad_(True)
    loss = _loss_fn(c)(img16, torch.tensor(c.tgt, device=DEV), gaze=list(c.gaze))
    loss.backward()
    loss32, grad32 = _run(_loss_fn(c), c, torch.tensor(c.img).half().float().numpy())
    assert img16.grad.dtype == torch.float16 and float(loss.detach()) == float(loss32) and torch.equal(img16.grad, grad32.half())
