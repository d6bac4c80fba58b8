"""The resized HVS loss (MetamericLossUniform(..., resize=...): the bilinear resize to the pyramid's size in k_hvs_level's level-0
load, its adjoint the gather k_hvs_bwd_resize, csrc/hvs.hip) on the GPU against the float64 yardstick of
tests/hvs_resize_cases.py (F.interpolate in float64, then tests/hvs_ref.hvs_loss, autograd to the SOURCE picture). The allowance
is tests/hvs_cases.allowance, unchanged: 3 x the distance of the reference's OWN float32 run (tests/golden/ref_hvs_resize.npz)
from that yardstick, floor 16 fp32 epsilons; every figure is printed and recorded through tests/parity_report.py (kind "hvs").
R0 135x16 -> 136x16: the 1080 -> 1088 ratio, the lerp phase through a whole cycle, width identity; R1 the same on the other axis
(a swapped scale or stride); R2 21x30 -> 24x32 both axes, RGB and YCrCb (colour after the lerp); R3 33x17 -> 64x32 two or three
resized pixels per source pixel in the gather, tile seams, the reflected halo through the lerp; R4 1x5 -> 4x8 one source row."""
import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd.odak_perception import MetamericLossUniform, pyramid_size
from tests import hvs_cases as hc
from tests import hvs_resize_cases as rc
from tests import parity_report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPACES = [(i, cs) for i, c in enumerate(rc.CASES) for cs in c[-1]]


def _loss_fn(c, filters=None):
    return MetamericLossUniform(device=DEV, pooling_size=c.pooling, n_pyramid_levels=c.levels, n_orientations=c.orientations,
                                loss_type=c.loss_type, bilinear_downsampling=True,
                                filters=filters if filters is not None else rc.filters_of(c))


def _run(fn, img_np, tgt_np, resize, colorspace="RGB", upstream=None, dtype=torch.float32):
    img = torch.tensor(img_np, device=DEV).to(dtype).requires_grad_(True)
    tgt = torch.tensor(tgt_np, device=DEV)
    loss = fn(img, tgt, image_colorspace=colorspace, resize=resize)
    (loss if upstream is None else loss * upstream).backward()
    return loss.detach(), img.grad


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("i,colorspace", SPACES)
def test_resized_loss_and_gradient_match_the_float64_yardstick(i, colorspace):
    c, y = rc.case(i), rc.yardstick(i, colorspace)
    ref_loss, ref_grad = rc.reference(i, colorspace)
    loss, grad = _run(_loss_fn(c), c.img, c.tgt, (c.H, c.W), colorspace)
    assert loss.dim() == 0 and loss.device.type == "cuda" and grad.shape == (1, 3, c.Hs, c.Ws)  # the SOURCE shape
    got_loss, got_grad = float(loss), grad.cpu().numpy()
    ref_rel = abs(ref_loss - y["loss"]) / abs(y["loss"])
    ref_l2, ref_mx = hc.distances(ref_grad, y["grad"])
    rel = abs(got_loss - y["loss"]) / abs(y["loss"])
    l2, mx = hc.distances(got_grad, y["grad"])
    name = f"R{i}" + ("" if colorspace == "RGB" else "/YCrCb")
    parity_report.record("hvs", name, rel_loss=rel, ref_rel_loss=ref_rel, grad_rel_l2=l2, ref_grad_rel_l2=ref_l2,
                         grad_max_over_max=mx, ref_grad_max_over_max=ref_mx)
    print(f"{name}: rel loss {rel:.3e} (reference {ref_rel:.3e}) grad rel L2 {l2:.3e} (reference {ref_l2:.3e}) "
          f"max/max {mx:.3e} (reference {ref_mx:.3e})")
    assert np.isfinite(got_grad).all()
    assert rel <= hc.allowance(ref_rel), (rel, ref_rel)
    assert l2 <= hc.allowance(ref_l2), (l2, ref_l2)
    assert mx <= hc.allowance(ref_mx), (mx, ref_mx)


def test_pyramid_keyword_size_tuple_and_pyramid_size_agree():
    c = rc.case(2)
    assert pyramid_size(c.Hs, c.Ws, c.levels) == (c.H, c.W)
    a = _run(_loss_fn(c), c.img, c.tgt, "pyramid")
    b = _run(_loss_fn(c), c.img, c.tgt, (c.H, c.W))
    d = _run(_loss_fn(c), c.img, c.tgt, pyramid_size(c.Hs, c.Ws, c.levels))
    assert _same(a, b) and _same(a, d)


@pytest.mark.parametrize("edge,resize", [(3, (8, 8)), (4, "pyramid")])
def test_a_resize_to_the_own_size_is_the_plain_call(edge, resize):
    c = hc.edge_case(edge)
    assert pyramid_size(c.H, c.W, c.levels) == (c.H, c.W)
    plain = _run(_loss_fn(c, hc.filters_of(c)), c.img, c.tgt, None)
    same = _run(_loss_fn(c, hc.filters_of(c)), c.img, c.tgt, resize)
    assert same[1].shape == (1, 3, c.H, c.W) and _same(plain, same)


def test_two_resized_calls_are_bit_identical():
    c = rc.case(3)
    assert _same(_run(_loss_fn(c), c.img, c.tgt, (c.H, c.W)), _run(_loss_fn(c), c.img, c.tgt, (c.H, c.W)))


def test_upstream_gradient_and_half_precision_source():
    c = rc.case(2)
    _, g1 = _run(_loss_fn(c), c.img, c.tgt, "pyramid")
    _, g2 = _run(_loss_fn(c), c.img, c.tgt, "pyramid", upstream=-2.5)
    assert torch.equal(g2, g1 * -2.5)  # one exact scaling of every element
    loss, grad = _run(_loss_fn(c), c.img, c.tgt, "pyramid", dtype=torch.float16)
    assert grad.dtype == torch.float16 and grad.shape == (1, 3, c.Hs, c.Ws)
    img16 = torch.tensor(c.img).half().float().numpy()  # the image was rounded to half before the call
    loss32, grad32 = _run(_loss_fn(c), img16, c.tgt, "pyramid")
    assert float(loss) == float(loss32) and torch.equal(grad, grad32.half())


def test_resized_target_state():
    c = rc.case(4)
    fn = _loss_fn(c)
    img = torch.tensor(c.img, device=DEV)
    tgt = torch.tensor(c.tgt, device=DEV)

    def run(f, t, resize):
        x = img.clone().requires_grad_(True)
        l = f(x, t, resize=resize)
        l.backward()
        return l.detach().clone(), x.grad.clone()

    first = run(fn, tgt, (4, 8))
    assert fn._target is not None and fn._target[0]() is tgt
    state = fn._target[2]
    again = run(fn, tgt, (4, 8))                    # the same object, unchanged: its state is reused ...
    assert fn._target[2] is state
    assert _same(first, again) and _same(first, run(_loss_fn(c), tgt.clone(), (4, 8)))  # ... and gives a fresh object's result
    larger = run(fn, tgt, (8, 8))                   # the same object with another resize size: recomputed
    assert fn._target[2] is not state and fn._target[2].numel() != state.numel()
    # (one source row resizes to equal rows at either height, so the two LOSSES agree; the state's size shows the recomputation)
    assert _same(larger, run(_loss_fn(c), tgt.clone(), (8, 8)))
    back = run(fn, tgt, (4, 8))
    assert _same(back, first)
    state = fn._target[2]
    other = torch.tensor(c.img[:, [2, 0, 1]], device=DEV)
    tgt.copy_(other)                                # modified in place: the new target's loss
    changed = run(fn, tgt, (4, 8))
    assert fn._target[2] is not state
    assert _same(changed, run(_loss_fn(c), other.clone(), (4, 8))) and not torch.equal(changed[0], first[0])


def test_three_dimensional_input_under_no_grad():
    c = rc.case(0)
    with torch.no_grad():
        a = _loss_fn(c)(torch.tensor(c.img[0], device=DEV), torch.tensor(c.tgt[0], device=DEV), resize="pyramid")
    b, _ = _run(_loss_fn(c), c.img, c.tgt, "pyramid")
    assert torch.equal(a, b)
