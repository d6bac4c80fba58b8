"""The fused metamer (fov3dgs_amd.odak_perception.MetamerMSELoss / pyramid_roundtrip, csrc/metamer.hip) on the GPU against the
float64 restatement (tests/metamer_ref.py) fed with the fixture's noise. Every element is compared; the allowance of a case is
4 x the distance of the reference's OWN float32 run from that yardstick, as stored in tests/golden/ref_metamer.npz
(tests/metamer_cases.allowance), in max |d| and in relative L2. Every measured figure is printed and recorded through
tests/parity_report.py (kind "metamer"). tests/test_metamer_cpu.py shows on the restatement that a synthesis which forgets one band
of one level, or the highpass term, lands at least 193 times outside these allowances."""
import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd.odak_perception import MetamerMSELoss, pyramid_roundtrip
from tests import hvs_cases as hc
from tests import metamer_cases as mc
from tests import parity_report

pytestmark = pytest.mark.gpu
CASES = list(range(6))
DEV = "cuda:0"
EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)


def _fn(c, filters=None, **kw):
    args = dict(device=DEV, alpha=c.alpha, real_image_width=c.width, real_viewing_distance=c.distance, mode=c.mode,
                n_pyramid_levels=c.levels, n_orientations=c.orientations, loss_type=c.loss_type, avg_pooling_downup=True,
                filters=hc.filters(c.orientations) if filters is None else filters)
    args.update(kw)
    return MetamerMSELoss(**args)


def _metamer(c, filters=None):
    return _fn(c, filters).gen_metamer(torch.tensor(c.tgt, device=DEV), list(c.gaze), noise=torch.tensor(c.noise, device=DEV),
                                       image_colorspace=c.colorspace)


def _check(name, got, want, allowance, ref):
    mx, l2 = mc.distances(got, want)
    parity_report.record("metamer", name, max_abs=mx, rel_l2=l2, ref_max_abs=ref[0], ref_rel_l2=ref[1], n=int(np.asarray(want).size))
    print(f"{name}: max |d| {mx:.3e} (reference {ref[0]:.3e}, allowed {allowance[0]:.3e}) rel L2 {l2:.3e} (reference {ref[1]:.3e}, "
          f"allowed {allowance[1]:.3e})")
    assert np.isfinite(got).all()
    assert mx <= allowance[0], (mx, allowance[0])
    assert l2 <= allowance[1], (l2, allowance[1])


@pytest.mark.parametrize("i", CASES)
def test_metamer_matches_the_float64_restatement(i):
    c, z = mc.case(i), mc.golden()
    got = _metamer(c)
    assert got.shape == (1, 3, c.H, c.W) and got.dtype == torch.float32 and got.device.type == "cuda"
    _check(c.name, got.cpu().numpy(), mc.yardstick(i), mc.allowance(i), (float(z[f"ref_max_abs_{i}"]), float(z[f"ref_rel_l2_{i}"])))
    assert float(got.min()) < 0 and float(got.max()) > 1   # not clamped: the reference's metamer leaves [0, 1] too


@pytest.mark.parametrize("i", CASES)
def test_roundtrip_matches_the_float64_restatement(i):
    """the synthesis without the matching: reconstruct(construct(x))"""
    c, z = mc.case(i), mc.golden()
    x = torch.tensor(c.tgt, device=DEV)
    got = pyramid_roundtrip(x, c.levels, c.orientations, filters=hc.filters(c.orientations), image_colorspace=c.colorspace)
    assert got.shape == x.shape
    ref = (float(z[f"ref_rt_max_abs_{i}"]), float(z[f"ref_rt_rel_l2_{i}"]))
    _check(c.name + "/roundtrip", got.cpu().numpy(), mc.yardstick_roundtrip(i), (mc.FACTOR * ref[0], mc.FACTOR * ref[1]), ref)
    assert torch.equal(pyramid_roundtrip(x[0], c.levels, c.orientations, filters=hc.filters(c.orientations), image_colorspace=c.colorspace), got[0])


@pytest.mark.parametrize("i", [0, 1])
def test_asymmetric_filters(i):
    """seeded filters none of whose blocks equals a mirror image of itself: a flipped or transposed kernel fails (test_metamer_cpu.py
    shows by how much). Judged against the restatement alone -- the reference cannot be handed other filters -- with the allowance
    of the case: the same sums over the same shapes, the coefficients at most 1.25 times the reference's own."""
    c, z = mc.case(i), mc.golden()
    f = mc.asymmetric_filters(c.orientations)
    _check(c.name + "/asymmetric", _metamer(c, f).cpu().numpy(), mc.restate(c, filters=f), mc.allowance(i),
           (float(z[f"ref_max_abs_{i}"]), float(z[f"ref_rel_l2_{i}"])))
    ref = (float(z[f"ref_rt_max_abs_{i}"]), float(z[f"ref_rt_rel_l2_{i}"]))
    got = pyramid_roundtrip(torch.tensor(c.tgt, device=DEV), c.levels, c.orientations, filters=f, image_colorspace=c.colorspace)
    _check(c.name + "/asymmetric/roundtrip", got.cpu().numpy(), mc.restate_roundtrip(c, filters=f), (mc.FACTOR * ref[0], mc.FACTOR * ref[1]), ref)


@pytest.mark.parametrize("i", [1, 5])
def test_same_bits_on_two_runs(i):
    c = mc.case(i)
    assert torch.equal(_metamer(c), _metamer(c))


def test_noise_none_is_the_seeded_draw():
    c = mc.case(0)
    tgt = torch.tensor(c.tgt, device=DEV)
    fn = _fn(c)
    got = fn.gen_metamer(tgt, list(c.gaze))
    torch.manual_seed(0)
    noise = torch.rand_like(tgt)
    assert torch.equal(got, fn.gen_metamer(tgt, list(c.gaze), noise=noise))
    assert not torch.equal(got, fn.gen_metamer(tgt, list(c.gaze), noise=torch.rand_like(tgt)))


@pytest.mark.parametrize("i", [0, 1, 5])
@pytest.mark.parametrize("loss_type", ["L1", "MSE"])
def test_loss_and_gradient_match_torch_in_float64(i, loss_type):
    """against torch.nn.L1Loss / MSELoss on the same two pictures in float64. The kernel adds the float64 differences of the float32
    pictures in double (n eps64 at the most) and rounds the mean once to float32 (eps32 / 2): 1 eps32 relative is allowed. A
    gradient element is sign / n or 2 d / n rounded to float32, then multiplied by the float32 upstream scalar: two roundings,
    2 eps32 relative allowed. The L1 pictures hold no element equal to the metamer's (the sign at 0 is a convention)."""
    c = mc.case(i)
    fn = _fn(c, loss_type=loss_type)
    tgt = torch.tensor(c.tgt, device=DEV)
    metamer = fn.gen_metamer(tgt, list(c.gaze))
    rng = np.random.default_rng(100 + i)
    off = rng.uniform(0.01, 0.1, metamer.shape) * rng.choice([-1.0, 1.0], metamer.shape)
    img = (metamer.cpu() + torch.tensor(off, dtype=torch.float32)).to(DEV).requires_grad_(True)
    assert not bool((img.detach() == metamer).any())
    upstream = 3.0
    loss = fn(img, tgt, gaze=list(c.gaze))
    (loss * upstream).backward()
    assert loss.dim() == 0 and loss.device.type == "cuda" and img.grad.shape == img.shape
    x64 = img.detach().double().cpu().requires_grad_(True)
    want = (torch.nn.L1Loss() if loss_type == "L1" else torch.nn.MSELoss())(x64, metamer.double().cpu())
    (want * upstream).backward()
    n = x64.numel()
    rel = abs(float(loss) - float(want)) / float(want)
    g, gw = img.grad.double().cpu().numpy(), x64.grad.numpy()
    grel = float((np.abs(g - gw) / np.abs(gw)).max())
    parity_report.record("metamer", f"{c.name}/{loss_type}/loss", rel_loss=rel, grad_max_rel=grel, n=n)
    print(f"{c.name} {loss_type}: loss rel {rel:.3e} (allowed {EPS32 / 2 + n * EPS64:.3e} < {EPS32:.3e}) gradient max rel {grel:.3e} (allowed {2 * EPS32:.3e})")
    assert rel <= EPS32
    assert grel <= 2 * EPS32


def test_the_metamer_is_kept_for_the_same_target_and_gaze_only(monkeypatch):
    c = mc.case(2)   # (M0's LOD is 0 everywhere: its metamer does not depend on the gaze)
    fn = _fn(c)
    made = []
    gen = fn.gen_metamer
    monkeypatch.setattr(fn, "gen_metamer", lambda *a, **k: made.append(1) or gen(*a, **k))
    tgt = torch.tensor(c.tgt, device=DEV)
    img = torch.tensor(c.img, device=DEV)
    a = fn(img, tgt, gaze=[0.5, 0.5])
    b = fn(img, tgt, gaze=[0.5, 0.5])
    assert len(made) == 1 and torch.equal(a, b)              # kept
    tgt.mul_(0.5)                                            # the same object, written in place: _version moved
    d = fn(img, tgt, gaze=[0.5, 0.5])
    assert len(made) == 2 and not torch.equal(a, d)
    e = fn(img, tgt, gaze=[0.1, 0.9])                        # the reference would keep the metamer of the old gaze
    assert len(made) == 3 and not torch.equal(d, e)
    fn(img, tgt, gaze=[0.1, 0.9])
    assert len(made) == 3
    fn(img, tgt.clone(), gaze=[0.1, 0.9])                    # an equal picture in another tensor: not provably the same
    assert len(made) == 4
    fresh = _fn(c)(img, tgt, gaze=[0.1, 0.9])
    assert torch.equal(e, fresh)                             # the regenerated metamer is the one a new object makes
