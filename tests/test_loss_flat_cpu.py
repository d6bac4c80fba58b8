"""The yardsticks of tests/loss_cases.py without a GPU: the fixture's CRCs, the float32 family's distances from float64 measured again
on every run (printed, and recorded in the parity report as kind "loss"), and the proof that four times those distances is still
narrow enough to see a subtly wrong kernel: the float64 restatement with ONE thing doctored at a time must leave the allowance of at
least one statistic on at least one case by a factor >= 2. The last test records why this file exists: the same wrong stabiliser
passes tests/test_loss.py's white-noise comparison."""
import math
import os

import numpy as np
import torch

from oracle import loss_oracle as lo
from tests import loss_cases as lc
from tests import parity_report


def test_the_family_is_measured_and_every_yardstick_is_finite_and_positive():
    z = lc.golden()
    assert os.path.getsize(os.path.join(lc.GOLDEN, "ref_loss3.npz")) < 600 * 1000
    assert not any(k.startswith(("a_", "b_", "x_", "y_")) for k in z), "the fixture holds recorded results, no pictures"
    for name in lc.NAMES:
        c = lc.case(name)
        x, y = lc.pictures(name)
        assert c["crc"] == int(z[f"crc_{name}"]) == lc.crc_of(x, y)
        assert z[f"grad_{name}"].shape == z[f"ssim_grad_{name}"].shape == x.shape and z[f"grad_{name}"].dtype == np.float32
        print(f"{name}: float64 l1 {c['l164']!r} ssim {c['ssim64']!r} loss {c['loss64']!r}; x == y on {float((x == y).mean()):.3f} of the pixels")
        for stat, yard in c["yardstick"].items():
            per = {m: s[stat] for m, s in c["members"].items()}
            print(f"  {stat:15s} yardstick {yard:.3e} allowance {c['allowance'][stat]:.3e}  members " + " ".join(f"{m} {v:.3e}" for m, v in per.items()))
            parity_report.record("loss", f"family/{name}/{stat}", yardstick=yard, allowance=c["allowance"][stat], **{"member_" + m: v for m, v in per.items()})
            assert set(per) == {"a", "b", "c", "d"} and all(math.isfinite(v) for v in per.values())
            if stat == "l1":  # derived, not measured: the family must itself be inside it
                assert 0 <= yard <= c["allowance"]["l1"] and c["allowance"]["l1"] == lc.L1_EPS * lc.EPS32 * c["l164"] > 0
            else:
                assert 0 < yard < 1e-2 and c["allowance"][stat] == lc.MARGIN * yard
        want = {"grad_loss_nmax", "grad_ssim_nmax"} if c["equal"] else \
            {"l1", "ssim", "loss", "grad_loss_max", "grad_loss_l2", "grad_ssim_max", "grad_ssim_l2"} | ({"grad_gt_max", "grad_gt_l2"} if name in lc.GT_GRAD else set())
        assert set(c["yardstick"]) == want
    c = lc.case("equal")
    assert c["l164"] == 0 and abs(c["ssim64"] - 1) < 1e-15 and float(c["grad_ssim64"].abs().max()) * c["n"] < 1e-10
    assert lc.MARGIN == 4


def test_the_cases_are_the_pictures_the_suite_did_not_have():
    x, y = lc.pictures("blob")
    assert 0.55 < float(((x == 0) & (y == 0)).mean()) < 0.65 and x.shape == (3, 70, 50) and float(x.max()) > 0.8
    x, y = lc.pictures("flat")
    assert (y[0] == 0).all() and (y[1] == 1).all() and (y[2] == 0.5).all() and (x[:, :35] == y[:, :35]).all() and (x[1:, 35:] != y[1:, 35:]).mean() > 0.4
    x, y = lc.pictures("steps")
    assert x[0, 0, 15] != x[0, 0, 16] and x[0, 31, 0] != x[0, 32, 0] and x[1, 0, 36] != x[1, 0, 37] and (x != y).all()
    x, y = lc.pictures("dark")
    assert float(x.max()) <= 0.02 and float(y.max()) < 0.04
    x, y = lc.pictures("tiny")
    assert x.shape == (3, 4, 4) and int((x == y).sum()) == 1
    x, y = lc.pictures("corner")
    assert x.shape == (1, 33, 17)
    x, y = lc.pictures("equal")
    assert (x == y).all() and len(np.unique(x[:, :, :25])) == 3 and len(np.unique(x[:, :, 25:])) > 1000


def test_the_float64_restatement_is_the_oracle():
    """restated() in float64, taps row-major ascending, is oracle/loss_oracle.py's own sum: the doctored variants below differ from the
    reference point by their doctoring alone."""
    for name in ("blob", "steps", "tiny"):
        c = lc.case(name)
        r = lc.restated(c["x"], c["y"], torch.float64, with_gt=name in lc.GT_GRAD)
        assert abs(r["ssim"] - c["ssim64"]) < 1e-14 and abs(r["loss"] - c["loss64"]) < 1e-14 and r["l1"] == c["l164"]
        assert float((r["grad_loss"] - c["grad_loss64"]).abs().max()) < 1e-15 and float((r["grad_ssim"] - c["grad_ssim64"]).abs().max()) < 1e-15
        if name in lc.GT_GRAD:
            assert float((r["grad_gt"] - c["grad_gt64"]).abs().max()) < 1e-15
        g = _analytic_ssim_grad(c["x"], c["y"])
        # another way to the same derivative: float64's own cancellation on flat ground separates the two by ~1e-13 of the scale
        assert float((g - c["grad_ssim64"]).abs().max()) < 1e-10 * float(c["grad_ssim64"].abs().max())


def _analytic_ssim_grad(x, y, drop_m2_term=False):
    """d mean(ssim map) / dx in float64 the way csrc/loss.hip forms it: three derivative maps (mu, sigma as functions of x:
    d map / d x(q) = w(p - q) [A(p) + 2 x(q) B(p) + y(q) C(p)]) and one more blur. drop_m2_term: map A without - m2 df_ds12."""
    x, y = x.double(), y.double()
    w2d, o = lc.window_2d(torch.float64), lc.ORDERS["rows_up"]
    m1, m2 = lc.blur(x, w2d, o), lc.blur(y, w2d, o)
    s1, s2, s12 = lc.blur(x * x, w2d, o) - m1 * m1, lc.blur(y * y, w2d, o) - m2 * m2, lc.blur(x * y, w2d, o) - m1 * m2
    a1, a2, b1, b2 = 2 * m1 * m2 + lc.C1, 2 * s12 + lc.C2, m1 * m1 + m2 * m2 + lc.C1, s1 + s2 + lc.C2
    ssim = a1 * a2 / (b1 * b2)
    df_dmu1, df_ds1, df_ds12 = 2 * m2 * a2 / (b1 * b2) - ssim * 2 * m1 / b1, -ssim / b2, 2 * a1 / (b1 * b2)
    A = df_dmu1 - 2 * m1 * df_ds1 - (0 if drop_m2_term else m2 * df_ds12)
    return (lc.blur(A, w2d, o) + 2 * x * lc.blur(df_ds1, w2d, o) + y * lc.blur(df_ds12, w2d, o)) / x.numel()


def _doctored(variant, c):
    """-> what statistics() takes: the float64 losses of case c with one thing wrong"""
    x, y = c["x"], c["y"]
    if variant == "C1 doubled":
        return lc.restated(x, y, torch.float64, with_gt=c["grad_gt64"] is not None, c1=2 * lc.C1)
    if variant == "C2 x 1.01":
        return lc.restated(x, y, torch.float64, with_gt=c["grad_gt64"] is not None, c2=1.01 * lc.C2)
    if variant == "edge-replicated padding":
        return lc.restated(x, y, torch.float64, with_gt=c["grad_gt64"] is not None, pad="replicate")
    if variant == "map A without - m2 df_ds12":
        g = _analytic_ssim_grad(x, y, drop_m2_term=True)
        return dict(grad_ssim=g, grad_loss=c["grad_loss64"] - lc.LAM * (g - c["grad_ssim64"]))  # loss = .. + lam (1 - ssim)
    if variant == "sign(0) = +1":
        return dict(grad_loss=c["grad_loss64"] + (1.0 - lc.LAM) / c["n"] * (x == y).double())
    raise KeyError(variant)


VARIANTS = ("C1 doubled", "C2 x 1.01", "edge-replicated padding", "map A without - m2 df_ds12", "sign(0) = +1")


def test_every_doctored_variant_leaves_an_allowance_by_a_factor_of_two():
    for variant in VARIANTS:
        worst = (0.0, None, None)
        with parity_report.muted():
            for name in lc.NAMES:
                c = lc.case(name)
                f = lc.ratios(c, lc.statistics(c, _doctored(variant, c)))
                parity_report.record("loss", f"doctored/{variant}/{name}", **f)
                print(f"{variant} / {name}: measured / allowance " + " ".join(f"{k} {v:.3g}" for k, v in f.items()))
                k = max(f, key=f.get)
                if f[k] > worst[0]:
                    worst = (f[k], name, k)
        print(f"{variant}: {worst[0]:.3g} times the allowance of {worst[2]} on {worst[1]}")
        assert worst[0] >= 2.0, (variant, worst)


def test_a_doubled_c1_passes_the_white_noise_comparison_of_test_loss():
    """Why the cases above exist: on tests/test_loss.py's (3, 17, 33) noise pair a kernel with C1 doubled stays inside that file's
    tolerances (3e-6 on the value; rtol 2e-4, atol 2e-7 + 1e-5 / n on the gradient), for every lam it uses."""
    shape = (3, 17, 33)
    g = torch.Generator().manual_seed(sum(shape))
    a = torch.rand(shape, generator=g)
    b = (a + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    x = a.double().requires_grad_(True)
    ss_bad = lc.ssim_restated(x, b.double(), c1=2 * lc.C1)
    gs_bad, ss_bad = torch.autograd.grad(ss_bad, x)[0], ss_bad.item()
    ss, gs = lo.ssim_with_grad(a, b)
    for lam in (0.2, 0.0, 1.0):
        want_loss, _, _, want_grad = lo.l1_ssim(a, b, lam)
        bad_loss = want_loss - lam * (ss_bad - ss)
        bad_grad = want_grad - lam * (gs_bad - gs)
        print(f"lam {lam}: C1 doubled moves the loss by {abs(bad_loss - want_loss):.3e} and the gradient by at most "
              f"{float(((bad_grad - want_grad).abs() / want_grad.abs().max()).max()):.3e} of its largest element")
        assert abs(bad_loss - want_loss) < 3e-6
        np.testing.assert_allclose(bad_grad.numpy(), want_grad.numpy(), atol=2e-7 + 1e-5 / a.numel(), rtol=2e-4)
    assert float((gs_bad - gs).abs().max()) > 0  # the doctoring did reach the gradient
