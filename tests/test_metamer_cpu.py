"""The metamer without a GPU: the float64 restatement (tests/metamer_ref.py) pinned to the reference's own vectors
(tests/golden/ref_metamer*.npz, from make_metamer_golden.py), what a synthesis that forgets a piece would cost, the C ABI's refusals
(made before anything is enqueued, so they need no device), the workspace query and the Python layer's refusals.

The dropped piece, measured on the restatement (test_a_dropped_piece_moves_the_metamer_beyond_the_allowance prints every figure):
leaving one oriented band of one level, or the highpass term, out of the synthesis moves the metamer by at least 193 times the
allowance of its case in max |d| (M1, the last band of level 1; the highpass term: at least 3.7e3 times) and at least 3.4e3 times
in relative L2, the smallest factors over all cases and levels. DROP_FACTOR below asserts 100 times in both measures."""
import sys

import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native
from fov3dgs_amd import odak_perception as op
from fov3dgs_amd.odak_perception import _native_hvs_fov
from tests import hvs_cases as hc
from tests import metamer_cases as mc
from tests import metamer_ref

CASES = list(range(6))
EPS32 = float(np.finfo(np.float32).eps)
# The stored distance is |float32 vector - float64 restatement|; recomputed here it can differ from the stored one only by the
# restatement's own float64 rounding (1e-16 absolute on a distance of 1e-7 .. 1e-4), should another build sum a convolution in
# another order: 1e-9 of the distance is a thousand times that and a millionth of what the allowance is made of.
SAME = 1e-9
DROP_FACTOR = 100.0


def test_the_fixture_holds_the_cases():
    assert mc.n_cases() == len(CASES) == len(mc.NAMES)
    c = mc.case(0)
    assert (c.H, c.W, c.levels, c.orientations) == (32, 64, 5, 2)
    c = mc.case(1)
    assert (c.H, c.W, c.levels, c.orientations, c.mode, c.gaze) == (40, 56, 3, 6, "linear", (0.2, 0.7))
    c = mc.case(4)
    assert (c.levels, c.gaze, c.colorspace) == (4, (1.2, -0.1), "YCrCb")
    assert (mc.case(5).H, mc.case(5).W) == (96, 160)


@pytest.mark.parametrize("i", CASES)
def test_reference_metamer_lies_at_the_stored_distance_from_the_restatement(i):
    z, y = mc.golden(), mc.yardstick(i)
    assert y.shape == z[f"metamer_{i}"].shape == (1, 3, mc.case(i).H, mc.case(i).W)
    mx, l2 = mc.distances(z[f"metamer_{i}"], y)
    print(f"{mc.NAMES[i]}: reference float32 vs restatement: max |d| {mx:.3e} rel L2 {l2:.3e}")
    assert mx == pytest.approx(float(z[f"ref_max_abs_{i}"]), rel=SAME) and l2 == pytest.approx(float(z[f"ref_rel_l2_{i}"]), rel=SAME)
    assert 0 < l2 < 1e-5   # a float32 run of the same computation, not another computation
    assert y.min() < 0 and y.max() > 1   # the metamer leaves [0, 1]: nothing clamps it


@pytest.mark.parametrize("i", CASES)
def test_reference_roundtrip_lies_at_the_stored_distance_from_the_restatement(i):
    z, y = mc.golden(), mc.yardstick_roundtrip(i)
    mx, l2 = mc.distances(z[f"roundtrip_{i}"], y)
    print(f"{mc.NAMES[i]}: reference float32 round trip vs restatement: max |d| {mx:.3e} rel L2 {l2:.3e}")
    assert mx == pytest.approx(float(z[f"ref_rt_max_abs_{i}"]), rel=SAME) and l2 == pytest.approx(float(z[f"ref_rt_rel_l2_{i}"]), rel=SAME)
    assert 0 < l2 < 1e-6


@pytest.mark.parametrize("i", CASES)
def test_reference_loss_and_gradient_are_the_restatements(i):
    """the loss within the float32 rounding of its mean (16 eps), plus what the metamer's own float32 distance moves it by; the
    gradient elementwise wherever the sign of image - metamer is decided beyond that distance"""
    c, z, y = mc.case(i), mc.golden(), mc.yardstick(i)
    x = torch.tensor(c.img, dtype=torch.float64, requires_grad=True)
    loss = metamer_ref.loss(x, torch.tensor(y), c.loss_type)
    loss.backward()
    d = float(z[f"ref_max_abs_{i}"])
    moved = d if c.loss_type == "L1" else 2 * d * float(np.abs(c.img - y).max())
    assert abs(float(z[f"loss_{i}"]) - float(loss)) <= 16 * EPS32 * float(loss) + moved
    decided = np.abs(c.img.astype(np.float64) - y) > 2 * d
    assert decided.mean() > 0.999
    g, want = z[f"grad_{i}"].astype(np.float64), x.grad.numpy()
    tol = 4 * EPS32 * np.abs(want) + (0 if c.loss_type == "L1" else 2 * d / want.size)
    assert (np.abs(g - want) <= tol)[decided].all()


def test_m3_is_the_round_trip_plus_noise_on_the_variance_floor():
    """alpha 0.001: LOD 0 everywhere, so the blended mean is the band itself and the variance sits on its floor: each matched band is
    the target's band plus the normalised noise band times sqrt(1e-7), and the synthesis is linear"""
    y, rt = mc.yardstick(3), mc.yardstick_roundtrip(3)
    assert np.abs(y - rt).max() < 40 * np.sqrt(1e-7)   # (a normalised band reaches a few sigma; the synthesis adds up to 10 of them)
    assert np.abs(y - rt).max() > np.sqrt(1e-7)


@pytest.mark.parametrize("i", CASES)
def test_a_dropped_piece_moves_the_metamer_beyond_the_allowance(i):
    c, y = mc.case(i), mc.yardstick(i)
    amx, al2 = mc.allowance(i)
    for drop in ["h"] + [(l, c.orientations - 1) for l in range(c.levels - 1)]:
        mx, l2 = mc.distances(mc.restate(c, drop=drop), y)
        print(f"{c.name}: without {drop}: max |d| {mx:.3e} = {mx / amx:.3g} x allowance, rel L2 {l2:.3e} = {l2 / al2:.3g} x allowance")
        assert mx > DROP_FACTOR * amx and l2 > DROP_FACTOR * al2, (drop, mx / amx, l2 / al2)


def test_asymmetric_filters_tell_a_flipped_or_transposed_kernel():
    """the set the GPU test runs with: every block differs from each of its mirror images, and a synthesis that flips or
    transposes its taps lands far outside the allowance"""
    c = mc.case(0)
    f = mc.asymmetric_filters(c.orientations)
    for name, block in [("l0", f["l0"]), ("h0", f["h0"])] + [(f"b{i}", b) for i, b in enumerate(f["b"])]:
        assert hc.asymmetry(block.numpy()) > 0.05, name
    y = mc.restate(c, filters=f)
    amx, _ = mc.allowance(0)
    for what, wrong in (("flipped", lambda t: torch.flip(t, (-2, -1))), ("transposed", lambda t: t.transpose(-2, -1).contiguous())):
        g = {"l0": f["l0"], "h0": f["h0"], "b": f["b"]}
        synth = {"l0": wrong(f["l0"]), "h0": wrong(f["h0"]), "b": [wrong(b) for b in f["b"]]}
        # analysis with the right set, synthesis with the wrong one
        with torch.no_grad():
            x = torch.tensor(c.tgt, dtype=torch.float64)
            from tests import hvs_ref
            h, bands, low = hvs_ref.pyramid(hvs_ref.rgb_2_ycrcb(x), hvs_ref.filters_to(g, dtype=torch.float64), c.levels)
            bad = metamer_ref.ycrcb_2_rgb(metamer_ref.reconstruct(h, bands, low, hvs_ref.filters_to(synth, dtype=torch.float64))).numpy()
        good = mc.restate_roundtrip(c, filters=f)
        assert np.abs(bad - good).max() > 1000 * amx, what
    assert np.isfinite(y).all()


# ---------------------------------------------------------------- the C ABI
A = 0x10000  # an aligned address that is never dereferenced: every call below is refused before anything is enqueued


def _metamer(H=32, W=64, alpha=0.2, width=0.2, dist=0.7, mode=1, gx=0.5, gy=0.5, levels=5, no=2, rgb=1, filters=A, target=A, noise=A,
             work=A, out=A):
    rc = _native.load().fr_hvs_metamer(H, W, alpha, width, dist, mode, gx, gy, levels, no, rgb, filters, target, noise, work, out, None)
    return rc, _native.last_error()


@pytest.mark.parametrize("kw, word", [
    (dict(H=30), "size 30x64"), (dict(W=65), "size 32x65"), (dict(levels=1), "n_pyramid_levels 1"), (dict(levels=7, H=128, W=128), "n_pyramid_levels 7"),
    (dict(no=0), "0 orientations"), (dict(no=9), "9 orientations"), (dict(H=64, W=32), "mip chain"), (dict(alpha=-1.0), "alpha"),
    (dict(alpha=float("nan")), "alpha"), (dict(width=0.0), "real_image_width"), (dict(dist=float("inf")), "real_viewing_distance"),
    (dict(gx=float("nan")), "gaze"), (dict(mode=2), "mode"), (dict(rgb=2), "rgb"), (dict(filters=None), "filters"),
    (dict(target=None), "target"), (dict(noise=None), "noise"), (dict(work=None), "workspace"), (dict(out=None), "out is null"),
    (dict(work=A + 4), "workspace must be 8-byte aligned"), (dict(noise=A + 2), "noise must be 4-byte aligned")])
def test_fr_hvs_metamer_refuses_by_field_name(kw, word):
    rc, msg = _metamer(**kw)
    assert rc != 0 and msg.startswith("hvs_metamer:") and word in msg, msg


def test_roundtrip_and_loss_calls_refuse_by_field_name():
    lib = _native.load()
    for args, word in [((30, 64, 5, 2, 1, A, A, A, A, None), "size 30x64"), ((32, 64, 5, 2, 3, A, A, A, A, None), "rgb"),
                       ((32, 64, 5, 2, 1, None, A, A, A, None), "filters"), ((32, 64, 5, 2, 1, A, None, A, A, None), "image"),
                       ((32, 64, 5, 2, 1, A, A, None, A, None), "workspace"), ((32, 64, 5, 2, 1, A, A, A, None, None), "out")]:
        assert lib.fr_hvs_metamer_roundtrip(*args) != 0 and word in _native.last_error(), _native.last_error()
    for args, word in [((0, 0, A, A, A, A, None), "n must"), ((10, 2, A, A, A, A, None), "mse"), ((10, 0, None, A, A, A, None), "image"),
                       ((10, 0, A, None, A, A, None), "metamer"), ((10, 0, A, A, None, A, None), "workspace"),
                       ((10, 0, A, A, A + 4, A, None), "8-byte"), ((10, 0, A, A, A, None, None), "out")]:
        assert lib.fr_hvs_metamer_loss_forward(*args) != 0 and word in _native.last_error(), _native.last_error()
    for args, word in [((-1, 0, A, A, A, A, None), "n must"), ((10, -1, A, A, A, A, None), "mse"), ((10, 1, None, A, A, A, None), "image"),
                       ((10, 1, A, None, A, A, None), "metamer"), ((10, 1, A, A, A, None, None), "dL_dimage")]:
        assert lib.fr_hvs_metamer_loss_backward(*args) != 0 and word in _native.last_error(), _native.last_error()


@pytest.mark.parametrize("H, W, levels, no", [(32, 64, 5, 2), (40, 56, 3, 6), (96, 160, 5, 2), (1088, 1920, 5, 6)])
def test_workspace_query(H, W, levels, no):
    """the documented layout: the doubles (LOD maps, two scalars per band, the partial sums of one pass over the largest level),
    the target's state as the foveated loss keeps it, the noise's bands and lowpasses, one running image per level"""
    lib = _native.load()
    st = _native_hvs_fov.Settings(H, W, 0.2, 0.2, 0.7, 1, 0.5, 0.5, levels, no, 0, 1)
    state, lod_doubles = _native_hvs_fov.floats(st, 0), _native_hvs_fov.floats(st, 3) // 2
    planes = [(H >> l) * (W >> l) for l in range(levels - 1)]
    nbands = 1 + (levels - 1) * no
    noise = sum((no + (1 if l == 0 else 0)) * 3 * p + 3 * (p // 4) for l, p in enumerate(planes))
    run = sum(3 * p for p in planes)
    doubles = lod_doubles + 2 * nbands + -(-3 * H * W // 1024) * (no + 1)
    assert lib.fr_hvs_metamer_workspace_floats(H, W, levels, no, 0) == 2 * doubles + state + noise + run
    assert lib.fr_hvs_metamer_workspace_floats(H, W, levels, no, 1) == state + run
    assert lib.fr_hvs_metamer_workspace_floats(H + 1, W, levels, no, 0) == -1 and "size" in _native.last_error()
    assert lib.fr_hvs_metamer_workspace_floats(H, W, levels, no, 2) == -1 and "roundtrip" in _native.last_error()
    assert lib.fr_hvs_metamer_loss_workspace_doubles(3 * H * W) == min(-(-3 * H * W // 4096), 4096) + 1
    assert lib.fr_hvs_metamer_loss_workspace_doubles(0) == -1


# ---------------------------------------------------------------- the Python layer
def test_the_references_import_line_works_against_the_package(monkeypatch):
    """eff_finetune.py:39, prune.py:41, metric_mask_learn.py:42, compose_models.py:37, hvs_loss_calc.py:17"""
    monkeypatch.setitem(sys.modules, "odak_perception", op)
    names = {}
    exec("from odak_perception import MetamerMSELoss, MetamericLoss, MetamericLossUniform", names)
    assert names["MetamerMSELoss"] is op.MetamerMSELoss and names["MetamericLoss"] is op.MetamericLoss
    assert {"MetamerMSELoss", "MetamericLoss", "MetamericLossUniform", "pyramid_roundtrip"} <= set(op.__all__)


def _fn(**kw):
    args = dict(device="cpu", avg_pooling_downup=True, filters=hc.filters(2))
    args.update(kw)
    return op.MetamerMSELoss(**args)


def test_the_constructor_keeps_the_references_signature_and_refuses_by_name():
    import inspect
    names = list(inspect.signature(op.MetamerMSELoss.__init__).parameters)[1:]
    assert names == ["device", "alpha", "real_image_width", "real_viewing_distance", "mode", "n_pyramid_levels", "n_orientations", "equi",
                     "loss_type", "avg_pooling_downup", "filters"]
    d = {k: v.default for k, v in inspect.signature(op.MetamerMSELoss.__init__).parameters.items()}
    assert (d["alpha"], d["real_image_width"], d["real_viewing_distance"], d["mode"], d["n_pyramid_levels"], d["n_orientations"], d["equi"],
            d["loss_type"], d["avg_pooling_downup"], d["filters"]) == (0.2, 0.2, 0.7, "quadratic", 5, 2, False, "L1", False, None)
    with pytest.raises(NotImplementedError, match="avg_pooling_downup"):
        op.MetamerMSELoss(filters=hc.filters(2))   # the reference's default
    with pytest.raises(NotImplementedError, match="equi"):
        _fn(equi=True)
    with pytest.raises(ValueError, match="loss_type"):
        _fn(loss_type="L2")
    with pytest.raises(ValueError, match="mode"):
        _fn(mode="cubic")
    with pytest.raises(ValueError, match="n_pyramid_levels"):
        _fn(n_pyramid_levels=7)
    with pytest.raises(ValueError, match="n_orientations"):
        _fn(n_orientations=9, filters=hc.filters(6))
    with pytest.raises(ValueError, match="alpha"):
        _fn(alpha=-0.1)
    fn = _fn()
    assert fn.to("cpu") is fn and fn.device == torch.device("cpu")


def test_the_calls_refuse_by_name():
    fn = _fn()
    x = torch.zeros(1, 3, 32, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn.gen_metamer(x, [0.5, 0.5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.pyramid_roundtrip(x, 5, 2, filters=hc.filters(2))
    with pytest.raises(ValueError, match="Multiplies of 2"):
        fn(torch.zeros(1, 3, 30, 64), torch.zeros(1, 3, 30, 64))
    with pytest.raises(ValueError, match="Multiplies of 2"):
        op.pyramid_roundtrip(torch.zeros(1, 3, 32, 48), 5, 2, filters=hc.filters(2))
    with pytest.raises(ValueError, match="differ"):
        fn(x, torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match="gaze"):
        fn.gen_metamer(x, [0.5])
    with pytest.raises(ValueError, match="gaze"):
        fn(x, x, gaze=[0.5, float("nan")])
    with pytest.raises(NotImplementedError, match="batches"):
        fn.gen_metamer(torch.zeros(2, 3, 32, 64), [0.5, 0.5])
    with pytest.raises(NotImplementedError, match="3-channel"):
        fn.gen_metamer(torch.zeros(1, 1, 32, 64), [0.5, 0.5])
    with pytest.raises(ValueError, match="image_colorspace"):
        fn.gen_metamer(x, [0.5, 0.5], image_colorspace="HSV")
    with pytest.raises(ValueError, match="n_pyramid_levels"):
        op.pyramid_roundtrip(x, 1, 2, filters=hc.filters(2))
    with pytest.raises(TypeError):
        fn.gen_metamer(np.zeros((1, 3, 32, 64)), [0.5, 0.5])


def test_metameric_loss_uniform_gen_metamer_keeps_raising():
    fn = op.MetamericLossUniform(bilinear_downsampling=True, filters=hc.filters(2))
    with pytest.raises(NotImplementedError, match="gen_metamer"):
        fn.gen_metamer(torch.zeros(1, 3, 32, 64))
