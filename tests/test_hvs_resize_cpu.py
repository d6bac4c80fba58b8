"""The resized HVS loss (MetamericLossUniform(..., resize=...)) without a GPU: what the fixture tests/golden/ref_hvs_resize.npz
holds (R0 .. R4, tests/hvs_resize_cases.CASES) and that its pictures keep both kinks away ON THE RESIZED PICTURES, the yardstick
(float64 F.interpolate, then tests/hvs_ref.hvs_loss) against the reference's own float32 vectors, pyramid_size against the
scripts' formula, the argument checks of resize=, and the three new entry points of the C ABI."""
import math
import os
import re

import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native
from fov3dgs_amd.odak_perception import MetamericLossUniform, _native_hvs, pyramid_size
from tests import hvs_cases as hc
from tests import hvs_ref, parity_report
from tests import hvs_resize_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = len(rc.CASES)
SPACES = [(i, cs) for i, c in enumerate(rc.CASES) for cs in c[-1]]


def test_fixture_holds_the_five_cases():
    z = rc.fixture()
    assert int(z["n"]) == N == 5
    for i, ((Hs, Ws), (H, W), levels, no, pool, kind, asym, spaces) in enumerate(rc.CASES):
        c = rc.case(i)
        assert (c.Hs, c.Ws, c.H, c.W, c.levels, c.orientations, c.pooling, c.loss_type, c.asymmetric, c.spaces) == \
            (Hs, Ws, H, W, levels, no, pool, kind, asym, spaces)
        assert (c.H, c.W) == pyramid_size(Hs, Ws, levels) or i in (3, 4)  # R3 and R4 grow by more than the next multiple
        assert c.H % 2 ** levels == 0 and c.W % 2 ** levels == 0 and c.H >= Hs and c.W >= Ws
        assert z[f"img_{i}"].dtype == np.uint16 == z[f"tgt_{i}"].dtype and z[f"grad_{i}"].dtype == np.float32
        assert z[f"grad_{i}"].shape == (1, 3, Hs, Ws) == z[f"img_{i}"].shape == z[f"tgt_{i}"].shape  # the SOURCE shape
        assert f"seed_{i}" in z
    assert z["grad_2_ycrcb"].shape == z["grad_2"].shape and not np.array_equal(z["grad_2_ycrcb"], z["grad_2"])
    # data only: pictures, vectors, case parameters; and smaller than the second fixture
    assert all(v.dtype.kind in "fiu" for v in z.values())
    assert os.path.getsize(os.path.join(hc.GOLDEN, "ref_hvs_resize.npz")) < os.path.getsize(os.path.join(hc.GOLDEN, "ref_hvs_edges.npz"))


def test_two_orientations_take_the_first_bands_of_the_stored_set_of_four():
    f2, f4 = rc.filters_of(rc.case(0)), hvs_ref.filters_from_npz(hc.edges(), 4, prefix="afilters")
    assert len(f2["b"]) == 2 and torch.equal(f2["l0"], f4["l0"]) and torch.equal(f2["h0"], f4["h0"])
    assert all(torch.equal(a, b) for a, b in zip(f2["b"], f4["b"]))
    assert all(hc.asymmetry(b.numpy()) >= hc.ASYMMETRY for b in [f2["l0"], f2["h0"]] + f2["b"])
    assert len(rc.filters_of(rc.case(4))["b"]) == 1 and len(rc.filters_of(rc.case(2))["b"]) == 4
    assert hc.asymmetry(rc.filters_of(rc.case(3))["l0"].numpy()) == 0.0  # R3: the reference's own filters


@pytest.mark.parametrize("i,colorspace", SPACES)
def test_resized_inputs_keep_both_kinks_away(i, colorspace):
    c = rc.case(i)
    f = hvs_ref.filters_to(rc.filters_of(c), dtype=torch.float64)
    img = rc.resize(torch.tensor(c.img, dtype=torch.float64), c.H, c.W)
    tgt = rc.resize(torch.tensor(c.tgt, dtype=torch.float64), c.H, c.W)
    assert img.shape == (1, 3, c.H, c.W)
    assert hvs_ref.variances_outside_band(img, tgt, f, c.pooling, c.levels, image_colorspace=colorspace) == 0
    if c.loss_type == "L1":
        n, share = hvs_ref.undecided_sign_gradient(img, tgt, f, c.pooling, c.levels, image_colorspace=colorspace)
        print(f"R{i} {colorspace}: {n} statistics differ by less than {hvs_ref.UNDECIDED}, share of the largest gradient {share:.3e}")
        assert share <= 2e-7  # (the generator's KINK_SHARE)
    assert hc.distances(rc.reference(i, colorspace)[1], rc.yardstick(i, colorspace)["grad"])[0] < 2e-5  # (the generator's REF_L2)


@pytest.mark.parametrize("i,colorspace", SPACES)
def test_yardstick_matches_the_reference_vectors(i, colorspace):
    """float64 resize + restatement vs the reference's float32 run through F.interpolate and its own MetamericLossUniform:
    test_hvs_cpu.py's bound for the reference's distance from float64"""
    y = rc.yardstick(i, colorspace)
    ref_loss, ref_grad = rc.reference(i, colorspace)
    rel_loss = abs(ref_loss - y["loss"]) / y["loss"]
    l2, mx = hc.distances(ref_grad, y["grad"])
    parity_report.record("hvs", f"reference_vs_float64/R{i}/{colorspace}", rel_loss=rel_loss, grad_rel_l2=l2, grad_max_over_max=mx)
    print(f"R{i} {colorspace}: reference fp32 vs float64: rel loss {rel_loss:.3e} grad rel L2 {l2:.3e} max/max {mx:.3e}")
    assert y["grad"].shape == ref_grad.shape == (1, 3, rc.case(i).Hs, rc.case(i).Ws)
    assert rel_loss < 1e-4 and l2 < 1e-4 and mx < 1e-4


@pytest.mark.parametrize("size,levels,want", [((1080, 1920), 5, (1088, 1920)), ((1080, 1920), 6, (1088, 1920)), ((135, 16), 3, (136, 16)),
                                              ((21, 30), 3, (24, 32)), ((64, 64), 5, (64, 64)), ((1, 5), 2, (4, 8)),
                                              ((1081, 1921), 5, (1088, 1952)), ((720, 1280), 5, (736, 1280))])
def test_pyramid_size_is_the_scripts_formula(size, levels, want):
    h, w = size
    d = 2 ** levels
    assert pyramid_size(h, w, levels) == (math.ceil(h / d) * d, math.ceil(w / d) * d) == want
    assert all(isinstance(v, int) for v in pyramid_size(h, w, levels))


def test_resize_argument_checks_name_what_is_wrong():
    fn = MetamericLossUniform(device="cuda", pooling_size=4, n_pyramid_levels=3, n_orientations=6, loss_type="L1",
                              bilinear_downsampling=True, filters=hc.filters(6))
    x = torch.rand(1, 3, 21, 30)
    with pytest.raises(ValueError, match="shrinking"):
        fn(x, x.clone(), resize=(16, 32))
    with pytest.raises(ValueError, match="shrinking"):
        fn(x, x.clone(), resize=(24, 24))
    with pytest.raises(ValueError, match="no multiple of 2 \\*\\* n_pyramid_levels"):
        fn(x, x.clone(), resize=(24, 36))
    for bad in ("pyramids", (24,), (24, 32, 3), (24.0, 32), 24, (0, 32), (True, 32)):
        with pytest.raises(ValueError, match="malformed"):
            fn(x, x.clone(), resize=bad)
    # without resize=, and with a resize to the pictures' own size, the call is the one it was: its own error for a size that
    # is no multiple
    for kw in ({}, {"resize": None}, {"resize": (21, 30)}):
        with pytest.raises(ValueError, match="Multiplies of 2"):
            fn(x, x.clone(), **kw)
    # a well-formed resize gets as far as the plain call does on the CPU
    for r in ("pyramid", (24, 32), [48, 32]):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, x.clone(), resize=r)
    with pytest.raises(ValueError, match="differ"):
        fn(x, torch.rand(1, 3, 24, 32), resize="pyramid")


def test_resized_abi_names_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fovraster.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fr_[a-z_0-9A-Z]+)\s*\(", txt))
    lib = _native.load()
    for n in ("fr_hvs_forward_resized", "fr_hvs_backward_resized", "fr_hvs_resized_backward_floats"):
        assert n in declared and n in _native.EXPORTS and hasattr(lib, n), n
        assert getattr(lib, n).argtypes is not None, n
    assert len(lib.fr_hvs_forward_resized.argtypes) == len(lib.fr_hvs_forward.argtypes) + 2
    assert len(lib.fr_hvs_backward_resized.argtypes) == len(lib.fr_hvs_backward.argtypes) + 2
    assert lib.fr_abi_version() == 12 == _native.ABI_VERSION


def test_resized_backward_workspace_and_refusals_on_the_host():
    lib = _native.load()
    plain = lib.fr_hvs_workspace_floats(1088, 1920, 9.0, 5, 6, 1)
    assert plain > 0
    assert lib.fr_hvs_resized_backward_floats(1080, 1920, 1088, 1920, 9.0, 5, 6) == plain + 3 * 1088 * 1920
    assert lib.fr_hvs_resized_backward_floats(1088, 1920, 1088, 1920, 9.0, 5, 6) == plain  # nothing to resize
    for c in (rc.case(i) for i in range(N)):
        st = _native_hvs.Settings(c.H, c.W, float(c.pooling), c.levels, c.orientations, 0, 1, c.Hs, c.Ws)
        assert _native_hvs.backward_floats(st) == _native_hvs.floats(st, 1) + 3 * c.H * c.W >= _native_hvs.floats(st, 1)
        _native_hvs.layout(st)  # the forward state is the H x W call's
    assert lib.fr_hvs_resized_backward_floats(1088, 1920, 1080, 1920, 9.0, 5, 6) == -1
    assert "shrinking" in _native.last_error()
    assert lib.fr_hvs_resized_backward_floats(64, 72, 64, 64, 9.0, 5, 6) == -1 and "shrinking" in _native.last_error()
    assert lib.fr_hvs_resized_backward_floats(0, 16, 32, 32, 4.0, 5, 6) == -1 and "positive" in _native.last_error()
    assert lib.fr_hvs_resized_backward_floats(30, 30, 40, 64, 4.0, 5, 6) == -1 and "multiple of 2" in _native.last_error()
    with pytest.raises(ValueError, match="shrinking"):
        _native_hvs.backward_floats(_native_hvs.Settings(32, 32, 4.0, 5, 6, 0, 1, 33, 32))
    # the launching calls refuse the same before they touch a pointer
    assert lib.fr_hvs_forward_resized(1088, 1920, 1080, 1920, 9.0, 5, 6, 0, 1, None, None, None, None, None, None, None, None) == -1
    assert "shrinking" in _native.last_error()
    assert lib.fr_hvs_backward_resized(1088, 1920, 1080, 1920, 9.0, 5, 6, 0, 1, None, None, None, None, None, None, None) == -1
    assert "shrinking" in _native.last_error()
    assert lib.fr_hvs_forward_resized(21, 30, 24, 32, 5.0, 3, 4, 0, 1, None, None, None, None, None, None, None, None) == -1
    assert "null" in _native.last_error()
