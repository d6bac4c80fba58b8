"""The uniform metameric (HVS) loss without a GPU: the float64 restatement (tests/hvs_ref.py) against the reference's own vectors,
the pooling window / size rules against torch, the argument checks of the public class, and the ABI."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native
from fov3dgs_amd.odak_perception import MetamericLossUniform, pack_filters
from fov3dgs_amd.odak_perception import _native_hvs
from tests import hvs_cases as hc
from tests import hvs_ref, parity_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(range(7))


def test_fixture_holds_the_seven_cases():
    assert hc.n_cases() == 7
    want = [(32, 64, 4, 5, 6, "L1"), (64, 96, 9, 5, 6, "L1"), (40, 56, 4, 3, 6, "MSE"), (32, 32, 1, 5, 6, "L1"),
            (64, 64, 16, 5, 6, "MSE"), (96, 160, 25, 5, 6, "L1"), (48, 80, 2, 4, 2, "L1")]
    assert [tuple(hc.case(i)[1:7]) for i in CASES] == want
    for f in ("ref_hvs.npz", "ref_hvs_maps.npz"):
        assert os.path.getsize(os.path.join(hc.GOLDEN, f)) < (1 << 20)


@pytest.mark.parametrize("i", CASES)
def test_restatement_matches_the_reference_vectors(i):
    """float64 restatement vs the reference's float32 run: the difference is the reference's rounding, which also is the
    allowance of the GPU tests (x3): bounded here by 1e-4 relative, far above fp32 rounding of these sums and far below any
    mistake in a window, a weight or a filter."""
    z, y = hc.golden(), hc.yardstick(i)
    rel_loss = abs(float(z[f"loss_{i}"]) - y["loss"]) / y["loss"]
    l2, mx = hc.distances(z[f"grad_{i}"], y["grad"])
    parity_report.record("hvs", f"reference_vs_float64/case{i}", rel_loss=rel_loss, grad_rel_l2=l2, grad_max_over_max=mx)
    print(f"case {i}: reference fp32 vs float64: rel loss {rel_loss:.3e} grad rel L2 {l2:.3e} max/max {mx:.3e}")
    assert rel_loss < 1e-4 and l2 < 1e-4 and mx < 1e-4
    idx = [int(v) for v in z[f"mapidx_{i}"]]
    for name, k in zip(("map0", "mapmid", "mapstd", "maplow"), idx):
        l2m, mxm = hc.distances(z[f"{name}_{i}"], y["maps"][k])
        print(f"   {name} (statistic {k}): rel L2 {l2m:.3e} max/max {mxm:.3e}")
        assert y["maps"][k].shape == z[f"{name}_{i}"].shape
        assert mxm < 1e-4, (name, mxm)


@pytest.mark.parametrize("i", CASES)
def test_inputs_keep_the_clamp_away_from_its_kink(i):
    c = hc.case(i)
    f = hvs_ref.filters_to(hc.filters(c.orientations), dtype=torch.float64)
    n = hvs_ref.variances_outside_band(torch.tensor(c.img, dtype=torch.float64), torch.tensor(c.tgt, dtype=torch.float64), f,
                                       c.pooling, c.levels)
    assert n == 0


@pytest.mark.parametrize("pooling", [9, 4.5, 2.25, 1.125, 4, 2, 1, 0.5, 0.25, 25, 12.5, 16, 0.5625])
@pytest.mark.parametrize("n", [4, 6, 8, 12, 40, 96])
def test_window_and_size_rules_match_interpolate(pooling, n):
    n_out = hvs_ref.pooled_size(n, pooling)
    if n_out < 1:
        return
    x = torch.arange(n * n, dtype=torch.float64).reshape(1, 1, n, n) ** 1.5
    down = F.interpolate(x, scale_factor=1.0 / pooling, mode="area")
    assert down.shape[-1] == n_out == down.shape[-2]
    mine = torch.empty(n_out, n_out, dtype=torch.float64)
    for jy in range(n_out):
        ys, ye = hvs_ref.window(jy, n, n_out)
        for jx in range(n_out):
            xs, xe = hvs_ref.window(jx, n, n_out)
            mine[jy, jx] = x[0, 0, ys:ye, xs:xe].mean()
    assert torch.allclose(mine, down[0, 0], rtol=1e-13, atol=0)
    k = 1.0 / pooling
    if k >= 1 and k == int(k):
        # 1/p an integer: the blur is the identity EXACTLY, in float32 too (the kernels' path without pooling relies on it)
        for dt in (torch.float32, torch.float64):
            xx = torch.rand(1, 3, n, n, dtype=dt, generator=torch.Generator().manual_seed(n))
            assert torch.equal(hvs_ref.uniform_blur(xx, pooling), xx)
            m, s, v = hvs_ref.find_stats(xx, pooling)
            assert torch.equal(v, torch.zeros_like(v)) and torch.equal(s, torch.full_like(s, 1e-7).sqrt())
    elif pooling < 1:
        xx = torch.rand(1, 1, n, n, dtype=torch.float64, generator=torch.Generator().manual_seed(n))
        assert not torch.equal(hvs_ref.uniform_blur(xx, pooling), xx)  # a fractional p below 1 is NOT the identity


def _filters():
    return hc.filters(6)


def test_argument_checks():
    f = _filters()
    with pytest.raises(NotImplementedError, match="bilinear_downsampling"):
        MetamericLossUniform(device="cpu", filters=f, n_orientations=6)
    with pytest.raises(ValueError, match="loss_type"):
        MetamericLossUniform(bilinear_downsampling=True, loss_type="L2", filters=f, n_orientations=6)
    with pytest.raises(ValueError, match="n_pyramid_levels"):
        MetamericLossUniform(bilinear_downsampling=True, n_pyramid_levels=7, filters=f, n_orientations=6)
    with pytest.raises(ValueError, match="pooling_size"):
        MetamericLossUniform(bilinear_downsampling=True, pooling_size=0, filters=f, n_orientations=6)
    with pytest.raises(ValueError, match="holds 2"):
        MetamericLossUniform(bilinear_downsampling=True, n_orientations=6, filters=hc.filters(2))
    bad = dict(f, l0=torch.zeros(1, 1, 9, 9))
    with pytest.raises(ValueError, match="5x5"):
        MetamericLossUniform(bilinear_downsampling=True, n_orientations=6, filters=bad)
    fn = MetamericLossUniform(device="cuda", pooling_size=4, n_pyramid_levels=5, n_orientations=6, loss_type="L1",
                              bilinear_downsampling=True, filters=f)
    x = torch.rand(1, 3, 32, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(x, x.clone())
    with pytest.raises(ValueError, match="Multiplies of 2"):
        fn(torch.rand(1, 3, 40, 64), torch.rand(1, 3, 40, 64))
    with pytest.raises(NotImplementedError, match="batches"):
        fn(torch.rand(2, 3, 32, 64), torch.rand(2, 3, 32, 64))
    with pytest.raises(NotImplementedError, match="1-channel"):
        fn(torch.rand(1, 1, 32, 64), torch.rand(1, 1, 32, 64))
    with pytest.raises(NotImplementedError, match="visualise_loss"):
        fn(x, x.clone(), visualise_loss=True)
    with pytest.raises(ValueError, match="image_colorspace"):
        fn(x, x.clone(), image_colorspace="HSV")
    with pytest.raises(ValueError, match="differ"):
        fn(x, torch.rand(1, 3, 64, 64))
    with pytest.raises(NotImplementedError, match="gen_metamer"):
        fn.gen_metamer(x)


def test_without_filters_the_error_says_to_pass_them(monkeypatch):
    monkeypatch.setattr(sys, "path", [p for p in sys.path if "metamer" not in p])
    for k in [k for k in sys.modules if k == "odak_perception" or k.startswith("odak_perception.")]:
        monkeypatch.delitem(sys.modules, k)
    with pytest.raises(RuntimeError, match="filters="):
        MetamericLossUniform(bilinear_downsampling=True, n_orientations=6)


def test_filters_come_from_the_callers_odak_perception(monkeypatch, tmp_path):
    """filters=None imports odak_perception.steerable_pyramid_filters from the caller's environment"""
    pkg = tmp_path / "odak_perception"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "steerable_pyramid_filters.py").write_text(
        "import torch\n"
        "def get_steerable_pyramid_filters(size, n, kind):\n"
        "    assert (size, kind) == (5, 'cropped')\n"
        "    t = lambda v: torch.full((1, 1, 5, 5), float(v))\n"
        "    return {'l0': t(1), 'h0': t(2), 'b': [t(3 + i) for i in range(n)]}\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    for k in [k for k in sys.modules if k == "odak_perception" or k.startswith("odak_perception.")]:
        monkeypatch.delitem(sys.modules, k)
    fn = MetamericLossUniform(bilinear_downsampling=True, n_orientations=2)
    assert fn._filters_cpu.reshape(4, 25)[:, 0].tolist() == [1.0, 2.0, 3.0, 4.0]


def test_pack_filters_layout():
    f = _filters()
    p = pack_filters(f, 6)
    assert p.shape == (8 * 25,) and p.dtype == torch.float32
    assert torch.equal(p[:25], f["l0"].reshape(25)) and torch.equal(p[25:50], f["h0"].reshape(25))
    assert torch.equal(p[50 + 5 * 25:], f["b"][5].reshape(25))


def test_no_source_file_holds_filter_coefficients():
    """the coefficients live in the fixture only: no source file of the library, the tests or the tools repeats one"""
    f = _filters()
    vals = {f"{abs(float(v)):.6g}".lstrip("0") for t in [f["l0"], f["h0"]] + f["b"] for v in t.reshape(-1) if abs(float(v)) > 1e-3}
    vals = {v for v in vals if len(v) >= 7}
    assert len(vals) > 20
    for base, exts in (("fov-3dgs_amd", (".py", ".hip", ".h")), ("include", (".h",)), ("tests", (".py",)), ("tools", (".py",))):
        for d, _, files in os.walk(os.path.join(ROOT, base)):
            for name in files:
                if name.endswith(exts):
                    txt = open(os.path.join(d, name), errors="replace").read()
                    hits = [v for v in vals if v in txt]
                    assert not hits, (name, hits[:3])


def test_abi_names_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fovraster.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fr_[a-z_0-9A-Z]+)\s*\(", txt))
    lib = _native.load()
    for n in ("fr_hvs_workspace_floats", "fr_hvs_forward", "fr_hvs_backward"):
        assert n in declared and n in _native.EXPORTS and hasattr(lib, n), n
    assert lib.fr_abi_version() == 12 == _native.ABI_VERSION


def test_workspace_sizes_and_refusals():
    st = _native_hvs.Settings(64, 96, 9.0, 5, 6, 0, 1)
    lv = _native_hvs.layout(st)  # asserts that the Python layout and the library agree on the size
    assert [v["identity"] for v in lv] == [False] * 4 and (lv[1]["ph"], lv[1]["pw"]) == (7, 10)
    assert [v["identity"] for v in _native_hvs.layout(_native_hvs.Settings(32, 64, 4.0, 5, 6, 0, 1))] == [False, False, True, True]
    assert all(v["identity"] for v in _native_hvs.layout(_native_hvs.Settings(32, 32, 1.0, 5, 6, 0, 1)))
    with pytest.raises(ValueError, match="multiple of 2"):
        _native_hvs.floats(_native_hvs.Settings(40, 64, 4.0, 5, 6, 0, 1), 0)
    with pytest.raises(ValueError, match="without a pooled pixel"):
        _native_hvs.floats(_native_hvs.Settings(32, 32, 64.0, 2, 6, 0, 1), 0)
    lib = _native.load()
    assert lib.fr_hvs_forward(32, 32, 1.0, 5, 6, 0, 1, None, None, None, None, None, None, None, None) == -1
    assert "null" in _native.last_error()


@pytest.mark.parametrize("i", [i for i in CASES if i not in (2, 4)])
def test_inputs_keep_the_absolute_value_away_from_its_kink(i):
    """L1 cases: the statistics that differ by less than 1e-9 carry no gradient that matters (tests/hvs_ref.py says why 1e-9)"""
    c = hc.case(i)
    f = hvs_ref.filters_to(hc.filters(c.orientations), dtype=torch.float64)
    n, share = hvs_ref.undecided_sign_gradient(torch.tensor(c.img, dtype=torch.float64), torch.tensor(c.tgt, dtype=torch.float64), f,
                                               c.pooling, c.levels)
    print(f"case {i}: {n} statistics differ by less than {hvs_ref.UNDECIDED}, share of the largest gradient {share:.3e}")
    assert share <= 2e-7  # (the generator's KINK_SHARE)
