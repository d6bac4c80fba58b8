"""The uniform metameric (HVS) loss without a GPU: the float64 restatement (tests/hvs_ref.py) against the reference's own vectors,
the pooling window / size rules against torch, the argument checks of the public class, and the ABI.
The second fixture (tests/golden/ref_hvs_edges.npz, cases E0 .. E7 listed at EDGE_CASES below) is held to the same rules: what it
holds, the restatement against the reference's vectors on ph > h levels, one-row and one-column pooled maps and asymmetric
filters, both kink conditions, the asymmetry of its filter sets, that E2, E4 and E7 SEE a mirrored l0, h0 or band filter where
the seven cases cannot, and the layout the library plans for them."""
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


# ---------------------------------------------------------------- the second fixture: ref_hvs_edges.npz (E0 .. E7)
EDGES = list(range(hc.EDGES))
#                (H, W, pooling, levels, orientations, type), asymmetric filters
EDGE_CASES = [((32, 32, 5, 5, 2, "L1"), False),     # E0: level 3 is 4x4 at p = 0.625, pooled 6x6 (ph > h)
              ((32, 32, 3, 5, 2, "MSE"), False),    # E1: two ph > h levels, 8x8 -> 10x10 and 4x4 -> 10x10
              ((16, 16, 3, 4, 1, "L1"), True),      # E2: one orientation; ph > h at 4x4 with asymmetric filters
              ((8, 8, 0.75, 2, 1, "L1"), True),     # E3: p < 1 at level 0, the fewest levels, an image smaller than a tile
              ((88, 136, 5, 3, 6, "L1"), True),     # E4: tile remainders 8, 8 at level 0 and 12, 4 at level 1 (44x68); p = 5, 2.5
              ((24, 72, 13, 3, 6, "L1"), True),     # E5: pooled maps of ONE row (1x5 at both levels); RGB and YCrCb
              ((36, 20, 13, 2, 4, "L1"), True),     # E6: pooled map 2x1, ONE column
              ((64, 64, 16, 6, 8, "MSE"), True)]    # E7: six levels, eight orientations, identity at the 4x4 last level
EDGE_SPACES = [(i, "RGB") for i in EDGES] + [(5, "YCrCb")]


def _edge_reference(i, colorspace):
    z, tag = hc.edges(), "" if colorspace == "RGB" else "_ycrcb"
    return float(z[f"loss_{i}{tag}"]), z[f"grad_{i}{tag}"]


def test_edge_fixture_holds_the_eight_cases():
    z = hc.edges()
    assert int(z["n"]) == hc.EDGES == len(EDGE_CASES)
    for i, (want, asym) in enumerate(EDGE_CASES):
        c = hc.edge_case(i)
        assert tuple(c[1:7]) == want and c.asymmetric == asym
        assert [int(v) for v in z[f"mapidx_{i}"]] == hc.edge_map_indices(c.pooling, c.levels, c.orientations)
        assert z[f"img_{i}"].dtype == np.uint16 == z[f"tgt_{i}"].dtype and z[f"grad_{i}"].dtype == np.float32
        assert z[f"grad_{i}"].shape == (1, 3, c.H, c.W) == z[f"img_{i}"].shape
    assert z["grad_5_ycrcb"].shape == z["grad_5"].shape and not np.array_equal(z["grad_5_ycrcb"], z["grad_5"])
    for no in (1, 4, 6, 8):
        assert z[f"afilters{no}_b"].shape == (no, 1, 1, 5, 5) and z[f"afilters{no}_b"].dtype == np.float32
        assert z[f"afilters{no}_l0"].shape == (1, 1, 5, 5) == z[f"afilters{no}_h0"].shape
    # arrays only: pictures, vectors, filter coefficients, case parameters
    assert all(v.dtype.kind in "fiu" for v in z.values())
    for f in ("ref_hvs_edges.npz", "ref_hvs_edges_maps.npz"):
        assert os.path.getsize(os.path.join(hc.GOLDEN, f)) < (1 << 20)


@pytest.mark.parametrize("i,colorspace", EDGE_SPACES)
def test_restatement_matches_the_reference_on_the_edge_cases(i, colorspace):
    """test_restatement_matches_the_reference_vectors' bound on the second fixture: it pins the restatement itself on ph > h
    windows, one-row and one-column maps and (E2 .. E7) on filters whose tap order matters, against the reference's own run"""
    z, y = hc.edges(), hc.edge_yardstick(i, colorspace)
    ref_loss, ref_grad = _edge_reference(i, colorspace)
    rel_loss = abs(ref_loss - y["loss"]) / y["loss"]
    l2, mx = hc.distances(ref_grad, y["grad"])
    parity_report.record("hvs", f"reference_vs_float64/E{i}/{colorspace}", rel_loss=rel_loss, grad_rel_l2=l2, grad_max_over_max=mx)
    print(f"E{i} {colorspace}: reference fp32 vs float64: rel loss {rel_loss:.3e} grad rel L2 {l2:.3e} max/max {mx:.3e}")
    assert rel_loss < 1e-4 and l2 < 1e-4 and mx < 1e-4
    if colorspace != "RGB":
        return
    idx = [int(v) for v in z[f"mapidx_{i}"]]
    for name, k in zip(("map0", "mapmid", "mapstd", "maplow"), idx):
        l2m, mxm = hc.distances(z[f"{name}_{i}"], y["maps"][k])
        print(f"   {name} (statistic {k}): rel L2 {l2m:.3e} max/max {mxm:.3e}")
        assert y["maps"][k].shape == z[f"{name}_{i}"].shape
        assert mxm < 1e-4, (name, mxm)


@pytest.mark.parametrize("i,colorspace", EDGE_SPACES)
def test_edge_inputs_keep_both_kinks_away(i, colorspace):
    c = hc.edge_case(i)
    f = hvs_ref.filters_to(hc.filters_of(c), dtype=torch.float64)
    img, tgt = torch.tensor(c.img, dtype=torch.float64), torch.tensor(c.tgt, dtype=torch.float64)
    assert hvs_ref.variances_outside_band(img, tgt, f, c.pooling, c.levels, image_colorspace=colorspace) == 0
    if c.loss_type == "L1":
        n, share = hvs_ref.undecided_sign_gradient(img, tgt, f, c.pooling, c.levels, image_colorspace=colorspace)
        print(f"E{i} {colorspace}: {n} statistics differ by less than {hvs_ref.UNDECIDED}, share of the largest gradient {share:.3e}")
        assert share <= 2e-7  # (the generator's KINK_SHARE)
        _, ref_grad = _edge_reference(i, colorspace)
        assert hc.distances(ref_grad, hc.edge_yardstick(i, colorspace)["grad"])[0] < 2e-5  # (the generator's REF_L2)


def _blocks(f):
    return [("l0", f["l0"]), ("h0", f["h0"])] + [(f"b[{k}]", b) for k, b in enumerate(f["b"])]


@pytest.mark.parametrize("no", [1, 4, 6, 8])
def test_asymmetric_filters_differ_from_every_mirror_image(no):
    """a condition on the fixture: a tap index swapped, flipped or reversed in a kernel changes every one of these filters by at
    least half its maximum, and no band filter is the negative of its rotation (which |a - b| and the std would not see)"""
    f = hvs_ref.filters_from_npz(hc.edges(), no, prefix="afilters")
    assert len(f["b"]) == no
    for name, a in _blocks(f):
        a = a.numpy().reshape(5, 5)
        assert hc.asymmetry(a) >= hc.ASYMMETRY, (name, hc.asymmetry(a))
        if name != "l0":  # unit L1 norm and no DC gain (make_hvs_edge_golden.py says why); l0 = a unit block + 1/25
            assert abs(np.abs(a).sum() - 1.0) < 1e-5 and abs(a.sum()) < 1e-6, name
        else:
            assert abs(np.abs(a - 1.0 / 25).sum() - 1.0) < 1e-5
    # and the reference's own sets are what the issue of the second fixture is about: they equal their mirror images
    g = hc.filters(6)
    assert hc.asymmetry(g["l0"].numpy()) == 0.0 == hc.asymmetry(g["h0"].numpy())
    assert all(hc.asymmetry(b.numpy()) < 1e-6 for b in g["b"])


def _doctored(f64, which):
    """a filter set with ONE mistake of the kind a tap index can make"""
    f = dict(f64, b=list(f64["b"]))
    if which == "l0 rotated":
        f["l0"] = torch.flip(f["l0"], (-2, -1))
    elif which == "h0 transposed":
        f["h0"] = f["h0"].transpose(-2, -1)
    else:
        f["b"][0] = torch.flip(f["b"][0], (-2, -1))
    return f


DOCTORINGS = ["l0 rotated", "h0 transposed", "band 0 rotated"]


@pytest.mark.parametrize("which", DOCTORINGS)
@pytest.mark.parametrize("i", [2, 4, 7])
def test_the_edge_cases_see_a_wrong_tap_order(i, which):
    """with ONE filter mirrored (in the forward of both pictures, the backward its transpose) the float64 restatement leaves the
    yardstick by at least 100 x the allowance the GPU tests grant the library: l0 and h0 in the loss or the gradient; a band
    rotated by 180 degrees at least in the stored mean map of band 0 ("mapmid")"""
    c, z, y = hc.edge_case(i), hc.edges(), hc.edge_yardstick(i)
    got = hc.evaluate(c, _doctored(hvs_ref.filters_to(hc.filters_of(c), dtype=torch.float64), which))
    ref_loss, ref_grad = _edge_reference(i, "RGB")
    if which != "band 0 rotated":
        rel, allow_rel = abs(got["loss"] - y["loss"]) / y["loss"], hc.allowance(abs(ref_loss - y["loss"]) / y["loss"])
        l2, allow_l2 = hc.distances(got["grad"], y["grad"])[0], hc.allowance(hc.distances(ref_grad, y["grad"])[0])
        print(f"E{i} {which}: rel loss {rel:.3e} (allowance {allow_rel:.3e}) grad rel L2 {l2:.3e} (allowance {allow_l2:.3e})")
        assert rel >= 100 * allow_rel or l2 >= 100 * allow_l2
    else:
        k = int(z[f"mapidx_{i}"][1])
        mx, allow = hc.distances(got["maps"][k], y["maps"][k])[1], hc.allowance(hc.distances(z[f"mapmid_{i}"], y["maps"][k])[1])
        print(f"E{i} {which}: mapmid max/max {mx:.3e} (allowance {allow:.3e})")
        assert mx >= 100 * allow


@pytest.mark.parametrize("which", DOCTORINGS)
@pytest.mark.parametrize("i", [0, 6])
def test_the_seven_cases_cannot_see_a_wrong_tap_order(i, which):
    """the gap the second fixture closes: the same mistakes with the reference's own filters move neither loss nor gradient"""
    c, y = hc.case(i), hc.yardstick(i)
    got = hc.evaluate(c, _doctored(hvs_ref.filters_to(hc.filters_of(c), dtype=torch.float64), which))
    rel, (l2, mx) = abs(got["loss"] - y["loss"]) / y["loss"], hc.distances(got["grad"], y["grad"])
    print(f"case {i} {which}: rel loss {rel:.3e} grad rel L2 {l2:.3e} max/max {mx:.3e}")
    assert rel <= 1e-6 and l2 <= 1e-6 and mx <= 1e-6


def test_layout_of_the_edge_cases():
    """ph > h at the levels E0 and E1 are named for, one pooled row for E5, one column for E6 (layout() itself asserts that the
    Python layout and fr_hvs_workspace_floats agree on the size)"""
    def lay(i):
        c = hc.edge_case(i)
        return _native_hvs.layout(_native_hvs.Settings(c.H, c.W, float(c.pooling), c.levels, c.orientations, int(c.loss_type == "MSE"), 1))
    e0, e1, e2, e3, e5, e6, e7 = (lay(i) for i in (0, 1, 2, 3, 5, 6, 7))
    assert not any(v["identity"] for v in e0 + e1 + e2 + e3 + e5 + e6)
    assert [(v["h"], v["ph"]) for v in e0] == [(32, 6), (16, 6), (8, 6), (4, 6)] and e0[3]["pw"] == 6
    assert [(v["h"], v["ph"]) for v in e1] == [(32, 10), (16, 10), (8, 10), (4, 10)] and (e1[2]["pw"], e1[3]["pw"]) == (10, 10)
    assert [(v["h"], v["ph"]) for v in e2] == [(16, 5), (8, 5), (4, 5)]
    assert [(v["h"], v["w"], v["ph"], v["pw"]) for v in e3] == [(8, 8, 10, 10)]
    assert [(v["ph"], v["pw"]) for v in e5] == [(1, 5), (1, 5)]
    assert [(v["h"], v["w"], v["ph"], v["pw"]) for v in e6] == [(36, 20, 2, 1)]
    assert [v["identity"] for v in e7] == [False, False, False, False, True] and (e7[4]["h"], e7[4]["w"]) == (4, 4)
    assert (e7[3]["ph"], e7[3]["pw"]) == (4, 4)


@pytest.mark.parametrize("i", [i for i in CASES if i not in (2, 4)])
def test_inputs_keep_the_absolute_value_away_from_its_kink(i):
    """L1 cases: the statistics that differ by less than 1e-9 carry no gradient that matters (tests/hvs_ref.py says why 1e-9)"""
    c = hc.case(i)
    f = hvs_ref.filters_to(hc.filters(c.orientations), dtype=torch.float64)
    n, share = hvs_ref.undecided_sign_gradient(torch.tensor(c.img, dtype=torch.float64), torch.tensor(c.tgt, dtype=torch.float64), f,
                                               c.pooling, c.levels)
    print(f"case {i}: {n} statistics differ by less than {hvs_ref.UNDECIDED}, share of the largest gradient {share:.3e}")
    assert share <= 2e-7  # (the generator's KINK_SHARE)
