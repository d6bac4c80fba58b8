"""The foveated metameric (HVS) loss without a GPU: the restatement (tests/hvs_fov_ref.py) against the reference's own vectors
(tests/golden/ref_hvs_fov.npz, from make_hvs_fov_golden.py) in float64 and in float32, its LOD maps against the stored ones, both
kink conditions of the fixture, the chain rule of supported sizes, the argument checks of the public class, and the ABI."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native
from fov3dgs_amd.hvs_loss_calc import HVSLoss
from fov3dgs_amd.odak_perception import MetamericLoss, _native_hvs_fov
from tests import hvs_cases as hc
from tests import hvs_fov_cases as fc
from tests import hvs_fov_ref, hvs_ref, parity_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(range(8))
#       (H, W, levels, orientations, alpha, mode, type, gaze, width, distance, colour space)
WANT = [(32, 64, 5, 6, 0.05, "quadratic", "MSE", (0.5, 0.5), 1.0, 0.5, "RGB"),
        (32, 64, 5, 6, 3.0, "quadratic", "L1", (0.3, 0.6), 1.0, 0.5, "RGB"),
        (64, 96, 5, 6, 0.5, "quadratic", "L1", (0.5, 0.5), 1.0, 0.5, "RGB"),
        (96, 64, 5, 2, 0.5, "quadratic", "MSE", (0.5, 0.5), 1.0, 0.5, "YCrCb"),
        (40, 56, 3, 6, 2.0, "linear", "L1", (0.2, 0.7), 1.0, 0.5, "RGB"),
        (64, 64, 5, 6, 0.001, "quadratic", "L1", (0.5, 0.5), 1.0, 0.5, "RGB"),
        (64, 64, 5, 6, 0.001, "quadratic", "MSE", (0.5, 0.5), 1.0, 0.5, "RGB"),
        (64, 96, 4, 6, 0.3, "quadratic", "MSE", (1.2, -0.1), 2.0, 1.0, "RGB")]


def test_fixture_holds_the_cases():
    z = fc.golden()
    assert fc.n_cases() == 8 == len(fc.NAMES)
    for i, want in enumerate(WANT):
        c = fc.case(i)
        assert tuple(c[2:13]) == want, (i, tuple(c[2:13]))
        assert z[f"img_{i}"].dtype == np.uint16 == z[f"tgt_{i}"].dtype and z[f"grad_{i}"].dtype == np.float32
        assert z[f"grad_{i}"].shape == (1, 3, c.H, c.W) == z[f"img_{i}"].shape
        for l in range(c.levels - 1):
            assert z[f"lod_{i}_{l}"].shape == (c.H >> l, c.W >> l) and z[f"lod_{i}_{l}"].dtype == np.float32
    assert all(v.dtype.kind in "fiu" for v in z.values())  # arrays only: pictures, vectors, maps, case parameters
    for f in ("ref_hvs_fov.npz", "ref_hvs_fov_maps.npz"):
        assert os.path.getsize(os.path.join(hc.GOLDEN, f)) < (1 << 20)


def test_the_cases_reach_what_they_are_named_for():
    z = fc.golden()
    lod = lambda i, l: z[f"lod_{i}_{l}"]
    # F0: a little foveation at level 0, the deeper levels all-identity
    assert 0 < lod(0, 0).max() < 1 and all(lod(0, l).max() == 0 for l in (1, 2, 3))
    # F1: 32x64 ends 1x2 -> the appended mean is the last level K = 6, and it is sampled (lod > 5)
    assert hvs_fov_ref.chain_sizes(32, 64)[-3:] == [(2, 4), (1, 2), (1, 1)] and lod(1, 0).max() > 5
    # F2: LOD up to about 5 of a 7-level chain (K = 6)
    assert len(hvs_fov_ref.chain_sizes(64, 96)) == 7 and 4.5 < lod(2, 0).max() < 6
    # F4: odd mip sizes at level 0 (40x56 -> .. 5x7 -> 2x3 -> 1x1) and lod >= K there
    assert hvs_fov_ref.chain_sizes(40, 56)[3:] == [(5, 7), (2, 3), (1, 1)] and lod(4, 0).max() >= 5
    # F5: lod = 0 everywhere
    assert all(lod(i, l).max() == 0 for i in (5, 6) for l in range(4))
    # F6: the gaze lies outside the picture: no pixel of level 0 is unblurred at its far corner, and the LOD grows away from it
    assert lod(7, 0)[0, -1] < lod(7, 0)[-1, 0]


@pytest.mark.parametrize("i", CASES)
def test_restatement_in_float64_matches_the_reference_vectors(i):
    """float64 restatement vs the reference's float32 run: the difference is the reference's rounding, which also is the
    allowance of the GPU tests (x3): bounded here by 1e-4 relative as for the uniform loss (tests/test_hvs_cpu.py), far above
    fp32 rounding of these sums and far below any mistake in a window, a weight, a blend or a LOD. The stored maps were blended
    with the reference's float32 LOD maps, d off the float64 ones (test_restated_lod_maps_match_the_stored_ones): a blend
    (1 - f) a + f b moves by d |b - a| <= 2 d max |map|, which is added to the maps' bound."""
    c, z, y = fc.case(i), fc.golden(), fc.yardstick(i)
    rel_loss = abs(float(z[f"loss_{i}"]) - y["loss"]) / y["loss"]
    l2, mx = hc.distances(z[f"grad_{i}"], y["grad"])
    parity_report.record("hvs_fov", f"reference_vs_float64/{c.name}", rel_loss=rel_loss, grad_rel_l2=l2, grad_max_over_max=mx)
    print(f"{c.name}: reference fp32 vs float64: rel loss {rel_loss:.3e} grad rel L2 {l2:.3e} max/max {mx:.3e}")
    assert rel_loss < 1e-4 and l2 < 1e-4 and mx < 1e-4
    idx = [int(v) for v in z[f"mapidx_{i}"]]
    for name, k in zip(("map0", "mapmid", "mapstd", "maplow"), idx):
        l2m, mxm = hc.distances(z[f"{name}_{i}"], y["maps"][k])
        print(f"   {name} (statistic {k}): rel L2 {l2m:.3e} max/max {mxm:.3e}")
        assert y["maps"][k].shape == z[f"{name}_{i}"].shape
        level = 0 if k < 2 else min((k // 2 - 1) // c.orientations, c.levels - 2)
        d = 0.0 if name == "maplow" else fc.max_abs(z[f"lod_{i}_{level}"], y["lods"][level])
        assert mxm < 1e-4 + 2 * d, (name, mxm, d)


@pytest.mark.parametrize("i", CASES)
def test_restatement_in_float32_matches_the_reference_vectors(i):
    """the restatement run as the reference runs, float32 on the CPU, against the reference's stored float32 run. Both are
    float32 evaluations of one formula that add in different orders, so each is about one reference-distance from the float64
    yardstick: their distance is bounded by twice the GPU tests' allowance of the reference's own distance (one allowance for
    each of the two)."""
    c, z, y = fc.case(i), fc.golden(), fc.yardstick(i)
    got = fc.restate(c, torch.float32)
    ref_rel = abs(float(z[f"loss_{i}"]) - y["loss"]) / y["loss"]
    ref_l2, ref_mx = hc.distances(z[f"grad_{i}"], y["grad"])
    rel = abs(got["loss"] - float(z[f"loss_{i}"])) / y["loss"]
    l2, mx = hc.distances(got["grad"], z[f"grad_{i}"])
    parity_report.record("hvs_fov", f"float32_restatement_vs_reference/{c.name}", rel_loss=rel, grad_rel_l2=l2, grad_max_over_max=mx)
    print(f"{c.name}: fp32 restatement vs reference: rel loss {rel:.3e} ({ref_rel:.3e}) grad rel L2 {l2:.3e} ({ref_l2:.3e}) "
          f"max/max {mx:.3e} ({ref_mx:.3e})")
    assert rel <= 2 * hc.allowance(ref_rel) and l2 <= 2 * hc.allowance(ref_l2) and mx <= 2 * hc.allowance(ref_mx)


# The reference builds its LOD maps in float32. Its dot product of two unit vectors is off by up to ~2 ulp = 2.4e-7, and
# eccentricity^2 ~ 2 (1 - dot) by twice that. The pooling size goes with ecc^2 ("quadratic") or ecc ("linear"), so lod =
# log2(pooling) is off by d(ecc^2) / (ecc^2 ln 2), or half that. The LOD is positive only where the pooling size exceeds a pixel:
# the smallest ecc^2 with lod > 0 among the cases is F4's (linear, alpha 2, 56 pixels wide), about 3e-4, which gives 1.2e-3;
# everything else (tan, sqrt, log2, the 1e-6) is within a few ulp of a number below 12.
LOD_ABS = 5e-3


@pytest.mark.parametrize("i", CASES)
def test_restated_lod_maps_match_the_stored_ones(i):
    c, z, y = fc.case(i), fc.golden(), fc.yardstick(i)
    for l in range(c.levels - 1):
        d = fc.max_abs(z[f"lod_{i}_{l}"], y["lods"][l])
        parity_report.record("hvs_fov", f"reference_vs_float64/{c.name}/lod{l}", max_abs=d)
        print(f"{c.name} level {l}: reference fp32 LOD map vs float64: max |d| {d:.3e} (max LOD {y['lods'][l].max():.3f})")
        assert d < LOD_ABS
        assert ((z[f"lod_{i}_{l}"] == 0) == (y["lods"][l] <= LOD_ABS)).mean() > 0.99  # the unblurred region is the same one


@pytest.mark.parametrize("i", CASES)
def test_inputs_keep_both_kinks_away(i):
    c, y = fc.case(i), fc.yardstick(i)
    f = hvs_ref.filters_to(hc.filters(c.orientations), dtype=torch.float64)
    lods = [torch.tensor(m) for m in y["lods"]]
    img, tgt = torch.tensor(c.img, dtype=torch.float64), torch.tensor(c.tgt, dtype=torch.float64)
    assert hvs_fov_ref.variances_outside_band(img, tgt, f, lods, c.levels, image_colorspace=c.colorspace) == 0
    if c.loss_type == "L1":
        n, share = hvs_fov_ref.undecided_sign_gradient(img, tgt, f, lods, c.levels, image_colorspace=c.colorspace)
        print(f"{c.name}: {n} statistics differ by less than {hvs_ref.UNDECIDED}, share of the largest gradient {share:.3e}")
        assert share <= 2e-7  # (the generator's KINK_SHARE)
        assert hc.distances(fc.golden()[f"grad_{i}"], y["grad"])[0] < 2e-5  # (the generator's REF_L2)


def test_blur_at_lod_zero_is_the_identity_and_the_variance_is_zero():
    """where lod = 0 the blend is (1 - 0) x + 0 up_1 = x in every precision: the variance is 0 exactly and the standard
    deviation the constant sqrt(1e-7) (csrc/hvs_fov.hip forms x x where it samples level 0 and relies on this)"""
    for dt in (torch.float32, torch.float64):
        x = torch.rand(1, 3, 16, 32, dtype=dt, generator=torch.Generator().manual_seed(3))
        lod = torch.zeros(16, 32, dtype=dt)
        assert torch.equal(hvs_fov_ref.blur(x, lod), x)
        m, s, v = hvs_fov_ref.find_stats(x, lod)
        assert torch.equal(v, torch.zeros_like(v)) and torch.equal(s, torch.full_like(s, 1e-7).sqrt())


@pytest.mark.parametrize("n", [2, 3, 5, 7, 15, 17, 40])
def test_chain_step_is_the_adaptive_window_mean(n):
    """scale_factor=0.5, mode="area": size floor(n / 2), windows [floor(j n / n'), ceil((j + 1) n / n'))"""
    x = torch.arange(n * n, dtype=torch.float64).reshape(1, 1, n, n) ** 1.5
    down = F.interpolate(x, scale_factor=0.5, mode="area", recompute_scale_factor=False)
    n2 = n // 2
    assert down.shape[-2:] == (n2, n2)
    for jy in range(n2):
        ys, ye = hvs_ref.window(jy, n, n2)
        for jx in range(n2):
            xs, xe = hvs_ref.window(jx, n, n2)
            assert abs(float(x[0, 0, ys:ye, xs:xe].mean()) - float(down[0, 0, jy, jx])) <= 1e-12 * float(down[0, 0, jy, jx])


def test_blend_is_continuous_in_the_lod():
    x = torch.rand(1, 1, 16, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    K = len(hvs_fov_ref.chain_sizes(16, 16)) - 1
    for k in range(1, K + 1):
        below = hvs_fov_ref.blur(x, torch.full((16, 16), k - 1e-9, dtype=torch.float64))
        at = hvs_fov_ref.blur(x, torch.full((16, 16), float(k), dtype=torch.float64))
        assert (below - at).abs().max() < 1e-8
    top = hvs_fov_ref.blur(x, torch.full((16, 16), K + 3.5, dtype=torch.float64))
    assert torch.equal(top, hvs_fov_ref.blur(x, torch.full((16, 16), float(K), dtype=torch.float64)))


def test_abi_names_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fovraster.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fr_[a-z_0-9A-Z]+)\s*\(", txt))
    lib = _native.load()
    for n in ("fr_hvs_fov_workspace_floats", "fr_hvs_fov_forward", "fr_hvs_fov_backward", "fr_hvs_fov_backward_plan"):
        assert n in declared and n in _native.EXPORTS and n not in _native.OPTIONAL_EXPORTS and hasattr(lib, n), n
    assert lib.fr_abi_version() == 12 == _native.ABI_VERSION
    assert "hvs_fov.hip" in open(os.path.join(ROOT, "fov-3dgs_amd", "csrc", "Makefile")).read()


def _settings(H, W, levels=5, no=6, Hs=0, Ws=0):
    return _native_hvs_fov.Settings(H, W, 0.05, 1.0, 0.5, 1, 0.5, 0.5, levels, no, 1, 1, Hs, Ws)


@pytest.mark.parametrize("H,W", [(64, 32), (32, 96), (96, 32)])
def test_sizes_on_which_the_reference_raises_are_refused(H, W):
    with pytest.raises(ValueError, match=rf"level \d \(\d+x\d+\).*reference.*fails") as e:
        _native_hvs_fov.floats(_settings(H, W), 0)
    print(e.value)
    with pytest.raises(ValueError):
        [hvs_fov_ref.chain_sizes(H >> l, W >> l) for l in range(4)]  # the restatement refuses them too


@pytest.mark.parametrize("H,W,levels", [(1088, 1920, 5), (32, 64, 5), (32, 32, 5), (64, 64, 5), (64, 96, 5), (96, 64, 5), (40, 56, 3),
                                        (136, 244, 2), (200, 344, 3), (392, 408, 3), (64, 64, 6)])  # ... and ref_hvs_fov_large.npz's
def test_supported_sizes_and_their_layout(H, W, levels):
    st = _settings(H, W, levels)
    lv = _native_hvs_fov.layout(st)  # asserts that the Python layout and the library agree on the sizes
    assert len(lv) == levels - 1 and all(v["chain"][-1] == (1, 1) for v in lv)
    assert all(_native_hvs_fov.floats(st, which) > 0 for which in (0, 1, 2, 3))
    if (H, W) == (1088, 1920):
        assert [s for s in lv[0]["chain"] if s[0] % 2 or s[1] % 2][:3] == [(17, 30), (8, 15), (4, 7)]  # odd sizes occur: 17 -> 8, 15 -> 7
        assert len({len(v["chain"]) + l for l, v in enumerate(lv)}) == 1  # every level ends after the same number of halvings
        rs = _settings(H, W, levels, Hs=1080, Ws=1920)
        assert _native_hvs_fov.floats(rs, 1) == _native_hvs_fov.floats(st, 1) + 3 * H * W


def test_workspace_refusals():
    with pytest.raises(ValueError, match="multiple of 2"):
        _native_hvs_fov.floats(_settings(40, 64), 0)
    with pytest.raises(ValueError, match="shrinking"):
        _native_hvs_fov.floats(_settings(64, 64, Hs=80, Ws=64), 1)
    with pytest.raises(ValueError, match="which"):
        _native_hvs_fov.floats(_settings(64, 64), 4)
    lib = _native.load()
    head = (0, 0, 64, 64, 0.05, 1.0, 0.5, 1, 0.5, 0.5, 5, 6, 1, 1)
    assert lib.fr_hvs_fov_forward(*head, None, None, None, None, None, None, 0, None, None, None) == -1
    assert "null" in _native.last_error()
    assert lib.fr_hvs_fov_backward(*head, None, None, None, None, None, None, None, None) == -1
    assert "null" in _native.last_error()
    bad = (0, 0, 64, 64, 0.05, -1.0, 0.5, 1, 0.5, 0.5, 5, 6, 1, 1)
    assert lib.fr_hvs_fov_forward(*bad, None, None, None, None, None, None, 0, None, None, None) == -1
    assert "real_image_width" in _native.last_error()


def test_argument_checks():
    f = hc.filters(6)
    ok = dict(use_bilinear_downup=True, use_l2_foveal_loss=False, n_orientations=6, filters=f)
    with pytest.raises(NotImplementedError, match="use_bilinear_downup"):
        MetamericLoss(**dict(ok, use_bilinear_downup=False))
    with pytest.raises(NotImplementedError, match="use_l2_foveal_loss"):
        MetamericLoss(**dict(ok, use_l2_foveal_loss=True))
    with pytest.raises(NotImplementedError, match="use_l2_foveal_loss"):
        MetamericLoss(use_bilinear_downup=True, n_orientations=6, filters=f)  # (the reference's default is True)
    with pytest.raises(NotImplementedError, match="use_radial_weight"):
        MetamericLoss(use_radial_weight=True, **ok)
    with pytest.raises(NotImplementedError, match="use_fullres_l0"):
        MetamericLoss(use_fullres_l0=True, **ok)
    with pytest.raises(NotImplementedError, match="equi"):
        MetamericLoss(equi=True, **ok)
    with pytest.raises(ValueError, match="mode"):
        MetamericLoss(mode="cubic", **ok)
    with pytest.raises(ValueError, match="loss_type"):
        MetamericLoss(loss_type="L2", **ok)
    with pytest.raises(ValueError, match="n_pyramid_levels"):
        MetamericLoss(n_pyramid_levels=7, **ok)
    with pytest.raises(ValueError, match="n_orientations"):
        MetamericLoss(**dict(ok, n_orientations=9))
    with pytest.raises(ValueError, match="holds 2"):
        MetamericLoss(**dict(ok, filters=hc.filters(2)))
    with pytest.raises(ValueError, match="alpha"):
        MetamericLoss(alpha=-1.0, **ok)
    with pytest.raises(ValueError, match="real_image_width"):
        MetamericLoss(real_image_width=0.0, **ok)
    with pytest.raises(ValueError, match="real_viewing_distance"):
        MetamericLoss(real_viewing_distance=0.0, **ok)
    MetamericLoss(fovea_weight=False, **ok)  # any fovea_weight without the foveal term, as HVSLoss passes
    fn = MetamericLoss(device="cuda", alpha=0.05, real_image_width=1.0, real_viewing_distance=0.5, **ok)
    x = torch.rand(1, 3, 32, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(x, x.clone())
    with pytest.raises(ValueError, match="multiple of 2"):
        fn(torch.rand(1, 3, 40, 64), torch.rand(1, 3, 40, 64))
    with pytest.raises(ValueError, match="resize="):
        fn(x, x.clone(), resize="nearest")
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
    for gaze in ([0.5], [0.5, float("nan")], "ab", None, [0.1, 0.2, 0.3]):
        with pytest.raises(ValueError, match="gaze"):
            fn(x, x.clone(), gaze=gaze)
    with pytest.raises(TypeError, match="tensors"):
        fn(x.numpy(), x)


def test_hvsloss_is_built_as_the_reference_builds_it():
    hvs = HVSLoss(filters=hc.filters(6))
    u, f = hvs.uniform_loss, hvs.fov_loss
    assert (u.pooling_size, u.n_pyramid_levels, u.n_orientations, u.loss_type, u.bilinear_downsampling) == (1, 5, 6, "MSE", True)
    assert (f.alpha, f.real_image_width, f.real_viewing_distance, f.n_pyramid_levels, f.mode, f.n_orientations, f.loss_type) == \
        (0.05, 1.0, 0.5, 5, "quadratic", 6, "MSE")
    assert f.use_l2_foveal_loss is False and f.fovea_weight is False and f.use_bilinear_downup is True
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hvs.calc_fov_loss(torch.rand(1, 3, 30, 60), torch.rand(1, 3, 30, 60))
