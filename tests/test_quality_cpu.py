"""The quality gate, the scale-decay loss and the opacity cap without a GPU: the C ABI of the new entry points (symbols,
argument validation before any HIP call), the Python entry points' refusal of CPU tensors and malformed arguments, and the
golden file tests/golden/ref_quality.npz checking its float64 values against a restatement on its own stored inputs."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native, image_utils, pruning, quality
from fov3dgs_amd import synthetic as syn
from tests import prune_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fr_quality_blocks", "fr_quality_forward", "fr_quality_finish", "fr_scale_decay_blocks", "fr_scale_decay_forward",
       "fr_scale_decay_backward", "fr_opacity_cap")


def test_header_library_and_exports_carry_the_new_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fovraster.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fr_[a-z_0-9A-Z]+)\s*\(", txt))
    lib = _native.load()
    for n in NEW:
        assert n in declared and n in _native.EXPORTS and n not in _native.OPTIONAL_EXPORTS and hasattr(lib, n), n
    assert lib.fr_abi_version() == 12 == _native.ABI_VERSION


def test_native_rejects_bad_arguments_without_launching():
    lib = _native.load()
    p = 4096  # a non-null, aligned address that is never dereferenced: every call below fails validation first

    def bad(rc, word):
        assert rc == -1 and word in lib.fr_last_error(), (rc, lib.fr_last_error())
    # one (ssim, squared error, absolute error) triple per 16 x 32 tile of a channel
    assert lib.fr_quality_blocks(3, 37, 53) == 3 * 2 * 4 and lib.fr_quality_blocks(1, 9, 5) == 1 and lib.fr_quality_blocks(3, 1080, 1920) == 3 * 34 * 120
    assert lib.fr_quality_blocks(0, 4, 4) == 0 and lib.fr_quality_blocks(3, -1, 4) == 0 and lib.fr_quality_blocks(65536, 4, 4) == 0
    bad(lib.fr_quality_forward(0, 4, 4, 1, p, p, p, None), b"C=0")
    bad(lib.fr_quality_forward(65536, 4, 4, 1, p, p, p, None), b"C=65536")
    bad(lib.fr_quality_forward(3, 4, 4, 1, None, p, p, None), b"null")
    bad(lib.fr_quality_forward(3, 4, 4, 1, p, None, p, None), b"null")
    bad(lib.fr_quality_forward(3, 4, 4, 1, p, p, None, None), b"null")
    bad(lib.fr_quality_forward(3, 4, 4, 1, p, p, p + 4, None), b"aligned")
    bad(lib.fr_quality_finish(3, 0, 4, 1, p, p, 0, 1, p, None), b"H=0")
    bad(lib.fr_quality_finish(3, 4, 4, 2, p, p, 0, 2, p, None), b"rows=2")
    bad(lib.fr_quality_finish(3, 4, 4, 0, p, p, 0, 2, p, None), b"rows=0")
    bad(lib.fr_quality_finish(3, 4, 4, 1, p, p, 2, 2, p, None), b"outside")    # the slot after the last
    bad(lib.fr_quality_finish(3, 4, 4, 3, p, p, 1, 3, p, None), b"outside")    # three rows from slot 1 of 3
    bad(lib.fr_quality_finish(3, 4, 4, 1, p, p, -1, 2, p, None), b"outside")
    bad(lib.fr_quality_finish(3, 4, 4, 1, None, p, 0, 2, p, None), b"null")
    bad(lib.fr_quality_finish(3, 4, 4, 1, p, None, 0, 2, p, None), b"null")
    bad(lib.fr_quality_finish(3, 4, 4, 1, p, p, 0, 2, p + 4, None), b"aligned")
    # scale decay
    assert [lib.fr_scale_decay_blocks(n) for n in (-1, 0, 1, 256, 257, 4097)] == [0, 0, 1, 1, 2, 17]
    for fn, word in ((lib.fr_scale_decay_forward, b"forward"), (lib.fr_scale_decay_backward, b"backward")):
        bad(fn(0, p, p, 4, 0, p, p, None), b"P=0")
        bad(fn(-5, p, p, 4, 0, p, p, None), b"P=-5")
        bad(fn(10, None, p, 4, 0, p, p, None), b"null")
        bad(fn(10, p, None, 4, 0, p, p, None), b"null")
        bad(fn(10, p, p, 4, 0, p, None, None), b"null")
        assert word in lib.fr_last_error()
    bad(lib.fr_scale_decay_forward(10, p, p, 4, 0, None, p, None), b"null")
    bad(lib.fr_scale_decay_forward(10, p, p, 4, 0, p + 4, p, None), b"aligned")
    # cap
    bad(lib.fr_opacity_cap(-1, p, 0.5, 0.0, p, p, p, None), b"P=-1")
    for m in (0.0, 1.0, -0.1, 1.5, float("nan")):
        bad(lib.fr_opacity_cap(10, p, m, 0.0, p, p, p, None), b"(0, 1)")
    bad(lib.fr_opacity_cap(10, None, 0.5, 0.0, p, p, p, None), b"null")
    bad(lib.fr_opacity_cap(10, p, 0.5, 0.0, None, p, p, None), b"null")
    assert lib.fr_opacity_cap(0, None, 0.5, 0.0, None, None, None, None) == 0


class _Cam:
    image_width, image_height = 8, 8
    original_image = torch.zeros(3, 8, 8)


def test_entry_points_have_no_cpu_fallback_and_validate_arguments():
    a, b = torch.rand(3, 8, 8), torch.rand(3, 8, 8)
    for fn in (image_utils.mse, image_utils.psnr):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(a, b)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(a[None], b[None])
        with pytest.raises(ValueError, match="differ"):
            fn(a, b[:, :7])
        with pytest.raises(ValueError, match="at least two dimensions"):
            fn(a.reshape(-1), b.reshape(-1))
        with pytest.raises(ValueError, match="floating-point"):
            fn(a.to(torch.int32), b.to(torch.int32))
        with pytest.raises(TypeError):
            fn(a.numpy(), b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        quality.QualityMeter("cpu", 4)
    for cap in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="capacity"):
            quality.QualityMeter("cuda:0", cap)
    model = prune_ref.Model(syn.scene_1k(P=10), torch.optim.Adam)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        quality.evaluate_views(model, [_Cam()], None, torch.zeros(3))
    with pytest.raises(ValueError, match="no cameras"):
        quality.evaluate_views(model, [], None, torch.zeros(3))
    # scale decay
    P = 10
    s, c = torch.rand(P, 3), torch.arange(P, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pruning.scale_decay_loss(s, c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pruning.scale_decay_loss(s, c.unsqueeze(1), threshold=2, raw=True)
    for bad_s in (torch.rand(P, 4), torch.rand(P), torch.rand(0, 3), torch.rand(P, 3, 1)):
        with pytest.raises(ValueError, match="scaling"):
            pruning.scale_decay_loss(bad_s, c)
    with pytest.raises(ValueError, match="float32"):
        pruning.scale_decay_loss(s.double(), c)
    with pytest.raises(ValueError, match="gs_count"):
        pruning.scale_decay_loss(s, c[:-1])
    with pytest.raises(ValueError, match="gs_count"):
        pruning.scale_decay_loss(s, torch.zeros(P, 2, dtype=torch.int32))
    for dtype in (torch.int64, torch.float32, torch.bool):
        with pytest.raises(ValueError, match="int32"):
            pruning.scale_decay_loss(s, c.to(dtype))
    for t in (2.5, None, True, 2 ** 31):
        with pytest.raises(ValueError, match="threshold"):
            pruning.scale_decay_loss(s, c, threshold=t)
    with pytest.raises(TypeError):
        pruning.scale_decay_loss(s.numpy(), c)
    # cap
    before = {k: v.clone() for k, v in prune_ref.state_tensors(model).items()}
    for fn in (lambda: pruning.reset_opacity_max(model), lambda: pruning.reset_opacity_max(model, max=0.1),
               lambda: pruning.reset_opacity(model), lambda: pruning.reset_opacity_upper_bound(model, 0.5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    for m in (0.0, 1.0, -0.5, 1.01, float("nan"), None, "0.5", True):
        with pytest.raises(ValueError, match=r"\(0, 1\)"):
            pruning.reset_opacity_max(model, max=m)
        with pytest.raises(ValueError, match=r"\(0, 1\)"):
            pruning.reset_opacity_upper_bound(model, m)
    after = prune_ref.state_tensors(model)
    assert after.keys() == before.keys() and all(prune_ref.same_bits(before[k], after[k]) for k in before)
    assert [g["params"][0] for g in model.optimizer.param_groups if g["name"] == "opacity"][0] is model._opacity


def _ssim64(a, b):
    """loss_utils.py:26-34, :57-76 restated in float64: the 11x11 window as the outer product of the normalised 1-D window (built
    in fp32, as the reference builds it), five zero-padded grouped convolutions, the map's mean."""
    g = torch.tensor([np.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    C = a.shape[0]
    w = g.mm(g.t()).float().expand(C, 1, 11, 11).double().contiguous()
    a, b = a[None], b[None]

    def conv(t):
        return F.conv2d(t, w, padding=5, groups=C)
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return float(m.mean())


def test_the_golden_float64_values_reproduce_from_the_stored_inputs():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_quality.npz"))
    assert int(z["n"]) == 4
    shapes = [(3, 37, 53), (3, 70, 33), (1, 9, 5), (3, 16, 16)]
    for i, shape in enumerate(shapes):
        a32, b32 = z[f"a{i}"], z[f"b{i}"]
        assert a32.shape == b32.shape == shape and a32.dtype == b32.dtype == np.float32
        a, b = a32.astype(np.float64), b32.astype(np.float64)
        d = a - b
        mse, mse_ch = (d ** 2).mean(), (d ** 2).reshape(shape[0], -1).mean(1)
        assert z[f"mse64_{i}"].dtype == np.float64 and z[f"ssim64_{i}"].dtype == np.float64 and z[f"ssim_{i}"].dtype == np.float32
        np.testing.assert_allclose(z[f"mse64_{i}"], mse, rtol=1e-13)
        np.testing.assert_allclose(z[f"mse_ch64_{i}"], mse_ch, rtol=1e-13)
        np.testing.assert_allclose(z[f"l164_{i}"], np.abs(d).mean(), rtol=1e-13)
        np.testing.assert_allclose(z[f"ssim64_{i}"], _ssim64(torch.from_numpy(a), torch.from_numpy(b)), rtol=1e-12)
        with np.errstate(divide="ignore"):
            psnr, psnr_ch = 20 * np.log10(1 / np.sqrt(mse)), 20 * np.log10(1 / np.sqrt(mse_ch))
        if i == 3:  # equal pictures
            assert mse == 0 and np.isposinf(z[f"psnr64_{i}"]) and np.isposinf(z[f"psnr_{i}"]) and np.isposinf(z[f"psnr_ch_{i}"]).all()
            assert z[f"ssim_{i}"] == 1 and z[f"l1_{i}"] == 0 and z[f"psnr_gap_{i}"] == 0
        else:
            np.testing.assert_allclose(z[f"psnr64_{i}"], psnr, rtol=1e-13)
            np.testing.assert_allclose(z[f"psnr_ch64_{i}"], psnr_ch, rtol=1e-13)
            # the reference's fp32 values lie where fp32 arithmetic puts them, and the stored gaps are those distances
            assert abs(abs(float(z[f"psnr_{i}"]) - psnr) - z[f"psnr_gap_{i}"]) < 1e-12 and z[f"psnr_gap_{i}"] < 5e-6
            np.testing.assert_allclose(np.abs(z[f"psnr_ch_{i}"].astype(np.float64) - psnr_ch), z[f"psnr_ch_gap_{i}"], rtol=0, atol=1e-12)
            assert z[f"psnr_ch_gap_{i}"].max() < 5e-6
            assert abs(float(z[f"ssim_{i}"]) - float(z[f"ssim64_{i}"])) < 1e-6 and abs(float(z[f"l1_{i}"]) - float(z[f"l164_{i}"])) < 1e-6
            assert abs(float(z[f"mse_{i}"]) / mse - 1) < 1e-6
