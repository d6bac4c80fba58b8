"""LPIPS without a GPU: the restatement's own float32 distance to float64 (the yardstick of tests/test_lpips_gpu.py), the Python
layer's refusals by name, the weight packing (both key spellings, the slab layout the convolution kernel reads), the C ABI's
refusals by field name, the size queries, and evaluate_views(lpips=None) staying what it was."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native, lpipsPyTorch, quality
from fov3dgs_amd import synthetic as syn
from tests import lpips_cases, lpips_ref, parity_report, prune_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fr_lpips_packed_bytes", "fr_lpips_pack_weights", "fr_lpips_workspace_bytes", "fr_lpips_forward")


def test_the_restatement_in_float32_stays_within_the_recorded_yardsticks():
    worst_f = worst_v = 0.0
    for name in lpips_cases.CASES:
        c = lpips_cases.case(name)
        fr = [lpips_cases.feature_ratio(a, b) for a, b in zip(c["feats32"], c["feats64"])]
        vr = lpips_cases.value_ratios(c["taps32"], c["value32"], c)
        print(f"{name}: value64 {c['value64']!r} taps64 {[float(t) for t in c['taps64']]} feature ratios {fr} value ratios {vr}")
        parity_report.record("lpips_restatement_f32", name, feature_ratio=max(fr), value_ratio=max(vr), value64=c["value64"])
        assert all(math.isfinite(r) for r in fr + vr) and math.isfinite(c["value64"])
        assert all(torch.isfinite(f).all() for f in c["feats64"]) and all(float(t) > 0 for t in c["taps64"])
        assert abs(float(c["taps64"].sum()) - c["value64"]) <= 1e-12 * c["value64"]
        N, H, W = lpips_cases.CASES[name]
        assert [tuple(f.shape) for f in c["feats64"]] == [(N, ch, H >> k, W >> k) for k, ch in enumerate(lpips_ref.TAP_CHANNELS)]
        worst_f, worst_v = max(worst_f, max(fr)), max(worst_v, max(vr))
    print(f"yardsticks: features {worst_f!r} (recorded {lpips_cases.FEAT_YARDSTICK}), values {worst_v!r} (recorded {lpips_cases.VALUE_YARDSTICK})")
    # the recorded constants are one machine's measurement (torch's CPU kernels block their sums by thread count): the figures of
    # this run go to the parity report, the GPU bounds stay the recorded yardsticks times 4
    assert lpips_cases.FEAT_RTOL == 4 * lpips_cases.FEAT_YARDSTICK and lpips_cases.VALUE_RTOL == 4 * lpips_cases.VALUE_YARDSTICK
    assert 0 < worst_f < 1e-4 and 0 < worst_v < 1e-4  # float32, not something else


def test_the_batch_of_two_is_the_sum_of_its_pictures_in_the_restatement():
    c = lpips_cases.case("64x48n2")
    w = lpips_cases.weights()
    with torch.no_grad():
        singles = [float(lpips_ref.lpips(c["x"][i:i + 1], c["y"][i:i + 1], w, torch.float64)[0]) for i in range(2)]
    assert abs(sum(singles) - c["value64"]) <= 1e-12 * c["value64"] and min(singles) > 0


def test_header_library_and_exports_carry_the_new_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fovraster.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fr_[a-z_0-9A-Z]+)\s*\(", txt))
    lib = _native.load()
    for n in NEW:
        assert n in declared and n in _native.EXPORTS and n not in _native.OPTIONAL_EXPORTS and hasattr(lib, n), n
    assert "lpips.hip" in open(os.path.join(ROOT, "fov-3dgs_amd", "csrc", "Makefile")).read()


def test_the_ctypes_struct_matches_the_header(tmp_path):
    import subprocess
    fields = [f[0] for f in _native.LpipsArgs._fields_]
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/fovraster.h"', 'int main(){',
            'printf("%zu\\n", sizeof(fr_lpips_args));'] + [f'printf("%zu\\n", offsetof(fr_lpips_args, {f}));' for f in fields] + ['return 0;}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(body))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    nums = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert nums[0] == C.sizeof(_native.LpipsArgs)
    for f, off in zip(fields, nums[1:]):
        assert getattr(_native.LpipsArgs, f).offset == off, f


def _args(**kw):
    p = 4096  # non-null, aligned, never dereferenced: every call below fails validation first
    a = _native.LpipsArgs(size=C.sizeof(_native.LpipsArgs), N=1, H=16, W=16, debug=0, x=p, y=p, packed=p, workspace=p, out=p)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_abi_refuses_by_field_name_without_launching():
    lib = _native.load()

    def bad(rc, word):
        assert rc == -1 and word in lib.fr_last_error(), (rc, lib.fr_last_error())
    bad(lib.fr_lpips_forward(None), b"args is null")
    bad(lib.fr_lpips_forward(C.byref(_args(size=C.sizeof(_native.LpipsArgs) - 8))), b"size=")
    bad(lib.fr_lpips_forward(C.byref(_args(size=0))), b"size=0")
    bad(lib.fr_lpips_forward(C.byref(_args(H=15))), b"H=15")
    bad(lib.fr_lpips_forward(C.byref(_args(W=15))), b"W=15")
    bad(lib.fr_lpips_forward(C.byref(_args(H=16385))), b"H=16385")
    bad(lib.fr_lpips_forward(C.byref(_args(N=0))), b"N=0")
    bad(lib.fr_lpips_forward(C.byref(_args(N=513))), b"N=513")
    for f in ("x", "y", "packed", "workspace", "out"):
        bad(lib.fr_lpips_forward(C.byref(_args(**{f: None}))), f"{f} is null".encode())
    bad(lib.fr_lpips_forward(C.byref(_args(workspace=4096 + 64))), b"aligned")
    bad(lib.fr_lpips_forward(C.byref(_args(packed=4096 + 4))), b"aligned")
    assert lib.fr_lpips_workspace_bytes(1, 15, 16) == -1 and b"H=15" in lib.fr_last_error()
    assert lib.fr_lpips_workspace_bytes(0, 16, 16) == -1 and b"N=0" in lib.fr_last_error()
    # the packing routine: a null array, a null entry
    buf = torch.zeros(lib.fr_lpips_packed_bytes(), dtype=torch.uint8)
    ws, bs, ls = lpipsPyTorch._normalise(lpips_cases.weights())

    def ptrs(ts, hole=None):
        return (C.c_void_p * len(ts))(*[None if i == hole else t.data_ptr() for i, t in enumerate(ts)])
    bad(lib.fr_lpips_pack_weights(None, ptrs(bs), ptrs(ls), buf.data_ptr()), b"conv_weights is null")
    bad(lib.fr_lpips_pack_weights(ptrs(ws), None, ptrs(ls), buf.data_ptr()), b"conv_biases is null")
    bad(lib.fr_lpips_pack_weights(ptrs(ws), ptrs(bs), None, buf.data_ptr()), b"lin_weights is null")
    bad(lib.fr_lpips_pack_weights(ptrs(ws), ptrs(bs), ptrs(ls), None), b"packed is null")
    bad(lib.fr_lpips_pack_weights(ptrs(ws, 7), ptrs(bs), ptrs(ls), buf.data_ptr()), b"conv_weights[7]")
    bad(lib.fr_lpips_pack_weights(ptrs(ws), ptrs(bs, 12), ptrs(ls), buf.data_ptr()), b"conv_biases[12]")
    bad(lib.fr_lpips_pack_weights(ptrs(ws), ptrs(bs), ptrs(ls, 4), buf.data_ptr()), b"lin_weights[4]")


def test_the_size_queries_grow_with_every_dimension():
    lib = _native.load()
    n_weights = sum(9 * ci * co + co for ci, co in lpips_ref.CHANNELS) + sum(lpips_ref.TAP_CHANNELS)
    assert lib.fr_lpips_packed_bytes() == 4 * n_weights
    base = lib.fr_lpips_workspace_bytes(1, 16, 16)
    assert base >= 2 * (2 * 64 * 16 * 16 * 4)
    prev = base
    for H in (17, 33, 64, 139, 1080):
        cur = lib.fr_lpips_workspace_bytes(1, H, 16)
        assert cur > prev
        prev = cur
    prev = base
    for W in (17, 33, 64, 141, 1920):
        cur = lib.fr_lpips_workspace_bytes(1, 16, W)
        assert cur > prev
        prev = cur
    prev = base
    for N in (2, 3, 8):
        cur = lib.fr_lpips_workspace_bytes(N, 16, 16)
        assert cur > prev
        prev = cur
    full = lib.fr_lpips_workspace_bytes(1, 1080, 1920)
    two_buffers = 2 * (2 * 64 * 1080 * 1920 * 4)
    assert two_buffers <= full <= two_buffers + (1 << 20)  # the README's 2.1 GB: two ping-pong buffers and under 1 MiB beside them


def _respelled(w):
    return dict(features={"features." + k: v for k, v in w["features"].items()} | {"classifier.0.bias": torch.zeros(3)},
                lin={k.replace("lin", "").replace("model.", ""): v for k, v in w["lin"].items()})


def test_both_key_spellings_pack_to_the_same_bytes_and_the_slabs_are_what_the_kernel_reads():
    w = lpips_cases.weights()
    before = lpipsPyTorch.PACK_COUNT
    a, b = lpipsPyTorch.pack_weights(w), lpipsPyTorch.pack_weights(_respelled(w))
    assert lpipsPyTorch.PACK_COUNT == before + 2
    assert a.dtype == torch.uint8 and a.numel() == _native.load().fr_lpips_packed_bytes() and torch.equal(a, b)
    assert "0.1.weight" in _respelled(w)["lin"] and "features.28.bias" in _respelled(w)["features"]
    p = a.view(torch.float32)
    # layer 2 (64 -> 128) read back the way k_lpips_conv reads it: slab (output block, 8-channel chunk) = [tap][group of 4][64][4]
    off = (27 * 64 + 64) + (9 * 64 * 64 + 64)
    slabs = p[off:off + 9 * 64 * 128].reshape(2, 8, 9, 2, 64, 4)  # [ob][ck][tap][cg][co][h]
    oihw = slabs.permute(0, 4, 1, 3, 5, 2).reshape(128, 64, 3, 3)  # co = 64 ob + co, ci = 8 ck + 4 cg + h, tap = 3 ky + kx
    assert torch.equal(oihw, w["features"]["5.weight"])
    assert torch.equal(p[off + 9 * 64 * 128:off + 9 * 64 * 128 + 128], w["features"]["5.bias"])
    # the first layer: [27][64]
    assert torch.equal(p[:27 * 64].reshape(27, 64).t().reshape(64, 3, 3, 3), w["features"]["0.weight"])
    assert torch.equal(p[-512:], w["lin"]["lin4.model.1.weight"].reshape(512))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 64, 5, 6, generator=g)
    assert torch.equal(F.conv2d(x, oihw, padding=1), F.conv2d(x, w["features"]["5.weight"], padding=1))


def test_the_python_layer_refuses_by_name():
    w = lpips_cases.weights()
    lpipsPyTorch.set_default_weights(None)
    for net in ("alex", "squeeze"):
        with pytest.raises(NotImplementedError, match="'vgg'"):
            lpipsPyTorch.LPIPS(net, weights=w)
        with pytest.raises(NotImplementedError, match="'vgg'"):
            lpipsPyTorch.lpips(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16), net_type=net, weights=w)
    with pytest.raises(NotImplementedError, match="'vgg'"):
        lpipsPyTorch.LPIPS(weights=w)  # the reference's default net_type is 'alex'
    assert list(inspect.signature(lpipsPyTorch.lpips).parameters) == ["x", "y", "net_type", "version", "weights"]
    assert inspect.signature(lpipsPyTorch.lpips).parameters["net_type"].default == "alex"
    assert list(inspect.signature(lpipsPyTorch.LPIPS.__init__).parameters)[1:] == ["net_type", "version", "weights"]
    with pytest.raises(AssertionError, match="v0.1"):
        lpipsPyTorch.LPIPS("vgg", version="0.0", weights=w)
    with pytest.raises(RuntimeError, match="weights="):
        lpipsPyTorch.LPIPS("vgg")
    with pytest.raises(RuntimeError, match="weights="):
        lpipsPyTorch.lpips(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16), net_type="vgg")
    # a missing key, a wrong shape: named
    feats = dict(w["features"])
    del feats["17.bias"]
    with pytest.raises(KeyError, match="17.bias"):
        lpipsPyTorch.LPIPS("vgg", weights=dict(features=feats, lin=w["lin"]))
    lin = dict(w["lin"])
    del lin["lin3.model.1.weight"]
    with pytest.raises(KeyError, match="lin3.model.1.weight"):
        lpipsPyTorch.LPIPS("vgg", weights=dict(features=w["features"], lin=lin))
    with pytest.raises(KeyError, match="'lin'"):
        lpipsPyTorch.LPIPS("vgg", weights=dict(features=w["features"]))
    feats = dict(w["features"])
    feats["10.weight"] = torch.zeros(256, 128, 3, 2)
    with pytest.raises(ValueError, match=r"10.weight has shape \(256, 128, 3, 2\)"):
        lpipsPyTorch.LPIPS("vgg", weights=dict(features=feats, lin=w["lin"]))
    lin = dict(w["lin"])
    lin["lin1.model.1.weight"] = torch.zeros(1, 64, 1, 1)
    with pytest.raises(ValueError, match="lin 1 has shape"):
        lpipsPyTorch.set_default_weights(dict(features=w["features"], lin=lin))
    with pytest.raises(TypeError, match="dict"):
        lpipsPyTorch.LPIPS("vgg", weights=[1, 2])
    # the pictures
    crit = lpipsPyTorch.LPIPS("vgg", weights=w)
    ok = torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError, match="at least 16 x 16"):
        crit(torch.zeros(1, 3, 15, 16), torch.zeros(1, 3, 15, 16))
    with pytest.raises(ValueError, match="at least 16 x 16"):
        crit(torch.zeros(1, 3, 16, 15), torch.zeros(1, 3, 16, 15))
    with pytest.raises(ValueError, match="equal shapes"):
        crit(ok, torch.zeros(1, 3, 16, 17))
    with pytest.raises(ValueError, match="equal shapes"):
        crit(ok, torch.zeros(2, 3, 16, 16))
    with pytest.raises(ValueError, match=r"\[N,3,H,W\]"):
        crit(torch.zeros(3, 16, 16), torch.zeros(3, 16, 16))
    with pytest.raises(ValueError, match="float32"):
        crit(ok.double(), ok.double())
    with pytest.raises(RuntimeError, match="x requires grad"):
        crit(ok.clone().requires_grad_(True), ok)
    with pytest.raises(RuntimeError, match="y requires grad"):
        crit(ok, ok.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(ok, ok)
    with pytest.raises(TypeError):
        crit(ok.numpy(), ok)


def test_the_package_holds_no_download_code():
    src = open(os.path.join(ROOT, "fov-3dgs_amd", "lpipsPyTorch", "__init__.py")).read()
    for word in ("http", "torch.hub", "urllib", "requests", "load_state_dict_from_url", "import torchvision", "from torchvision"):
        assert word not in src, word


def test_load_weights_reads_local_files(tmp_path):
    w = lpips_cases.weights()
    small = dict(features={k: v for k, v in w["features"].items() if k.startswith("0.")}, lin={"lin0.model.1.weight": w["lin"]["lin0.model.1.weight"]})
    torch.save(small["features"], tmp_path / "f.pth")
    torch.save(small["lin"], tmp_path / "l.pth")
    got = lpipsPyTorch.load_weights(tmp_path / "f.pth", tmp_path / "l.pth")
    assert set(got) == {"features", "lin"} and torch.equal(got["features"]["0.weight"], w["features"]["0.weight"])
    assert torch.equal(got["lin"]["lin0.model.1.weight"], w["lin"]["lin0.model.1.weight"])
    with pytest.raises(KeyError, match="2.weight"):  # the incomplete set is refused by name
        lpipsPyTorch.set_default_weights(got)


class _Cam:
    image_width, image_height = 8, 8
    original_image = torch.zeros(3, 8, 8)


def test_evaluate_views_without_lpips_is_what_it_was():
    sig = inspect.signature(quality.evaluate_views)
    assert list(sig.parameters) == ["model", "cameras", "pipe", "bg", "render", "hvs", "resize", "lpips"]
    assert sig.parameters["lpips"].default is None and sig.parameters["hvs"].default is None and sig.parameters["resize"].default == "pyramid"
    model = prune_ref.Model(syn.scene_1k(P=10), torch.optim.Adam)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        quality.evaluate_views(model, [_Cam()], None, torch.zeros(3))
    with pytest.raises(ValueError, match="no cameras"):
        quality.evaluate_views(model, [], None, torch.zeros(3), lpips=None)
