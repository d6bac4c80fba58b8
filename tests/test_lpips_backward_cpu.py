"""The LPIPS backward pass without a GPU: that the frozen-decision restatement (tests/lpips_grad_ref.py) is lpips_ref.lpips, the
float32 autograd's own distance from float64 (the yardsticks of tests/test_lpips_backward_gpu.py), that the comparison sees a
dropped seam row and a wrong pool winner, the C ABI (symbols, struct layouts, refusals by field name, size queries), the backward
weight slabs, and the Python layer's refusals by name."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native, lpipsPyTorch
from tests import lpips_cases, lpips_grad_cases, lpips_grad_ref, lpips_ref, parity_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fr_lpips_backward_packed_bytes", "fr_lpips_pack_backward_weights", "fr_lpips_keep_workspace_bytes",
       "fr_lpips_keep_activation_offset", "fr_lpips_forward_keep", "fr_lpips_backward")
NAMES = list(lpips_cases.CASES)


def test_frozen_to_its_own_decisions_the_restatement_is_the_free_float64_autograd():
    w = lpips_cases.weights()
    for name in NAMES:
        c, g = lpips_cases.case(name), lpips_grad_cases.case(name)
        # the free run is lpips_ref.lpips under torch.autograd
        x = c["x"].double().requires_grad_(True)
        v = lpips_ref.lpips(x, c["y"], w, torch.float64)[0]
        gx, = torch.autograd.grad(v.sum(), x)
        assert float(v.detach()) == c["value64"] and torch.equal(g["value64"], v.detach()) and torch.equal(gx, g["grad64"])
        assert all(torch.equal(g["maps64"][l], t) for l, t in zip(lpips_grad_ref.TAP_LAYERS, c["feats64"]))
        vf, gf = lpips_grad_cases.frozen64(c["x"], c["y"], g["maps64"], name)
        dv = abs(float(vf) - c["value64"]) / c["value64"]
        dg = float((gf - gx).abs().max() / gx.abs().max())
        print(f"{name}: frozen against free float64: value {dv!r}, gradient {dg!r} of the largest element")
        assert dv <= 1e-12 and dg <= 1e-12 and float(gx.abs().max()) > 0


def test_the_float32_autograd_stays_within_the_recorded_yardsticks():
    worst = dict(ratio=0.0, l2=0.0, act=0.0)
    for name in NAMES:
        g = lpips_grad_cases.case(name)
        same = all(torch.equal(a > 0, b > 0) for a, b in zip(g["maps32"], g["maps64"]))
        _, g64 = lpips_grad_cases.frozen64(g["x"], g["y"], g["maps32"], name)  # float64, float32's decisions
        ratio, l2 = lpips_grad_cases.grad_ratio(g["grad32"], g64), lpips_grad_cases.grad_l2(g["grad32"], g64)
        act = max(lpips_cases.feature_ratio(a, b) for a, b in zip(g["maps32"], g["maps64"]))
        print(f"{name}: float32 autograd: ratio {ratio!r}, relative L2 {l2!r}, 13 maps {act!r}, float32's decisions are float64's: {same}")
        parity_report.record("lpips_gradient_f32", name, ratio=ratio, rel_l2=l2, maps_ratio=act, same_decisions=int(same))
        assert torch.isfinite(g["grad32"]).all() and g["grad32"].dtype == torch.float32
        worst = dict(ratio=max(worst["ratio"], ratio), l2=max(worst["l2"], l2), act=max(worst["act"], act))
    print(f"yardsticks: {worst} (recorded {lpips_grad_cases.GRAD_YARDSTICK}, {lpips_grad_cases.GRAD_L2_YARDSTICK}, {lpips_grad_cases.ACT_YARDSTICK})")
    # the recorded constants are one machine's measurement (torch's CPU kernels block their sums by thread count): this run's
    # figures go to the parity report, the GPU bounds stay the recorded yardsticks times 4
    assert lpips_grad_cases.GRAD_RTOL == 4 * lpips_grad_cases.GRAD_YARDSTICK and lpips_grad_cases.GRAD_L2_RTOL == 4 * lpips_grad_cases.GRAD_L2_YARDSTICK
    assert lpips_grad_cases.ACT_RTOL == 4 * lpips_grad_cases.ACT_YARDSTICK
    assert 0 < worst["ratio"] <= lpips_grad_cases.GRAD_RTOL and 0 < worst["l2"] <= lpips_grad_cases.GRAD_L2_RTOL
    assert 0 < worst["act"] <= lpips_grad_cases.ACT_RTOL


def _doctored(name, edit=None, reroute=None):
    """the float64 gradient of a case with `edit(l, grad)` applied to the gradient arriving at each post-ReLU map, and the pools'
    gradients sent where `reroute` says (lpips_grad_ref.activations)"""
    c, g = lpips_cases.case(name), lpips_grad_cases.case(name)
    w = lpips_cases.weights()
    x = c["x"].double().requires_grad_(True)
    ax = lpips_grad_ref.activations(x, w["features"], torch.float64, g["maps64"], reroute)
    if edit is not None:
        for l, a in enumerate(ax):
            a.register_hook(lambda grad, l=l: edit(l, grad))
    v = lpips_grad_ref.value(ax, g["ymaps64"], w["lin"], torch.float64)
    assert abs(float(v.detach()) - c["value64"]) <= 1e-12 * c["value64"]  # the doctoring touches the gradient only
    return torch.autograd.grad(v.sum(), x)[0]


def test_the_comparison_sees_a_dropped_seam_row_and_a_wrong_pool_winner():
    g = lpips_grad_cases.case("35x50")
    want = g["grad64"]
    assert lpips_grad_cases.grad_ratio(_doctored("35x50"), want) <= 1e-12
    # relu1_2's last row (35 -> 17: row 34 lies in no pool window and receives the tap's own gradient only) dropped

    def drop_row(l, grad):
        if l == 1:
            grad = grad.clone()
            grad[:, :, 34] = 0
        return grad
    r = lpips_grad_cases.grad_ratio(_doctored("35x50", edit=drop_row), want)
    print(f"relu1_2's uncovered row dropped: ratio {r!r} (bound {lpips_grad_cases.GRAD_RTOL})")
    assert r > lpips_grad_cases.GRAD_RTOL
    # ONE 2 x 2 window of relu1_2 (rows 10-11, columns 20-21) in one channel: the gradient goes to the second maximum
    m = g["maps64"][1]
    ch = int(m[0, :, 10:12, 20:22].reshape(64, 4).min(1).values.argmax())  # a channel alive at all four positions
    win = m[0, ch, 10:12, 20:22].reshape(4)
    second = int(win.argsort(descending=True)[1])
    assert float(win.min()) > 0 and len(set(win.tolist())) == 4

    def second_max(l, where):
        if l == 1:
            where = where.clone()
            where[0, ch, 5, 10] = (10 + second // 2) * 50 + 20 + second % 2
        return where
    r = lpips_grad_cases.grad_ratio(_doctored("35x50", reroute=second_max), want)
    print(f"one window's gradient sent to the second maximum: ratio {r!r} (bound {lpips_grad_cases.GRAD_RTOL})")
    assert r > lpips_grad_cases.GRAD_RTOL


def test_header_library_and_exports_carry_the_new_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fovraster.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fr_[a-z_0-9A-Z]+)\s*\(", txt))
    lib = _native.load()
    for n in NEW:
        assert n in declared and n in _native.EXPORTS and n not in _native.OPTIONAL_EXPORTS and hasattr(lib, n), n
    assert lib.fr_abi_version() == _native.ABI_VERSION  # symbols and structs were added, none changed: the version stays


@pytest.mark.parametrize("ctype,cname", [(_native.LpipsKeepArgs, "fr_lpips_keep_args"), (_native.LpipsBackwardArgs, "fr_lpips_backward_args")])
def test_the_ctypes_structs_match_the_header(tmp_path, ctype, cname):
    fields = [f[0] for f in ctype._fields_]
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/fovraster.h"', 'int main(){',
            f'printf("%zu\\n", sizeof({cname}));'] + [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in fields] + ['return 0;}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(body))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    nums = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert nums[0] == C.sizeof(ctype) and fields[0] == "size"
    for f, off in zip(fields, nums[1:]):
        assert getattr(ctype, f).offset == off, f


P = 4096  # non-null, aligned, never dereferenced: every call below fails validation first


def _keep_args(**kw):
    a = _native.LpipsKeepArgs(size=C.sizeof(_native.LpipsKeepArgs), N=1, H=16, W=16, debug=0, x=P, y=P, packed=P, workspace=P, keep=P, out=P)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _backward_args(**kw):
    a = _native.LpipsBackwardArgs(size=C.sizeof(_native.LpipsBackwardArgs), N=1, H=16, W=16, debug=0, packed_backward=P, keep=P, workspace=P,
                                  grad_out=P, grad_x=P)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_abi_refuses_by_field_name_without_launching():
    lib = _native.load()

    def bad(rc, word):
        assert rc == -1 and word in lib.fr_last_error(), (rc, word, lib.fr_last_error())
    calls = ((lib.fr_lpips_forward_keep, _keep_args, _native.LpipsKeepArgs, ("x", "y", "packed", "workspace", "keep", "out"),
              ("workspace", "keep"), "packed"),
             (lib.fr_lpips_backward, _backward_args, _native.LpipsBackwardArgs, ("packed_backward", "keep", "workspace", "grad_out", "grad_x"),
              ("workspace", "keep"), "packed_backward"))
    for fn, args, ctype, pointers, aligned256, aligned16 in calls:
        bad(fn(None), b"args is null")
        bad(fn(C.byref(args(size=C.sizeof(ctype) - 8))), b"size=")
        bad(fn(C.byref(args(size=0))), b"size=0")
        for H in (15, 16385):
            bad(fn(C.byref(args(H=H))), f"H={H}".encode())
            bad(fn(C.byref(args(W=H))), f"W={H}".encode())
        bad(fn(C.byref(args(N=0))), b"N=0")
        bad(fn(C.byref(args(N=513))), b"N=513")
        for f in pointers:
            bad(fn(C.byref(args(**{f: None}))), f"{f} is null".encode())
        for f in aligned256:
            bad(fn(C.byref(args(**{f: P + 64}))), b"aligned")
        bad(fn(C.byref(args(**{aligned16: P + 4}))), b"aligned")
    assert lib.fr_lpips_keep_workspace_bytes(1, 15, 16) == -1 and b"H=15" in lib.fr_last_error()
    assert lib.fr_lpips_keep_workspace_bytes(1, 16, 16385) == -1 and b"W=16385" in lib.fr_last_error()
    assert lib.fr_lpips_keep_workspace_bytes(0, 16, 16) == -1 and b"N=0" in lib.fr_last_error()
    assert lib.fr_lpips_keep_activation_offset(1, 16, 15, 0) == -1 and b"W=15" in lib.fr_last_error()
    assert lib.fr_lpips_keep_activation_offset(1, 16, 16, 13) == -1 and b"layer=13" in lib.fr_last_error()
    assert lib.fr_lpips_keep_activation_offset(1, 16, 16, -1) == -1 and b"layer=-1" in lib.fr_last_error()
    buf = torch.zeros(lib.fr_lpips_backward_packed_bytes(), dtype=torch.uint8)
    ws, _, _ = lpipsPyTorch._normalise(lpips_cases.weights())

    def ptrs(ts, hole=None):
        return (C.c_void_p * len(ts))(*[None if i == hole else t.data_ptr() for i, t in enumerate(ts)])
    bad(lib.fr_lpips_pack_backward_weights(None, buf.data_ptr()), b"conv_weights is null")
    bad(lib.fr_lpips_pack_backward_weights(ptrs(ws), None), b"packed_backward is null")
    bad(lib.fr_lpips_pack_backward_weights(ptrs(ws, 7), buf.data_ptr()), b"conv_weights[7]")


def test_the_kept_state_grows_with_every_dimension_and_stays_within_its_bound():
    lib = _native.load()
    base = lib.fr_lpips_keep_workspace_bytes(1, 16, 16)
    assert base >= 4 * sum(co * (16 >> s) ** 2 for (_, co), s in zip(lpips_ref.CHANNELS, (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)))
    for dims in (((1, H, 16) for H in (17, 33, 64, 139, 1080)), ((1, 16, W) for W in (17, 33, 64, 141, 1920)), ((N, 16, 16) for N in (2, 3, 8))):
        prev = base
        for d in dims:
            cur = lib.fr_lpips_keep_workspace_bytes(*d)
            assert cur > prev, d
            prev = cur
    # the 13 maps of one 1080 x 1920 picture: pooled sizes 540x960, 270x480, 135x240, 67x120
    maps = sum(co * (1080 >> s) * (1920 >> s) for (_, co), s in zip(lpips_ref.CHANNELS, (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)))
    assert maps == 559_779_840
    full = lib.fr_lpips_keep_workspace_bytes(1, 1080, 1920)
    print(f"kept state of one 1080 x 1920 pair: {full} bytes ({full / 1e9:.3f} GB); the 13 maps of one picture {4 * maps}")
    assert 4 * maps <= full <= 4 * (2 * maps + 2 * 64 * 1080 * 1920) + (1 << 20)
    assert full <= 4 * maps + 4 * sum(c * (1080 >> k) * (1920 >> k) for k, c in enumerate(lpips_ref.TAP_CHANNELS)) + (1 << 20)  # x's maps and five tap gradients
    offs = [lib.fr_lpips_keep_activation_offset(1, 1080, 1920, l) for l in range(13)]
    assert offs[0] == 0 and all(b > a and b % 256 == 0 for a, b in zip(offs, offs[1:])) and offs[-1] < full
    # what the evaluation call needs is what it was
    n_weights = sum(9 * ci * co + co for ci, co in lpips_ref.CHANNELS) + sum(lpips_ref.TAP_CHANNELS)
    assert lib.fr_lpips_packed_bytes() == 4 * n_weights
    two_buffers = 2 * (2 * 64 * 1080 * 1920 * 4)
    assert two_buffers <= lib.fr_lpips_workspace_bytes(1, 1080, 1920) <= two_buffers + (1 << 20)
    assert lib.fr_lpips_backward_packed_bytes() == 4 * sum(9 * ci * co for ci, co in lpips_ref.CHANNELS)


def test_the_backward_slabs_are_the_transposed_flipped_weights_in_the_kernels_layout():
    w = lpips_cases.weights()
    p = lpipsPyTorch.pack_backward_weights(w).view(torch.float32)
    assert p.numel() * 4 == _native.load().fr_lpips_backward_packed_bytes()
    # layer 2 (64 -> 128 forward, 128 -> 64 backward) read back the way k_lpips_conv reads it: [ob][ck][tap][cg][out][h]
    off = 27 * 64 + 9 * 64 * 64
    slabs = p[off:off + 9 * 64 * 128].reshape(1, 16, 9, 2, 64, 4)
    oihw = slabs.permute(0, 4, 1, 3, 5, 2).reshape(64, 128, 3, 3)  # out = 64 ob + out, in = 8 ck + 4 cg + h, tap = 3 ky + kx
    want = w["features"]["5.weight"].transpose(0, 1).flip(2, 3)
    assert torch.equal(oihw, want)
    # the last layer, 512 -> 512: eight output blocks
    off = p.numel() - 9 * 512 * 512
    oihw = p[off:].reshape(8, 64, 9, 2, 64, 4).permute(0, 4, 1, 3, 5, 2).reshape(512, 512, 3, 3)
    assert torch.equal(oihw, w["features"]["28.weight"].transpose(0, 1).flip(2, 3))
    # the first layer: [chunk of 8][tap][8][3]
    first = p[:27 * 64].reshape(8, 9, 8, 3).permute(3, 0, 2, 1).reshape(3, 64, 3, 3)
    assert torch.equal(first, w["features"]["0.weight"].transpose(0, 1).flip(2, 3))
    # and a convolution with them is the gradient of the forward convolution with respect to its input
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 64, 5, 6, generator=g, dtype=torch.float64).requires_grad_(True)
    up = torch.randn(1, 128, 5, 6, generator=g, dtype=torch.float64)
    (F.conv2d(x, w["features"]["5.weight"].double(), padding=1) * up).sum().backward()
    assert torch.allclose(F.conv2d(up, want.double(), padding=1), x.grad, rtol=1e-12, atol=1e-12)


def test_the_python_layer_refuses_by_name():
    w = lpips_cases.weights()
    lpipsPyTorch.set_default_weights(None)
    ok = torch.zeros(1, 3, 16, 16)
    for net in ("alex", "squeeze"):
        with pytest.raises(NotImplementedError, match="'vgg'"):
            lpipsPyTorch.LPIPSLoss(net, weights=w)
        with pytest.raises(NotImplementedError, match="'vgg'"):
            lpipsPyTorch.lpips_loss(ok, ok, net_type=net, weights=w)
    with pytest.raises(AssertionError, match="v0.1"):
        lpipsPyTorch.LPIPSLoss("vgg", version="0.0", weights=w)
    with pytest.raises(RuntimeError, match="weights="):
        lpipsPyTorch.LPIPSLoss()
    with pytest.raises(RuntimeError, match="weights="):
        lpipsPyTorch.lpips_loss(ok, ok)
    feats = dict(w["features"])
    del feats["17.bias"]
    with pytest.raises(KeyError, match="17.bias"):
        lpipsPyTorch.LPIPSLoss(weights=dict(features=feats, lin=w["lin"]))
    assert list(inspect.signature(lpipsPyTorch.lpips_loss).parameters) == ["x", "y", "net_type", "version", "weights"]
    assert inspect.signature(lpipsPyTorch.lpips_loss).parameters["net_type"].default == "vgg"
    assert list(inspect.signature(lpipsPyTorch.LPIPSLoss.__init__).parameters)[1:] == ["net_type", "version", "weights"]
    assert inspect.signature(lpipsPyTorch.LPIPSLoss.__init__).parameters["net_type"].default == "vgg"
    assert issubclass(lpipsPyTorch.LPIPSLoss, lpipsPyTorch.LPIPS)
    # the evaluation names are what they were
    assert list(inspect.signature(lpipsPyTorch.lpips).parameters) == ["x", "y", "net_type", "version", "weights"]
    assert inspect.signature(lpipsPyTorch.lpips).parameters["net_type"].default == "alex"
    assert list(inspect.signature(lpipsPyTorch.LPIPS.__init__).parameters)[1:] == ["net_type", "version", "weights"]
    with pytest.raises(RuntimeError, match="x requires grad"):
        lpipsPyTorch.LPIPS("vgg", weights=w)(ok.clone().requires_grad_(True), ok)
    crit = lpipsPyTorch.LPIPSLoss(weights=w)
    for call in (crit, lambda x, y: lpipsPyTorch.lpips_loss(x, y, weights=w)):
        for x in (ok, ok.clone().requires_grad_(True)):
            with pytest.raises(RuntimeError, match=r"y requires grad.*detach\(\)"):
                call(x, ok.clone().requires_grad_(True))
            with pytest.raises(ValueError, match="at least 16 x 16"):
                call(x[:, :, :15], ok[:, :, :15])
            with pytest.raises(ValueError, match="equal shapes"):
                call(x, torch.zeros(1, 3, 16, 17))
            with pytest.raises(ValueError, match=r"\[N,3,H,W\]"):
                call(x[0], ok[0])
            with pytest.raises(ValueError, match="float32"):
                call(x.double(), ok.double())
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call(x, ok)
        with pytest.raises(TypeError):
            call(ok.numpy(), ok)
    with pytest.raises(RuntimeError, match="differentiable forward first"):
        crit.activations()
