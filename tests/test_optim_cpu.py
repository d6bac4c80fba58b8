"""fov3dgs_amd.optim without a GPU: the C layout of the descriptor table, the state_dict interchange with torch.optim.Adam,
argument validation, reference_param_groups, and the reference runs of tests/adam_ref.py checking themselves."""
import copy
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native, optim
from tests import adam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adam_structs_match_c_layout(tmp_path):
    ft = [f[0] for f in _native.AdamTensor._fields_]
    fa = [f[0] for f in _native.AdamArgs._fields_]
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/fovraster.h"', 'int main(){',
            'printf("%zu\\n", sizeof(fr_adam_tensor));']
    body += [f'printf("%zu\\n", offsetof(fr_adam_tensor, {f}));' for f in ft]
    body += ['printf("%zu\\n", sizeof(fr_adam_args));']
    body += [f'printf("%zu\\n", offsetof(fr_adam_args, {f}));' for f in fa]
    body += ['printf("%d %d %d %d %d\\n", FR_ADAM_MAX_TENSORS, FR_ADAM_DENSE, FR_ADAM_EXACT, FR_ADAM_LAZY, FR_ABI_VERSION);', 'return 0;}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert nums[0] == C.sizeof(_native.AdamTensor)
    for f, off in zip(ft, nums[1:1 + len(ft)]):
        assert getattr(_native.AdamTensor, f).offset == off, f
    k = 1 + len(ft)
    assert nums[k] == C.sizeof(_native.AdamArgs)
    for f, off in zip(fa, nums[k + 1:k + 1 + len(fa)]):
        assert getattr(_native.AdamArgs, f).offset == off, f
    assert nums[-5:] == [_native.ADAM_MAX_TENSORS, _native.ADAM_DENSE, _native.ADAM_EXACT, _native.ADAM_LAZY, _native.ABI_VERSION]
    assert _native.ABI_VERSION == 12


def test_native_rejects_bad_tables_without_launching():
    lib = _native.load()
    a = _native.AdamArgs()
    a.num_tensors = _native.ADAM_MAX_TENSORS + 1
    assert lib.fr_adam_step(C.byref(a), None) == -1 and b"tensors" in lib.fr_last_error()
    a.num_tensors = 1
    a.tensors[0].numel, a.tensors[0].width, a.tensors[0].mode = 12, 1, _native.ADAM_DENSE
    assert lib.fr_adam_step(C.byref(a), None) == -1 and b"null" in lib.fr_last_error()
    a.tensors[0].width = 0
    assert lib.fr_adam_step(C.byref(a), None) == -1 and b"bad sizes" in lib.fr_last_error()
    a.num_tensors = 0
    assert lib.fr_adam_step(C.byref(a), None) == 0  # nothing to do, nothing launched


def _cpu_model(P=40, seed=0):
    return {n: torch.nn.Parameter(p) for n, p in adam_ref.make_params(P, seed).items()}


def _torch_adam(ps):
    return torch.optim.Adam(adam_ref.groups_of(ps), lr=0.0, eps=1e-15)


def _set_grads(ps, seed):
    g = torch.Generator().manual_seed(seed)
    for p in ps.values():
        p.grad = torch.randn(p.shape, generator=g)


def test_state_dict_interchanges_with_torch_adam():
    ps = _cpu_model()
    t = _torch_adam(ps)
    for s in range(3):
        _set_grads(ps, s)
        t.step()
    sd = t.state_dict()

    ours = optim.Adam(adam_ref.groups_of(ps), lr=0.0, eps=1e-15)
    ours.load_state_dict(sd)
    back = ours.state_dict()
    assert back["state"].keys() == sd["state"].keys()
    for k in sd["state"]:
        assert set(back["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
        for f in ("step", "exp_avg", "exp_avg_sq"):
            a, b = back["state"][k][f], sd["state"][k][f]
            assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and torch.equal(a, b), (k, f)
    assert len(back["param_groups"]) == 6
    for ga, gb in zip(back["param_groups"], sd["param_groups"]):
        assert ga == gb  # every entry: name, lr, betas, eps, weight_decay, amsgrad, maximize, ..., params
    assert [g["name"] for g in back["param_groups"]] == list(adam_ref.NAMES)

    # torch continues from the re-exported dict exactly as it would have without the round trip
    ps2 = {n: torch.nn.Parameter(p.detach().clone()) for n, p in ps.items()}
    t2 = _torch_adam(ps2)
    t2.load_state_dict(copy.deepcopy(back))  # (a checkpoint: load_state_dict itself does not copy same-dtype tensors)
    _set_grads(ps, 99)
    _set_grads(ps2, 99)
    t.step()
    t2.step()
    for n in ps:
        assert torch.equal(ps[n], ps2[n]), n
        for f in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(t.state[ps[n]][f], t2.state[ps2[n]][f]), (n, f)


def test_fresh_state_dict_loads_into_torch_and_steps():
    ps = _cpu_model()
    ours = optim.Adam(adam_ref.groups_of(ps), lr=0.0, eps=1e-15)
    for g in ours.param_groups:
        assert g["weight_decay"] == 0 and g["amsgrad"] is False and g["maximize"] is False and g["eps"] == 1e-15
    t = torch.optim.Adam(adam_ref.groups_of(ps), lr=1.0)
    t.load_state_dict(ours.state_dict())
    _set_grads(ps, 0)
    t.step()  # indexes group["weight_decay"], group["amsgrad"], ... directly
    assert t.param_groups[0]["lr"] == adam_ref.LRS["xyz"] and t.param_groups[0]["eps"] == 1e-15


def test_load_refuses_what_the_kernel_does_not_do():
    ps = _cpu_model()
    for kw in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True)):
        t = torch.optim.Adam(adam_ref.groups_of(ps), lr=0.0, eps=1e-15, **kw)
        ours = optim.Adam(adam_ref.groups_of(ps), lr=0.0, eps=1e-15)
        with pytest.raises(ValueError):
            ours.load_state_dict(t.state_dict())


def test_step_has_no_cpu_fallback_and_arguments_are_validated():
    ps = _cpu_model()
    ours = optim.Adam(adam_ref.groups_of(ps), lr=0.0, eps=1e-15)
    _set_grads(ps, 0)
    before = {n: p.detach().clone() for n, p in ps.items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ours.step()
    assert all(torch.equal(before[n], ps[n]) for n in ps) and len(ours.state) == 0
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="Invalid learning rate"):
        optim.Adam(p, lr=-1.0)
    with pytest.raises(ValueError, match="Invalid beta parameter at index 0"):
        optim.Adam(p, betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="Invalid beta parameter at index 1"):
        optim.Adam(p, betas=(0.9, -0.1))
    with pytest.raises(ValueError, match="Invalid epsilon value"):
        optim.Adam(p, eps=-1e-8)
    with pytest.raises(ValueError, match="sparse"):
        optim.Adam(p, sparse="sloppy")
    with pytest.raises(ValueError):
        optim.Adam([{"params": p, "weight_decay": 0.1}])
    assert optim.Adam(p, sparse="lazy").sparse == "lazy" and optim.Adam(p).sparse == "exact"


def test_reference_param_groups():
    ps = adam_ref.make_params(7)
    model = SimpleNamespace(**{adam_ref.ATTRS[n]: torch.nn.Parameter(p) for n, p in ps.items()})
    args = SimpleNamespace(position_lr_init=0.00016, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
    groups = optim.reference_param_groups(model, args, spatial_lr_scale=2.5)
    assert [g["name"] for g in groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    lrs = {g["name"]: g["lr"] for g in groups}
    assert lrs == {"xyz": 0.00016 * 2.5, "f_dc": 0.0025, "f_rest": 0.0025 / 20.0, "opacity": 0.05, "scaling": 0.005, "rotation": 0.001}
    for g in groups:
        assert len(g["params"]) == 1 and g["params"][0] is getattr(model, adam_ref.ATTRS[g["name"]])
    assert optim.reference_param_groups(model, args)[0]["lr"] == 0.00016
    from fov3dgs_amd import synthetic as syn
    cloud = syn.scene_1k(P=10)
    assert [tuple(g["params"][0].shape[1:]) for g in optim.reference_param_groups(cloud, args)] == [(3,), (1, 3), (15, 3), (1,), (3,), (4,)]


def test_adam_ref_lazy_with_every_row_is_plain_adam_and_exact_is_adam_on_to_dense():
    P, steps = 50, 4
    ps = adam_ref.make_params(P)
    grads = adam_ref.make_grads(P, steps)
    every = torch.arange(P)
    dense, lazy_all, exact, on_dense = (adam_ref.RefAdam(ps, torch.float32) for _ in range(4))
    lazy = adam_ref.RefAdam(ps, torch.float32)
    for rows, g in grads:
        dense.step(g)
        lazy_all.step({n: adam_ref.to_row_sparse(x, every) for n, x in g.items()}, rule="lazy")
        sp = {n: adam_ref.to_row_sparse(x, rows) for n, x in g.items()}
        exact.step(sp, rule="exact")
        on_dense.step({n: x.to_dense() for n, x in sp.items()})
        lazy.step(sp, rule="lazy")
    a, b, c, d, e = dense.state(), lazy_all.state(), exact.state(), on_dense.state(), lazy.state()
    for n in adam_ref.NAMES:
        for k in range(3):
            assert torch.equal(a[n][k], b[n][k]), (n, k)
            assert torch.equal(c[n][k], d[n][k]), (n, k)
    # the lazy rule is a different optimizer: a row that was never listed has not moved and has no moments
    never = torch.ones(P, dtype=torch.bool)
    for rows, _ in grads:
        never[rows] = False
    assert never.any()
    assert torch.equal(e["xyz"][0][never], ps["xyz"][never].double()) and not e["xyz"][1][never].any()
    assert not torch.equal(e["xyz"][0], c["xyz"][0])
