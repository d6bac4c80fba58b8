"""fov3dgs_amd.pruning without a GPU: the C ABI of the pruning entry points (symbols, layout, constants, argument
validation before any HIP call), and the reference restatements of tests/prune_ref.py checking themselves against torch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native, pruning
from fov3dgs_amd import synthetic as syn
from tests import prune_ref
from tests.adam_ref import ATTRS, NAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fr_prune_workspace_bytes", "fr_prune_metric_max", "fr_prune_select_lowest", "fr_compact_plan", "fr_compact_rows")


def test_header_library_and_exports_carry_the_new_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fovraster.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fr_[a-z_0-9A-Z]+)\s*\(", txt))
    lib = _native.load()
    for n in NEW:
        assert n in declared and n in _native.EXPORTS and hasattr(lib, n), n
    assert lib.fr_abi_version() == 12


def test_compact_structs_and_constants_match_c_layout(tmp_path):
    ft = [f[0] for f in _native.CompactTensor._fields_]
    fa = [f[0] for f in _native.CompactArgs._fields_]
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/fovraster.h"', 'int main(){',
            'printf("%zu\\n", sizeof(fr_compact_tensor));']
    body += [f'printf("%zu\\n", offsetof(fr_compact_tensor, {f}));' for f in ft]
    body += ['printf("%zu\\n", sizeof(fr_compact_args));']
    body += [f'printf("%zu\\n", offsetof(fr_compact_args, {f}));' for f in fa]
    body += ['printf("%d %d %d\\n", FR_COMPACT_MAX_TENSORS, FR_PRUNE_MAX_COMP_EFFICIENCY, FR_PRUNE_CONTRIB);', 'return 0;}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert nums[0] == C.sizeof(_native.CompactTensor)
    for f, off in zip(ft, nums[1:1 + len(ft)]):
        assert getattr(_native.CompactTensor, f).offset == off, f
    k = 1 + len(ft)
    assert nums[k] == C.sizeof(_native.CompactArgs)
    for f, off in zip(fa, nums[k + 1:k + 1 + len(fa)]):
        assert getattr(_native.CompactArgs, f).offset == off, f
    assert nums[-3:] == [_native.COMPACT_MAX_TENSORS, _native.PRUNE_MAX_COMP_EFFICIENCY, _native.PRUNE_CONTRIB] == [32, 0, 1]


def test_native_rejects_bad_arguments_without_launching():
    lib = _native.load()
    p = 4096  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails validation first

    def bad(rc, word):
        assert rc == -1 and word in lib.fr_last_error(), (rc, lib.fr_last_error())
    assert lib.fr_prune_workspace_bytes(0) == 0 and lib.fr_prune_workspace_bytes(-3) == 0
    assert lib.fr_prune_workspace_bytes(6_000_000) % 16 == 0 and 0 < lib.fr_prune_workspace_bytes(6_000_000) < (1 << 20)
    # metric
    bad(lib.fr_prune_metric_max(-1, 0, p, p, p, None), b"P=-1")
    bad(lib.fr_prune_metric_max(10, 2, p, p, p, None), b"kind")
    bad(lib.fr_prune_metric_max(10, -1, p, p, p, None), b"kind")
    bad(lib.fr_prune_metric_max(10, 0, None, p, p, None), b"null")
    bad(lib.fr_prune_metric_max(10, 0, p, None, p, None), b"null")
    bad(lib.fr_prune_metric_max(10, 1, p, None, None, None), b"null")
    assert lib.fr_prune_metric_max(0, 0, None, None, None, None) == 0
    # select
    bad(lib.fr_prune_select_lowest(-1, p, 0, p, p, None), b"P=-1")
    bad(lib.fr_prune_select_lowest(10, p, -1, p, p, None), b"k=-1")
    bad(lib.fr_prune_select_lowest(10, p, 11, p, p, None), b"k=11")
    bad(lib.fr_prune_select_lowest(10, None, 3, p, p, None), b"null")
    bad(lib.fr_prune_select_lowest(10, p, 3, None, p, None), b"null")
    bad(lib.fr_prune_select_lowest(10, p, 3, p, None, None), b"null")
    bad(lib.fr_prune_select_lowest(0, None, 1, None, None, None), b"k=1")
    assert lib.fr_prune_select_lowest(0, None, 0, None, None, None) == 0
    # plan
    bad(lib.fr_compact_plan(-1, p, 0, p, p, None), b"P=-1")
    bad(lib.fr_compact_plan(10, None, 0, p, p, None), b"null")
    bad(lib.fr_compact_plan(10, p, 0, None, p, None), b"null")
    bad(lib.fr_compact_plan(10, p, 0, p, None, None), b"null")
    assert lib.fr_compact_plan(0, None, 0, None, None, None) == 0
    # rows
    bad(lib.fr_compact_rows(None, None), b"null")
    a = _native.CompactArgs()
    a.P, a.num_tensors = 10, _native.COMPACT_MAX_TENSORS + 1
    bad(lib.fr_compact_rows(C.byref(a), None), b"tensors")
    a.num_tensors = -1
    bad(lib.fr_compact_rows(C.byref(a), None), b"tensors")
    a.num_tensors = 1
    bad(lib.fr_compact_rows(C.byref(a), None), b"null")  # no mask, no workspace
    a.mask, a.workspace = p, p
    a.tensors[0].row_words, a.tensors[0].dst_rows = 3, 5
    bad(lib.fr_compact_rows(C.byref(a), None), b"null")  # no data pointers
    a.tensors[0].src, a.tensors[0].dst, a.tensors[0].row_words = p, p, -1
    bad(lib.fr_compact_rows(C.byref(a), None), b"bad sizes")
    a.tensors[0].row_words, a.tensors[0].dst_rows = 3, 11
    bad(lib.fr_compact_rows(C.byref(a), None), b"bad sizes")
    a.P = -1
    bad(lib.fr_compact_rows(C.byref(a), None), b"P=-1")
    a.P, a.num_tensors = 0, 0
    assert lib.fr_compact_rows(C.byref(a), None) == 0
    a.P, a.num_tensors = 10, 0
    assert lib.fr_compact_rows(C.byref(a), None) == 0  # nothing to do, nothing launched


def _nasty(n, seed=0):
    """float32 values with everything the order has to get right: zeros of both signs, NaNs of both signs and several payloads,
    +-inf, negatives, denormals of both signs, and long runs of equal values."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n).astype(np.float32)
    special = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -1e-39, 1.0, -1.0, 3.5], dtype=np.float32)
    where = rng.random(n)
    v = np.where(where < 0.6, special[rng.integers(0, len(special), n)], v).astype(np.float32)
    bits = v.view(np.uint32).copy()
    odd_nan = rng.random(n) < 0.05
    bits[odd_nan] = np.uint32(0x7F800001) | (rng.integers(0, 1 << 22, n).astype(np.uint32)[odd_nan]) | (rng.integers(0, 2, n).astype(np.uint32)[odd_nan] << np.uint32(31))
    return bits.view(np.float32)


def test_key_model_is_torch_stable_sort():
    for n, seed in ((1, 0), (2, 1), (257, 2), (5000, 3), (100_000, 4)):
        m = _nasty(n, seed)
        _, want = torch.sort(torch.from_numpy(m.copy()), descending=False, dim=0, stable=True)
        assert np.array_equal(prune_ref.order(m), want.numpy()), n
        # ... also in the reference's [P,1] layout
        _, want2 = torch.sort(torch.from_numpy(m.copy()).unsqueeze(1), descending=False, dim=0, stable=True)
        assert np.array_equal(want2.squeeze(1).numpy(), want.numpy())
    m = _nasty(1000, 5)
    for k in (0, 1, 20, 500, 999, 1000):
        mask = prune_ref.lowest_k_mask(m, k)
        assert mask.sum() == k
        want = np.zeros(1000, dtype=bool)
        want[torch.sort(torch.from_numpy(m.copy()), stable=True)[1][:k].numpy()] = True
        assert np.array_equal(mask, want)
    z = np.zeros(100, dtype=np.float32)
    z[::2] = -0.0
    assert np.array_equal(np.nonzero(prune_ref.lowest_k_mask(z, 7))[0], np.arange(7))  # one tie: the lowest indices


def _literal_update(metrics, contribs, counts, metric):
    """What prune.py:82-86 (:90-92, :95-98 without the count) computes, in torch's own operations on [P,1] columns: the view's
    value is the contribution per tile test, 0 for a Gaussian no tile tested, and it replaces the metric where it is larger."""
    m = metrics.clone().unsqueeze(1)
    cur = contribs.unsqueeze(1).float()
    if metric == "max_comp_efficiency":
        tests = counts.unsqueeze(1).float()
        cur = cur / (tests + 1e-7)
        cur[tests < 1] = 0
    larger = m < cur
    m[larger] = cur[larger]
    return m.squeeze(1)


@pytest.mark.parametrize("metric", prune_ref.METRICS)
def test_metric_update_is_the_literal_torch_expression(metric):
    P = 4001
    got = np.zeros(P, dtype=np.float32)
    want = torch.zeros(P)
    for view in range(3):
        contribs, counts = prune_ref.metric_inputs(P, view)
        if view == 0:
            counts[:3] = torch.tensor([0, 1, 2], dtype=torch.int32)
            contribs[:3] = 0.3
        got = prune_ref.metric_update(got, contribs.numpy(), counts.numpy(), metric)
        want = _literal_update(want, contribs, counts, metric)
        assert np.array_equal(got.view(np.int32), want.numpy().view(np.int32)), view
        if view == 0 and metric == "max_comp_efficiency":
            # 1.0f + 1e-7f rounds to 1.00000012, 2.0f + 1e-7f to 2.0
            assert got[0] == 0 and got[1] == np.float32(0.3) / np.float32(1.00000012) and got[2] == np.float32(0.3) / np.float32(2.0)
            assert got[1] != np.float32(0.3)
    assert np.isfinite(got).all() and (got > 0).any()  # a NaN never gets in


def test_prune_ref_prune_points_is_direct_indexing():
    P = 40
    model = prune_ref.Model(syn.scene_1k(P=P), torch.optim.Adam)
    g = torch.Generator().manual_seed(0)
    for _ in range(2):
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        model.optimizer.step()
    before = {k: v.clone() for k, v in prune_ref.state_tensors(model).items()}
    mask = torch.rand(P, generator=g) < 0.4
    copy_ = prune_ref.clone_model(model)
    prune_ref.assert_same_state(model, copy_, "clone")
    prune_ref.prune_points(model, mask)
    after = prune_ref.state_tensors(model)
    assert after.keys() == before.keys()
    for k, v in before.items():
        want = v if k.endswith(".step") else v[~mask]
        assert prune_ref.same_bits(after[k], want), k
    n = int((~mask).sum())
    for name in NAMES:
        p = getattr(model, ATTRS[name])
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.shape[0] == n
        assert set(model.optimizer.state[p]) == {"step", "exp_avg", "exp_avg_sq"}
    assert len(model.optimizer.state) == 6
    prune_ref.assert_same_state(copy_, prune_ref.clone_model(copy_), "the copy is untouched and P rows long")
    assert copy_._xyz.shape[0] == P
    # side arrays of another length are zeroed at the new size; a group without state only loses rows
    fresh = prune_ref.Model(syn.scene_1k(P=P), torch.optim.Adam)
    fresh.xyz_gradient_accum = torch.ones(5, 1)
    prune_ref.prune_points(fresh, mask)
    assert len(fresh.optimizer.state) == 0 and fresh._rotation.shape == (n, 4)
    assert fresh.xyz_gradient_accum.shape == (n, 1) and not fresh.xyz_gradient_accum.any()
    assert fresh.denom.shape == (n, 1) and not fresh.denom.any() and fresh.max_radii2D.shape == (n,) and not fresh.max_radii2D.any()
    assert torch.equal(fresh.indexes, torch.arange(P)[~mask])


def test_pruning_has_no_cpu_fallback_and_validates_arguments():
    P = 10
    m = torch.zeros(P)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pruning.update_metric_(m, torch.ones(P), torch.ones(P, dtype=torch.int32), "max_comp_efficiency")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pruning.lowest_k_mask(m, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pruning.compact_rows(torch.ones(P, dtype=torch.bool), [torch.zeros(P, 3)])
    model = prune_ref.Model(syn.scene_1k(P=P), torch.optim.Adam)
    before = {k: v.clone() for k, v in prune_ref.state_tensors(model).items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pruning.prune_points(model, torch.zeros(P, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pruning.prune(model, "opacity", 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pruning.metric_pruning(model, [], None, torch.zeros(3))
    after = prune_ref.state_tensors(model)
    assert all(prune_ref.same_bits(before[k], after[k]) for k in before)
    with pytest.raises(ValueError, match="Prune method not recognized"):
        pruning.prune(model, "size", 0.5)
    with pytest.raises(ValueError, match="unknown pruning metric"):
        pruning.update_metric_(m, m, m, "biggest")
    with pytest.raises(ValueError, match="unknown pruning metric"):
        pruning.metric_pruning(model, [], None, torch.zeros(3), metric="biggest")
