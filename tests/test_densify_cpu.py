"""fov3dgs_amd.densify without a GPU: the C ABI of the densification entry points (symbols, layout, constants, argument
validation before any HIP call), the argument errors of densify.py, and the restatement the GPU tests compare against:
tests/densify_ref.py's literal four-pass densify_and_prune equals its one-decision-per-source-row formulation."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native, densify
from fov3dgs_amd import synthetic as syn
from tests import densify_ref, prune_ref
from tests.adam_ref import ATTRS, NAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fr_densify_workspace_bytes", "fr_densify_stats", "fr_densify_plan", "fr_densify_rows")
PERCENT_DENSE, EXTENT = 0.08, 1.0   # t_dense = 0.08: about the median largest scale of scene_1k; t_world = 0.1
MAX_GRAD, MIN_OPACITY = 0.2, 0.1


def cpu_model(P, seed=0, steps=2):
    model = prune_ref.Model(syn.scene_1k(P=P, seed=seed), torch.optim.Adam)
    model.percent_dense = PERCENT_DENSE
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        model.optimizer.step()
    model.optimizer.zero_grad(set_to_none=True)
    # (prune_ref.Model: accum = rand, denom = 0 .. 8, so denom = 0 with accum > 0 is there) + 0 / 0 and negative sums
    kind = torch.rand(P, generator=g)
    model.xyz_gradient_accum[kind < 0.1] *= -1.0
    zero = (kind >= 0.1) & (kind < 0.2)
    model.xyz_gradient_accum[zero] = 0.0
    model.denom[zero] = 0.0
    return model


def test_header_library_and_exports_carry_the_new_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fovraster.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fr_[a-z_0-9A-Z]+)\s*\(", txt))
    lib = _native.load()
    for n in NEW:
        assert n in declared and n in _native.EXPORTS and hasattr(lib, n), n


def test_densify_structs_and_constants_match_c_layout(tmp_path):
    pairs = (("fr_densify_plan_args", _native.DensifyPlanArgs), ("fr_densify_tensor", _native.DensifyTensor),
             ("fr_densify_rows_args", _native.DensifyRowsArgs))
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/fovraster.h"', 'int main(){']
    for cname, ct in pairs:
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f[0]}));' for f in ct._fields_]
    body += ['printf("%d %d %d %d %d %d %d %d %d\\n", FR_DENSIFY_CLONE_MASK, FR_DENSIFY_SPLIT_MASK, FR_DENSIFY_CLONE_GRAD, FR_DENSIFY_SPLIT_GRAD,'
             ' FR_DENSIFY_AND_PRUNE, FR_DENSIFY_COPY, FR_DENSIFY_ZERO_NEW, FR_DENSIFY_XYZ, FR_DENSIFY_SCALING);', 'return 0;}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    k = 0
    for cname, ct in pairs:
        assert nums[k] == C.sizeof(ct), cname
        for f, off in zip(ct._fields_, nums[k + 1:]):
            assert getattr(ct, f[0]).offset == off, (cname, f[0])
        k += 1 + len(ct._fields_)
    assert nums[k:] == [_native.DENSIFY_CLONE_MASK, _native.DENSIFY_SPLIT_MASK, _native.DENSIFY_CLONE_GRAD, _native.DENSIFY_SPLIT_GRAD,
                        _native.DENSIFY_AND_PRUNE, _native.DENSIFY_COPY, _native.DENSIFY_ZERO_NEW, _native.DENSIFY_XYZ,
                        _native.DENSIFY_SCALING] == [0, 1, 2, 3, 4, 0, 1, 2, 3]


def test_native_rejects_bad_arguments_without_launching():
    lib = _native.load()
    p = 4096  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails validation first

    def bad(rc, word):
        assert rc == -1 and word in lib.fr_last_error(), (rc, lib.fr_last_error())
    assert lib.fr_densify_workspace_bytes(0) == 0 and lib.fr_densify_workspace_bytes(-3) == 0
    assert lib.fr_densify_workspace_bytes(6_000_000) % 16 == 0 and 6_000_000 <= lib.fr_densify_workspace_bytes(6_000_000) < 6_200_000
    bad(lib.fr_densify_stats(-1, p, p, p, p, None), b"P=-1")
    bad(lib.fr_densify_stats(10, p, None, p, p, None), b"null")
    assert lib.fr_densify_stats(0, None, None, None, None, None) == 0
    bad(lib.fr_densify_plan(None, None), b"null")
    a = _native.DensifyPlanArgs()
    a.P, a.mode, a.N = -1, 0, 2
    bad(lib.fr_densify_plan(C.byref(a), None), b"P=-1")
    a.P, a.mode = 10, 5
    bad(lib.fr_densify_plan(C.byref(a), None), b"mode")
    for n in (0, 5):
        a.mode, a.N = 0, n
        bad(lib.fr_densify_plan(C.byref(a), None), b"1..4")
    a.N = 2
    bad(lib.fr_densify_plan(C.byref(a), None), b"null")      # no counts, no workspace
    a.counts_out, a.workspace = p, p + 4
    bad(lib.fr_densify_plan(C.byref(a), None), b"aligned")
    a.workspace = p
    bad(lib.fr_densify_plan(C.byref(a), None), b"mask")
    a.mode, a.n_grad, a.scaling, a.accum = _native.DENSIFY_SPLIT_GRAD, 11, p, p
    bad(lib.fr_densify_plan(C.byref(a), None), b"n_grad")
    a.mode, a.n_grad = _native.DENSIFY_AND_PRUNE, 9
    bad(lib.fr_densify_plan(C.byref(a), None), b"densify_and_prune needs")
    a.P = 0
    assert lib.fr_densify_plan(C.byref(a), None) == 0        # nothing launched
    bad(lib.fr_densify_rows(None, None), b"null")
    r = _native.DensifyRowsArgs()
    r.P, r.N, r.num_tensors = 10, 2, _native.COMPACT_MAX_TENSORS + 1
    bad(lib.fr_densify_rows(C.byref(r), None), b"tensors")
    r.num_tensors, r.n_keep = 1, 11
    bad(lib.fr_densify_rows(C.byref(r), None), b"bad counts")
    r.n_keep, r.n_split, r.n_child = 5, 2, 3
    bad(lib.fr_densify_rows(C.byref(r), None), b"bad counts")
    r.n_child = 2
    bad(lib.fr_densify_rows(C.byref(r), None), b"workspace")
    r.workspace = p
    r.tensors[0].row_words, r.tensors[0].role = 3, 4
    bad(lib.fr_densify_rows(C.byref(r), None), b"role")
    r.tensors[0].role = _native.DENSIFY_XYZ
    bad(lib.fr_densify_rows(C.byref(r), None), b"null")      # no data pointers
    r.tensors[0].src, r.tensors[0].dst = p, p
    bad(lib.fr_densify_rows(C.byref(r), None), b"needs scaling")
    r.tensors[0].row_words, r.scaling, r.rotation, r.noise = 4, p, p, p
    bad(lib.fr_densify_rows(C.byref(r), None), b"3 words")
    r.N = 5
    bad(lib.fr_densify_rows(C.byref(r), None), b"1..4")
    r.N, r.n_keep, r.n_split, r.n_child = 2, 0, 0, 0
    assert lib.fr_densify_rows(C.byref(r), None) == 0        # no output rows: nothing launched
    r.P = 0
    assert lib.fr_densify_rows(C.byref(r), None) == 0


def _compare(a, b, n_fixed, what):
    """Everything bit for bit, except the children's xyz and scaling (rows n_fixed ..), which are compared with allclose."""
    sa, sb = prune_ref.state_tensors(a), prune_ref.state_tensors(b)
    assert sa.keys() == sb.keys(), (what, sorted(sa), sorted(sb))
    for k in sa:
        if k in ("xyz", "scaling"):
            assert sa[k].shape == sb[k].shape, (what, k)
            assert prune_ref.same_bits(sa[k][:n_fixed], sb[k][:n_fixed]), (what, k)
            assert torch.allclose(sa[k][n_fixed:], sb[k][n_fixed:], rtol=1e-6, atol=1e-7), (what, k)
        else:
            assert prune_ref.same_bits(sa[k], sb[k]), f"{what} {k}: {tuple(sa[k].shape)} vs {tuple(sb[k].shape)}"


@pytest.mark.parametrize("N", (2, 3))
@pytest.mark.parametrize("P", (1, 64, 5000))
def test_the_literal_sequence_equals_the_per_row_plan(P, N):
    for max_screen_size in (20, None):
        base = cpu_model(P, seed=P)
        assert densify_ref.open_gaps(base, (PERCENT_DENSE * EXTENT, 0.1 * EXTENT), MIN_OPACITY) == 0
        lit, plan = prune_ref.clone_model(base), prune_ref.clone_model(base)
        split = densify_ref.plan_classes(base, MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size, N)[2]
        noise = torch.randn(N * int(split.sum()), 3, generator=torch.Generator().manual_seed(7))
        n_clone_all, n_split = densify_ref.densify_and_prune(lit, MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size, N, noise)
        n_keep, n_clone, n_split2, n_child = densify_ref.densify_and_prune_plan(plan, MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size, N, noise)
        assert n_split == n_split2 and n_clone <= n_clone_all and n_child <= n_split
        assert len(lit) == len(plan) == n_keep + n_clone + N * n_child
        _compare(lit, plan, n_keep + n_clone, f"P={P} N={N} max_screen_size={max_screen_size}")
        for m in (lit, plan):
            for name in NAMES:
                p = getattr(m, ATTRS[name])
                st = m.optimizer.state[p]
                assert float(st["step"]) == 2 and not st["exp_avg"][n_keep:].any() and not st["exp_avg_sq"][n_keep:].any()
            assert not m.xyz_gradient_accum.any() and not m.denom.any() and not m.max_radii2D.any()
        if P == 5000:  # every class occurs, and the world-size test cuts parents and children when it is on
            keep, clone, split, child = densify_ref.plan_classes(base, MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size, N)
            assert min(int(keep.sum()), n_clone, n_child) > 100 and n_child < n_split and n_clone < n_clone_all
            neg = (base.xyz_gradient_accum.reshape(-1) < 0) & (base.denom.reshape(-1) > 0)
            assert (clone & neg).any() and not (split & neg).any()  # |g| clones, signed g never splits
            if max_screen_size:
                free = densify_ref.plan_classes(base, MAX_GRAD, MIN_OPACITY, EXTENT, None, N)
                assert int(free[0].sum()) > int(keep.sum()) and int(free[3].sum()) > n_child


def test_densify_has_no_cpu_fallback_and_validates_arguments():
    P = 10
    model = cpu_model(P)
    before = {k: v.clone() for k, v in prune_ref.state_tensors(model).items()}
    mask = torch.zeros(P, dtype=torch.bool)
    grads = torch.zeros(P, 1)
    calls = (lambda: densify.clone_rows(model, mask), lambda: densify.split_rows(model, mask),
             lambda: densify.idx_densify_and_split(model, mask), lambda: densify.position_grad_densify(model, 0.1),
             lambda: densify.scale_densify_and_split(model, 1.0, 0.1), lambda: densify.densify_and_split_big_size(model, 0.1),
             lambda: densify.densify_and_clone(model, grads, 0.1, 1.0), lambda: densify.densify_and_split(model, grads, 0.1, 1.0),
             lambda: densify.densify_and_prune(model, 0.1, 0.005, 1.0, 20),
             lambda: densify.add_densification_stats(model, torch.zeros(P, 3), mask))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad_mask in (torch.zeros(P + 1, dtype=torch.bool), torch.zeros(P, 2, dtype=torch.bool), torch.zeros(0, dtype=torch.bool)):
        for fn in (densify.clone_rows, densify.split_rows, densify.idx_densify_and_split):
            with pytest.raises(ValueError, match="mask"):
                fn(model, bad_mask)
        with pytest.raises(ValueError, match="mask"):
            densify.add_densification_stats(model, torch.zeros(P, 3), bad_mask)
    for n in (0, 5, -1):
        with pytest.raises(ValueError, match="1..4"):
            densify.split_rows(model, mask, N=n)
        with pytest.raises(ValueError, match="1..4"):
            densify.densify_and_prune(model, 0.1, 0.005, 1.0, 20, N=n)
        with pytest.raises(ValueError, match="1..4"):
            densify.scale_densify_and_split(model, 1.0, 0.1, N=n)
    with pytest.raises(ValueError, match="grads"):
        densify.densify_and_split(model, torch.zeros(P + 1), 0.1, 1.0)
    with pytest.raises(ValueError, match="grads"):
        densify.densify_and_clone(model, torch.zeros(P - 1), 0.1, 1.0)
    with pytest.raises(ValueError, match="gradient"):
        densify.add_densification_stats(model, torch.zeros(P + 1, 3), mask)
    after = prune_ref.state_tensors(model)
    assert all(prune_ref.same_bits(before[k], after[k]) for k in before)
