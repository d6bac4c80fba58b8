"""The foveated renderer's FULL backward pass without a GPU: the C ABI (new symbols only; every pinned struct keeps its size; refusals by
field name before anything is enqueued) and the conditions the GPU half (tests/test_fov_full_backward_gpu.py) relies on, asserted on
the reference alone (tests/fov_full_backward_ref.py): its image is the oracle's, its per-level gradients are FovBackwardRef's (two
derivations of one number), its float32 flavour stays within what the comparison allows against its float64 flavour on every scene
and tensor, and every scene's census holds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fov3dgs_amd import _native
from tests import fov_backward_scenes as fs
from tests import fov_full_backward_ref as F
from tests.checks import check_image
from tests.helpers import ROOT

NEW_SYMBOLS = ("fr_forward_begin_fov_keep_full", "fr_forward_fov_keep_full_call", "fr_geometry_bytes_fov_keep_full", "fr_backward_fov")
HEADER = os.path.join(ROOT, "include", "fovraster.h")
# sizeof of the structs existing callers were compiled against (ABI 12)
PINNED = {"fr_fov_state": 64, "fr_backward_fov_args": 80, "fr_forward_args": 352, "fr_forward_ext": 16, "fr_foveation": 28, "fr_backward_args": 320}
# live Gaussians of every scene of the GPU half (counted here; asserted below)
LIVE = {"faint": 2352, "deep": 6387, "faint-L2": 2527, "close-wide-x2.5-fov": 984, "tiny-17x15": 2494, "tiny-8x8": 1206, "tiny-15x1": 711}


# ---- (a) ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_new_symbols_and_every_pinned_struct_keeps_its_size(tmp_path):
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTS and name in _native.FOV_FULL_BACKWARD_EXPORTS and hasattr(lib, name), name
    assert _native.has_fov_full_backward(lib)
    assert lib.fr_abi_version() == 12 == _native.ABI_VERSION
    cls = _native.BackwardFovFullArgs
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"',
            'int (*bwd)(const fr_backward_fov_full_args *) = fr_backward_fov;',
            'int (*fwd)(fr_forward_args *, const fr_forward_ext *, const fr_foveation *, fr_fov_state *) = fr_forward_fov_keep_full_call;',
            'int (*beg)(fr_forward_args *, const fr_forward_ext *, const fr_foveation *, fr_fov_state *, fr_frame **) = fr_forward_begin_fov_keep_full;',
            'size_t (*siz)(int32_t, int32_t) = fr_geometry_bytes_fov_keep_full;',
            'int main(void){', 'printf("%d %d\\n", FR_ABI_VERSION, FR_FOV_STATE_FULL);']
    body += [f'printf("%zu\\n", sizeof({name}));' for name in PINNED]
    body.append('printf("%zu\\n", sizeof(fr_backward_fov_full_args));')
    body += [f'printf("%zu\\n", offsetof(fr_backward_fov_full_args, {f[0]}));' for f in cls._fields_]
    body.append('return 0;}')
    src = tmp_path / "layout_fov_full.c"
    src.write_text("\n".join(body))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-o", str(tmp_path / "decl.o"), str(src)])  # the declared signatures
    src.write_text("\n".join(ln for ln in body if "= fr_" not in ln))  # (sizes from a program that does not reference the library)
    exe = tmp_path / "layout_fov_full"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert nums[:2] == [12, _native.FOV_STATE_FULL]
    assert nums[2:2 + len(PINNED)] == list(PINNED.values())
    for name, c in (("fr_fov_state", _native.FovState), ("fr_backward_fov_args", _native.BackwardFovArgs), ("fr_forward_args", _native.ForwardArgs),
                    ("fr_forward_ext", _native.ForwardExt), ("fr_foveation", _native.Foveation), ("fr_backward_args", _native.BackwardArgs)):
        assert C.sizeof(c) == PINNED[name], name
    k = 2 + len(PINNED)
    assert nums[k] == C.sizeof(cls)
    for f, off in zip(cls._fields_, nums[k + 1:]):
        assert getattr(cls, f[0]).offset == off, f[0]


def test_the_larger_workspace_lies_behind_the_keep_layout():
    lib = _native.load()
    for P, L in ((0, 4), (1, 2), (3000, 4), (6_000_000, 3)):
        keep, full = lib.fr_geometry_bytes_fov_keep(P, L), lib.fr_geometry_bytes_fov_keep_full(P, L)
        assert full >= keep + 32 * P and full - keep <= 32 * P + 1024, (P, L)
    assert lib.fr_geometry_bytes_fov_keep_full(10, 5) == 0 and "levels" in _native.last_error()


def _state(variant=3 | _native.FOV_STATE_FULL, levels=4):
    st = _native.FovState()
    st.size, st.variant, st.P, st.W, st.H, st.levels, st.num_rendered, st.num_items = C.sizeof(_native.FovState), variant, 5, 32, 32, levels, 7, 4
    st.geometry = st.binning = st.image = 4096
    return st


def _args(st):
    a = _native.BackwardFovFullArgs()
    a.size, a.state = C.sizeof(_native.BackwardFovFullArgs), C.pointer(st)
    a.P, a.M, a.sh_degree, a.tanfovx, a.tanfovy, a.scale_modifier = 5, 16, 3, 0.5, 0.5, 1.0
    for f, _ in _native.BackwardFovFullArgs._fields_:
        if f.startswith("dL_") or f in ("means3D", "scales", "rotations", "shs_rest", "viewmatrix", "projmatrix", "campos", "background"):
            setattr(a, f, 4096)   # (never dereferenced: every call below is refused before anything is enqueued)
    return a


REQUIRED = ("means3D", "scales", "rotations", "shs_rest", "viewmatrix", "projmatrix", "campos", "background", "dL_dpix", "dL_dopacities",
            "dL_dshs_dcs", "dL_dshs_rest", "dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dmeans2D")


def test_refusals_name_the_field_before_anything_is_enqueued():
    lib = _native.load()

    def refused(a, word):
        assert lib.fr_backward_fov(C.byref(a)) == -1   # FR_ERR_INVALID
        assert word in _native.last_error(), (word, _native.last_error())
    st = _state()
    for f in REQUIRED:
        a = _args(st)
        setattr(a, f, None)
        refused(a, f)
    a = _args(st)
    a.state = None
    refused(a, "state")
    refused(_args(_state(variant=3)), "FR_FOV_STATE_FULL")                      # a plain keep state: no rows of moments
    refused(_args(_state(variant=1 | _native.FOV_STATE_FULL)), "variant")       # another variant
    refused(_args(_state(levels=5)), "levels")
    a = _args(st)
    a.P = 6
    refused(a, "P is")
    a = _args(st)
    a.size = 8
    refused(a, "size")
    # ... and the appearance pass refuses a _full state (documented in include/fovraster.h)
    b = _native.BackwardFovArgs()
    b.size, b.state = C.sizeof(_native.BackwardFovArgs), C.pointer(st)
    b.background = b.dL_dpix = b.dL_dopacities = b.dL_dshs_dcs = 4096
    assert lib.fr_backward_fov_appearance(C.byref(b)) != 0 and "variant" in _native.last_error()


def _set(**fields):
    def change(st):
        for k, v in fields.items():
            setattr(st, k, v)
    return change


# every malformed state either entry point refuses -> the field its message names
MALFORMED = (("short size", _set(size=8), "fr_fov_state.size"), ("wrong variant", None, "variant"), ("levels 1", _set(levels=1), "levels"),
             ("levels 5", _set(levels=5), "levels"), ("W = 0", _set(W=0), "W=0"), ("W < 0", _set(W=-16), "W=-16"), ("H = 0", _set(H=0), "H=0"),
             ("H < 0", _set(H=-16), "H=-16"), ("num_rendered < 0", _set(num_rendered=-1), "num_rendered=-1"),
             ("num_items > 4 T", _set(num_items=4 * 4 + 1), "num_items=17"), ("null geometry", _set(geometry=None), "geometry"),
             ("null image", _set(image=None), "image"), ("null binning", _set(binning=None), "binning"))


def test_both_backward_entry_points_refuse_the_same_malformed_states():
    """fr_backward_fov_appearance and fr_backward_fov check the state they are handed with one validator: a state one of them refuses
    for its sizes, variant, levels or workspaces is refused by the other, FR_ERR_INVALID, with the same field named."""
    lib = _native.load()

    def appearance(st):
        b = _native.BackwardFovArgs()
        b.size, b.state = C.sizeof(_native.BackwardFovArgs), None if st is None else C.pointer(st)
        b.background = b.dL_dpix = b.dL_dopacities = b.dL_dshs_dcs = 4096
        return lib.fr_backward_fov_appearance(C.byref(b))

    def full(st):
        a = _args(st if st is not None else _state())
        if st is None:
            a.state = None
        return lib.fr_backward_fov(C.byref(a))
    for entry, own in ((appearance, 3), (full, 3 | _native.FOV_STATE_FULL)):
        assert entry(None) == -1 and "state" in _native.last_error(), entry.__name__
        for what, change, field in MALFORMED:
            st = _state(variant=own)
            if change is None:
                st.variant = 1 | (own & _native.FOV_STATE_FULL)
            else:
                change(st)
            assert entry(st) == -1, (entry.__name__, what)   # FR_ERR_INVALID
            assert field in _native.last_error(), (entry.__name__, what, _native.last_error())


def test_the_full_forward_refuses_what_the_keep_forward_refuses():
    from tests.test_fov_backward_cpu import _forward_args
    lib = _native.load()
    st = _native.FovState()
    st.size = C.sizeof(_native.FovState)
    a, cb = _forward_args()
    a.packed_geom = 4096
    assert lib.fr_forward_fov_keep_full_call(C.byref(a), None, None, C.byref(st)) != 0 and "packed" in _native.last_error()
    a, cb = _forward_args()
    fov = _native.Foveation(C.sizeof(_native.Foveation), 5, 12.0, 2.0, 1.0, 0.5, 0.5)
    assert lib.fr_forward_fov_keep_full_call(C.byref(a), None, C.byref(fov), C.byref(st)) != 0 and "levels" in _native.last_error()
    a, cb = _forward_args(variant=1)
    assert lib.fr_forward_fov_keep_full_call(C.byref(a), None, None, C.byref(st)) != 0 and "variant" in _native.last_error()


# ---- (b) - (e) the reference -----------------------------------------------------------------------------------------------------------
SCENES = tuple(F.LARGE) + F.TINY + F.SHORT_NAMES


@pytest.mark.parametrize("name", SCENES)
def test_reference_image_gradients_noise_and_census(name):
    """(b) the reference's float64 image is the forward's within check_image; (c) its dL_dopacities / dL_dshs_dcs / dL_dlevel_colours
    equal FovBackwardRef's float64 gradients within F64_AGREEMENT of the tensor's largest entry; (d) its float32 flavour passes the
    GPU half's comparison against its float64 flavour (judged as `got`: the allowance is the same arithmetic's own share times 1.5);
    (e) the census: the live Gaussians counted when the scene was chosen, MIN_LIVE / MIN_BRANCH on the large scenes."""
    r = F.reference(name)
    check_image(r["full"].image(np.float64).astype(np.float32), r["fwd"]["color"], name=f"{name} reference image")
    want, mine = r["ref"].backward(r["dpix"]), r["full"].level_gradients_on(r["fwd"], r["dpix"])
    for k in F.LEVELLED:
        scale = float(np.abs(want[k]).max())
        worst = float(np.abs(mine[k] - want[k]).max())
        print(f"{name} {k}: autograd vs hand-written sums, float64: {worst / max(scale, 1e-300):.2e} of the largest entry")
        assert worst <= F.F64_AGREEMENT * scale, (name, k, worst, scale)
    cen, lcen = r["census"], r["level_census"]
    live = int(cen["live"].sum())
    print(f"{name}: census", {k: int(v.sum()) for k, v in cen.items()})
    F.record_census(name, cen)
    if name in LIVE:
        assert live == LIVE[name], (name, live)
    if name in F.LARGE:
        assert live >= F.MIN_LIVE
        for br in F.LARGE[name]:
            assert int(cen[br].sum()) >= F.MIN_BRANCH, (name, br, int(cen[br].sum()))
        F.judge(r["g32"], r["g32"], r["g64"], cen, lcen, f"{name} float32 reference", r["L"], branches=F.LARGE[name])
    elif name in F.TINY:
        F.judge(r["g32"], r["g32"], r["g64"], cen, lcen, f"{name} float32 reference", r["L"], min_rows=min(live, int(lcen["live"].sum())))
    else:
        P = int(name.split("-")[1])
        assert 1 <= live <= P
        for k in F.GEOMETRY + F.LEVELLED:
            from tests.checks import grad_stats
            x32, x64 = np.asarray(r["g32"][k]), np.asarray(r["g64"][k])
            st = grad_stats(x32.reshape(len(x32), -1), x64.reshape(len(x64), -1), rtol=F.SHORT_RTOL)
            print(f"{name} {k}: float32 reference worst row {st['row_rel_max']:.2e}")
            assert st["frac_bad"] == 0.0, (name, k, st["row_rel_max"])


@pytest.mark.parametrize("name", F.NOTHING)
def test_a_frame_that_renders_nothing_has_a_zero_reference(name):
    r = F.reference(name)
    assert r["fwd"]["num_rendered"] == 0 and not r["census"]["live"].any()
    for k in F.GEOMETRY + F.LEVELLED:
        assert not np.asarray(r["g64"][k]).any(), k


@pytest.mark.parametrize("deg", F.DEGREES)
def test_coefficients_above_the_degree_get_exact_zeros_in_the_reference(deg):
    r = F.reference("faint", deg)
    g = np.asarray(r["g64"]["dL_dshs_rest"])
    n = (deg + 1) ** 2 - 1
    assert not g[:, n:].any() and (deg == 0 or g[:, :n].any())
    assert int(r["census"]["live"].sum()) >= F.MIN_LIVE


def test_the_comparison_rejects_a_defect_in_the_moments():
    """judge() is not vacuous: the float32 reference with the geometry gradients of the two-level Gaussians scaled by 1 + 3e-4 (an
    opacity factor applied slightly wrong in one state) is rejected on that branch."""
    r = F.reference("faint")
    bad = {k: np.array(v) for k, v in r["g32"].items()}
    sel = r["census"]["two_level"]
    bad["dL_dmeans3D"][sel] *= np.float32(1.0003)
    with pytest.raises(AssertionError):
        F.judge(bad, r["g32"], r["g64"], r["census"], r["level_census"], "doctored", r["L"], branches=F.LARGE["faint"])
