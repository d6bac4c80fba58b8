"""The foveated renderer's appearance backward pass without a GPU: the C ABI (new symbols beside the unchanged structs, refusals by
field name before anything is enqueued), the reference of the GPU tests validated on its own (tests/fov_backward_ref.py: its forward
image against the C oracle, its gradients against central finite differences in double with the decisions frozen), and the coverage
the GPU comparisons rely on, asserted on the reference alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import fov_backward_ref as R
from tests.checks import check_image
from tests.helpers import ROOT
from fov3dgs_amd import _native

NEW_SYMBOLS = ("fr_forward_begin_fov_keep", "fr_forward_fov_keep_call", "fr_geometry_bytes_fov_keep", "fr_image_bytes_fov_keep",
               "fr_image_fov_state_T", "fr_image_fov_state_n", "fr_backward_fov_appearance")
HEADER = os.path.join(ROOT, "include", "fovraster.h")


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_new_symbols_under_the_same_abi_version():
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTS and name in _native.FOV_BACKWARD_EXPORTS and hasattr(lib, name), name
    assert _native.has_fov_backward(lib)
    assert lib.fr_abi_version() == 12 == _native.ABI_VERSION


def test_header_compiles_as_c_and_the_new_structs_match_ctypes(tmp_path):
    structs = (("fr_fov_state", _native.FovState), ("fr_backward_fov_args", _native.BackwardFovArgs))
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"',
            'int (*bwd)(const fr_backward_fov_args *) = fr_backward_fov_appearance;',
            'int (*fwd)(fr_forward_args *, const fr_forward_ext *, const fr_foveation *, fr_fov_state *) = fr_forward_fov_keep_call;',
            'int (*beg)(fr_forward_args *, const fr_forward_ext *, const fr_foveation *, fr_fov_state *, fr_frame **) = fr_forward_begin_fov_keep;',
            'int main(void){', 'printf("%d\\n", FR_ABI_VERSION);']
    for cname, cls in structs:
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f[0]}));' for f in cls._fields_]
    # the structs existing tests pin keep their sizes
    body += ['printf("%zu %zu %zu %zu\\n", sizeof(fr_forward_args), sizeof(fr_forward_ext), sizeof(fr_foveation), sizeof(fr_backward_args));',
             'return 0;}']
    src = tmp_path / "layout_fov_bwd.c"
    src.write_text("\n".join(body))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-o", str(tmp_path / "decl.o"), str(src)])  # the declared signatures
    lines = [ln for ln in body if "= fr_" not in ln]  # (sizes from a program that does not reference the library: it runs anywhere)
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout_fov_bwd"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert nums[0] == 12
    k = 1
    for cname, cls in structs:
        assert nums[k] == C.sizeof(cls), cname
        for f, off in zip(cls._fields_, nums[k + 1:]):
            assert getattr(cls, f[0]).offset == off, (cname, f[0])
        k += 1 + len(cls._fields_)
    assert nums[k:] == [C.sizeof(_native.ForwardArgs), C.sizeof(_native.ForwardExt), C.sizeof(_native.Foveation), C.sizeof(_native.BackwardArgs)]


def _forward_args(variant=3, P=5):
    """fr_forward_args that pass validate_forward for the foveated variant (pointers are never dereferenced: the calls below are
    refused before anything is enqueued)."""
    a = _native.ForwardArgs()
    a.variant, a.P, a.W, a.H, a.M, a.D = variant, P, 32, 32, 15 if variant == 3 else 16, 3
    for f in ("out_color", "means3D", "opacities", "viewmatrix", "projmatrix", "campos", "background", "radii", "shs", "scales", "rotations"):
        setattr(a, f, 4096)
    if variant == 3:
        a.shs_dcs = a.highest_levels = 4096
    if variant == 1:
        a.gaussians_count = a.contributions = 4096
    cb = _native.RESIZE_FN(lambda user, n: None)
    a.geometry_resize = a.binning_resize = a.image_resize = cb
    return a, cb


def _state():
    st = _native.FovState()
    st.size = C.sizeof(_native.FovState)
    return st


def test_the_state_keeping_forward_refuses_by_field_name():
    lib = _native.load()
    err = lambda: lib.fr_last_error()
    # wrong variant
    a, cb = _forward_args(variant=1)
    st = _state()
    assert lib.fr_forward_fov_keep_call(C.byref(a), None, None, C.byref(st)) == -1 and b"variant" in err()
    # levels > 4 (5 .. 8 would need a second row of sums: the follow-up)
    a, cb = _forward_args()
    fov = _native.Foveation(C.sizeof(_native.Foveation), 5, 12.0, 2.0, 1.0, 0.5, 0.5)
    assert lib.fr_forward_fov_keep_call(C.byref(a), None, C.byref(fov), C.byref(st)) == -1 and b"levels" in err()
    handle = C.c_void_p()
    assert lib.fr_forward_begin_fov_keep(C.byref(a), None, C.byref(fov), C.byref(st), C.byref(handle)) == -1 and not handle.value and b"levels" in err()
    # a packed model
    for field in ("packed_geom", "packed_colour", "packed_cull"):
        a, cb = _forward_args()
        a.packed_geom = a.packed_colour = a.packed_cull = 4096
        assert lib.fr_forward_fov_keep_call(C.byref(a), None, None, C.byref(st)) == -1 and field.encode() in err(), field
    # a missing state / a state of a shorter struct
    a, cb = _forward_args()
    assert lib.fr_forward_fov_keep_call(C.byref(a), None, None, None) == -1 and b"state" in err()
    short = _native.FovState()
    short.size = 8
    assert lib.fr_forward_fov_keep_call(C.byref(a), None, None, C.byref(short)) == -1 and b"fr_fov_state.size" in err()
    # the existing size queries answer what they answered; the new ones are larger by the kept arrays
    P, W, H = 1000, 200, 120
    assert lib.fr_geometry_bytes_fov_keep(P, 4) >= lib.fr_geometry_bytes_fov(3, P, 4) + 64 * P
    assert lib.fr_geometry_bytes_fov(3, P, 4) == lib.fr_geometry_bytes(3, P)
    assert lib.fr_image_bytes_fov_keep(W, H) >= lib.fr_image_bytes(3, W, H) + 16 * W * H
    assert lib.fr_geometry_bytes_fov_keep(P, 5) == 0 and b"levels" in err()


def test_the_backward_entry_refuses_by_field_name():
    lib = _native.load()
    err = lambda: lib.fr_last_error()
    assert lib.fr_backward_fov_appearance(None) == -1

    def args(st):
        a = _native.BackwardFovArgs()
        a.size = C.sizeof(_native.BackwardFovArgs)
        a.state = C.pointer(st) if st is not None else None
        a.background = a.dL_dpix = a.dL_dopacities = a.dL_dshs_dcs = 4096
        return a

    def good_state():
        st = _state()
        st.variant, st.P, st.W, st.H, st.levels = 3, 5, 32, 32, 4
        st.geometry = st.image = st.binning = 4096
        return st
    short = args(good_state())
    short.size = 8
    assert lib.fr_backward_fov_appearance(C.byref(short)) == -1 and b"fr_backward_fov_args.size" in err()
    assert lib.fr_backward_fov_appearance(C.byref(args(None))) == -1 and b"state" in err()
    st = good_state()
    st.variant = 1
    assert lib.fr_backward_fov_appearance(C.byref(args(st))) == -1 and b"variant" in err()
    st = good_state()
    st.levels = 5
    assert lib.fr_backward_fov_appearance(C.byref(args(st))) == -1 and b"levels" in err()
    for field in ("dL_dpix", "background", "dL_dopacities", "dL_dshs_dcs"):
        st = good_state()
        a = args(st)
        setattr(a, field, None)
        assert lib.fr_backward_fov_appearance(C.byref(a)) == -1 and field.encode() in err(), field
    st = good_state()
    st.geometry = None
    assert lib.fr_backward_fov_appearance(C.byref(args(st))) == -1 and b"geometry" in err()
    st = good_state()
    st.num_items = 4 * 4 + 1  # more work items than four per tile: not a state the forward call wrote
    assert lib.fr_backward_fov_appearance(C.byref(args(st))) == -1 and b"num_items" in err()
    st = good_state()
    st.P = 0
    assert lib.fr_backward_fov_appearance(C.byref(args(st))) == 0  # nothing to do, as fr_backward


def test_python_refusals_need_no_gpu():
    """appearance_only refuses another input that requires grad (in the words of _check_appearance_only) and a packed model before
    anything reaches the library."""
    import torch
    from fov3dgs_amd.diff_gaussian_rasterization_fov_pcheck_obb import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(image_height=16, image_width=16, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3), scale_modifier=1.0,
                                       viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=3, campos=torch.zeros(3),
                                       prefiltered=False, debug=False)
    r = GaussianRasterizer(rs)
    P = 4
    kw = dict(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 4, requires_grad=True), shs_rest=torch.zeros(P, 15, 3),
              scales=torch.ones(P, 3), rotations=torch.zeros(P, 4), shs_dcs=torch.zeros(P, 4, 3), highest_levels=torch.zeros(P, 1),
              gazeArray=(0.5, 0.5), alpha=0.05)
    for name in ("means3D", "scales", "rotations", "shs_rest", "highest_levels"):
        bad = dict(kw)
        bad[name] = kw[name].clone().requires_grad_(True)
        with pytest.raises(ValueError, match="appearance_only: .*requires grad"):
            r(**bad, appearance_only=True)
    with pytest.raises(ValueError, match="packed"):
        r(**kw, packed=object(), appearance_only=True)


# ---- the reference validated on its own ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", R.PARITY, ids=lambda k: f"a{k['alpha']}-g{k['gaze'][0]}-{k['gaze'][1]}-w{k.get('width', 200)}")
def test_reference_image_matches_the_oracle_forward(kw):
    """(a) the reference's forward image -- the frozen decisions evaluated in double -- against orc.forward("fov_pcheck_obb", ...)"""
    scene, cam, fwd, ref, dL = R.case(**kw)
    check_image(ref.image().astype(np.float32), fwd["color"], name="reference image")
    # ... and the fp32 flavour of the same arithmetic
    check_image(ref.image(dtype=np.float32), fwd["color"], name="reference image fp32")
    n = int((ref.backward(dL)["dL_dopacities"] != 0).sum())
    print(kw, "rows with a gradient:", n)
    assert n >= (4 * R.MIN_ROWS_PER_LEVEL if kw is R.MAIN else R.MIN_ROWS_OTHER)


def test_reference_gradients_match_central_differences():
    """(b) loss = sum(dL_dpix * image), decisions frozen, opacities clipped to <= 0.98 so that the 0.99 saturation binds nowhere: the
    frozen function is linear in any single opacity or DC coefficient (a Gaussian is in a pixel's list at most once, the two states of
    a pixel use different levels), so a central difference is exact up to rounding: agreement to 1e-6 relative. >= 40 entries of each
    tensor, over all levels and both kinds of tile; entries whose gradient is below 1e-6 of the tensor's largest are not sampled (the
    difference of two sums of ~10^4 terms carries ~1e-13 / h absolute)."""
    scene, cam, fwd, ref, dL = R.case(**R.MAIN, mutate="clip98")
    assert ref.opac.max() <= np.float32(0.98)
    g = ref.backward(dL)
    rng = np.random.default_rng(5)
    h = 1e-2
    opac0, dcs0 = ref.opac.astype(np.float64), ref.dcs.astype(np.float64)

    def samples(grad, per_cell=7):
        """(Gaussian, level[, channel]) entries: per level and kind of tile, `per_cell` entries with a gradient worth the name"""
        big = np.abs(grad) >= 1e-6 * np.abs(grad).max()
        out = []
        for lev in range(4):
            for used in (ref.used_single & ~ref.used_blend, ref.used_blend):
                cand = np.argwhere(big[:, lev] & (used[:, lev] if grad.ndim == 2 else used[:, lev][:, None]))
                take = cand[rng.permutation(len(cand))[:per_cell]]
                out += [(int(c[0]), lev) + tuple(int(x) for x in c[1:]) for c in take]
        return out
    s_op, s_dc = samples(g["dL_dopacities"]), samples(g["dL_dshs_dcs"])
    assert len(s_op) >= 40 and len(s_dc) >= 40, (len(s_op), len(s_dc))
    assert {s[1] for s in s_op} == {0, 1, 2, 3} == {s[1] for s in s_dc}
    worst = 0.0
    for idx in s_op:
        tiles = ref.tiles_with(idx[0])
        hi, lo = opac0.copy(), opac0.copy()
        hi[idx] += h
        lo[idx] -= h
        fd = (ref.frozen_loss(dL, hi, dcs0, tiles) - ref.frozen_loss(dL, lo, dcs0, tiles)) / (2 * h)
        an = g["dL_dopacities"][idx]
        worst = max(worst, abs(fd - an) / abs(an))
        assert abs(fd - an) <= 1e-6 * abs(an), ("opacities", idx, fd, an)
    for idx in s_dc:
        tiles = ref.tiles_with(idx[0])
        hi, lo = dcs0.copy(), dcs0.copy()
        hi[idx] += h
        lo[idx] -= h
        fd = (ref.frozen_loss(dL, opac0, hi, tiles) - ref.frozen_loss(dL, opac0, lo, tiles)) / (2 * h)
        an = g["dL_dshs_dcs"][idx]
        worst = max(worst, abs(fd - an) / abs(an))
        assert abs(fd - an) <= 1e-6 * abs(an), ("shs_dcs", idx, fd, an)
    print("samples", len(s_op), len(s_dc), "worst relative difference", worst)


# ---- coverage, asserted on the reference alone -----------------------------------------------------------------------------------
def test_main_scene_covers_every_level_and_both_kinds_of_tile():
    scene, cam, fwd, ref, dL = R.case(**R.MAIN)
    g = ref.backward(dL)
    per_level = [int((g["dL_dopacities"][:, lev] != 0).sum()) for lev in range(4)]
    blend_tiles = sum(1 for t in ref.tiles if t["blend"])
    single = [sum(1 for t in ref.tiles if not t["blend"] and t["states"][0]["lev"] == lev) for lev in range(4)]
    longest = max(len(t["g"]) for t in ref.tiles)
    print("rows per level", per_level, "two-level tiles", blend_tiles, "single-level tiles per level", single, "longest list", longest)
    assert min(per_level) >= R.MIN_ROWS_PER_LEVEL, per_level
    assert blend_tiles >= R.MIN_BLEND_TILES
    assert min(single) >= 1 and longest > 64  # every level has tiles of its own; lists longer than one 64-entry batch
    # both states of two-level tiles carry gradients, the upper state's existence skip drops entries, and some state-1 pixels start finished
    assert (ref.used_blend.sum(axis=0) > 0).sum() >= 3
    started_finished = sum(int(((t["states"][0]["n_contrib"] == 0) & t["inside"] & (t["states"][1]["n_contrib"] > 0)).sum()) for t in ref.tiles if t["blend"])
    assert started_finished > 0
    # the variants of the scene the GPU tests use
    cl = R.case(**R.MAIN, mutate="clamp")[3]
    used = ref.used_single | ref.used_blend
    clamped = (np.nan_to_num(cl.colours, nan=1.0) == 0) & (cl.used_single | cl.used_blend)[..., None]
    share = clamped.sum() / (3 * (cl.used_single | cl.used_blend).sum())
    print("clamped share of the used channels", share)
    assert 0.25 <= share <= 0.6 and used.sum() >= 4 * R.MIN_ROWS_PER_LEVEL
    sat = R.case(**R.MAIN, mutate="sat")
    gs = sat[3].backward(sat[4])
    assert int(((sat[3].opac == 1.0) & (gs["dL_dopacities"] != 0)).sum()) >= 20  # saturated opacities that carry a gradient
