"""The head kernels' geometry for frames that share the GPU (fr_forward_args.no_helper_streams bit 1; csrc/preprocess.hip:
launch_project keeps fewer k_project workgroups resident, launch_bin smaller k_bin workgroups whose slabs k_emit replays through
EmitArgs::bin_bw). Nothing a frame leaves may depend on it: the cull pass lists its survivors in index order whatever the wave
count, the tile lists are sorted on (depth bits, item), every tile is cleared or stored by somebody. So the same call with the flag
0, 1 and 3 must leave the same radii, visibility, ranges, tile lists, level rows and image, bit for bit."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import cam_dict, scene_dict, small_camera, small_case, small_cloud, syn
from tests.checks import check_image
from oracle import oracle as orc

gpu = pytest.mark.gpu

FOV = "fov_pcheck_obb"
BG = (0.3, 0.6, 0.9)
NAN = float("nan")
GAZES = ((0.5, 0.5), (0.05, 0.95), (0.25, 0.75))
FLAGS = (0, 1, 3)
ITEM_NONE = 0xffffffff
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_gpu():
    if not torch.cuda.is_available():  # only reached by an explicit -m gpu run (tests/conftest.py skips otherwise)
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _frame(variant, scene, cam, flag, **kw):
    """tests/abi_forward.abi_forward with fr_forward_args.no_helper_streams = flag -> everything the frame left, as device tensors:
    color, radii, visibility, num_rendered, vis_list (the cull pass's survivors), ranges, items (the tile lists), and for the foveated
    variant level_ranges and the level rows of the items that landed in a tile (the rows of the others are never written)."""
    from fov3dgs_amd import _native
    from tests import abi_forward as af
    from tests.gpu_helpers import _view, vis_list_of

    def args():
        a = real()
        a.no_helper_streams = flag
        return a
    lib, vid = _native.load(), _native.VARIANT_IDS[variant]  # (loaded before the struct's name stands for a function)
    real = _native.ForwardArgs
    _native.ForwardArgs = args
    try:
        out = af.abi_forward(variant, scene, cam, visibility_fill=0xFF, **kw)
    finally:
        _native.ForwardArgs = real
    P, W, H = int(out["radii"].numel()), int(cam["image_width"]), int(cam["image_height"])
    T = ((W + 15) // 16) * ((H + 15) // 16)
    geom, binb, img = out["_ws"].buf
    D = out["num_rendered"]
    st = {k: out[k] for k in ("color", "radii", "visibility", "num_rendered")}
    st["vis_list"] = vis_list_of(lib, vid, P, geom)
    st["ranges"] = _view(img, lib.fr_image_ranges(vid, W, H, img.data_ptr()), 2 * T, torch.int32).clone()
    st["items"] = (_view(binb, lib.fr_binning_point_list(vid, D, binb.data_ptr()), D, torch.int32).clone() if D > 0
                   else torch.zeros(0, dtype=torch.int32, device=img.device))
    if variant == FOV:
        n = int(st["vis_list"].numel())
        lr = _view(geom, lib.fr_geometry_level_ranges(P, geom.data_ptr()), P, torch.int32)[:n].clone()
        rows = _view(geom, lib.fr_geometry_level_colours(P, geom.data_ptr()), 16 * P, torch.float32).view(P, 16)[:n]
        st["level_ranges"] = lr
        st["level_rows"] = rows[(lr.long() & 0xffffffff) != ITEM_NONE].clone()
        st["tile_blend"] = out["tile_blend"]
    st["_keep"] = out
    return st


def _same(a, b, what):
    for k in a:
        if k.startswith("_"):
            continue
        if isinstance(a[k], torch.Tensor):
            # (level rows: compared as bits -- a NaN colour would be equal to itself)
            x, y = (a[k].view(torch.int32), b[k].view(torch.int32)) if a[k].dtype == torch.float32 else (a[k], b[k])
            assert x.shape == y.shape and torch.equal(x, y), (what, k)
        else:
            assert a[k] == b[k], (what, k)


def _flags_agree(variant, scene, cam, want=None, **kw):
    got = {f: _frame(variant, scene, cam, f, **kw) for f in FLAGS}
    for fa, fb in ((0, 1), (1, 3), (0, 3)):
        _same(got[fa], got[fb], f"flags {fa} / {fb}")
    vis = got[3]["visibility"]
    assert torch.equal(vis, (got[3]["radii"] > 0).to(torch.uint8))
    if want is not None:
        assert got[3]["num_rendered"] == want["num_rendered"]
        check_image(got[3]["color"].cpu().numpy(), want["color"], name=f"{variant} shared geometry")
    return got[3]


@functools.lru_cache(maxsize=None)
def _case(variant, P, W, H, gaze):
    scene, cam = small_case(variant, P=P, seed=3, bg=BG, gaze=gaze, width=W, height=H)
    return scene, cam, orc.forward(variant, scene, cam)


# ---- no GPU needed -------------------------------------------------------------------------------------------------------------------
def test_abi_is_unchanged():
    """The flag's second bit is a value of an existing field: ABI 12, the structs' sizes and the field's place stay"""
    from fov3dgs_amd import _native
    header = open(os.path.join(ROOT, "include", "fovraster.h")).read()
    assert re.search(r"#define\s+FR_ABI_VERSION\s+12\b", header)
    assert re.search(r"FR_FRAME_NO_HELPER_STREAMS\s*=\s*1\b", header) and re.search(r"FR_FRAME_SHARES_GPU\s*=\s*2\b", header)
    assert _native.load().fr_abi_version() == 12
    assert C.sizeof(_native.ForwardArgs) == 352 and C.sizeof(_native.ForwardExt) == 16  # (LP64, as before the flag had a second bit)
    assert _native.ForwardArgs.no_helper_streams.offset == 344 and _native.ForwardArgs.no_helper_streams.size == 4


# ---- flag equality -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("P", (1, 37, 1037, 20000))
@pytest.mark.parametrize("gaze", GAZES)
@pytest.mark.parametrize("W,H", ((203, 131), (640, 360)))
def test_flags_leave_the_same_frame(W, H, gaze, P):
    """P = 1, 37, 1037: fewer Gaussians than waves (waves without a chunk, without a slab), no multiple of 64; 20 000: a wave of
    the smaller k_bin workgroups takes more than one slab. Both layouts: the model's tensors (candidate rows) and the packed model."""
    _need_gpu()
    scene, cam, want = _case(FOV, P, W, H, gaze)
    a = _flags_agree(FOV, scene, cam, want)
    b = _flags_agree(FOV, scene, cam, want, packed=True)
    assert a["num_rendered"] == b["num_rendered"] and torch.equal(a["radii"], b["radii"])


@gpu
@pytest.mark.parametrize("P", (37, 20000))
def test_plain_cull_variant(P):
    """pcheck_obb: k_project's other instantiation takes the shared grid too (k_bin keeps its workgroups: the smaller ones are the
    foveated frames')"""
    _need_gpu()
    scene, cam, want = _case("pcheck_obb", P, 203, 131, (0.5, 0.5))
    _flags_agree("pcheck_obb", scene, cam, want)


@functools.lru_cache(maxsize=None)
def _large():
    """400 000 Gaussians at 640 x 360: more 1024-Gaussian pieces (391) than k_project keeps workgroups resident in either geometry
    -- the shared grid is a part of the lone one --, and about two (twelve waves) or three (eight) slabs for every wave of k_bin's
    full grid of 256 workgroups"""
    return small_case(FOV, P=400_000, seed=5, bg=BG, gaze=(0.25, 0.75), width=640, height=360)


@gpu
@pytest.mark.parametrize("packed", (False, True))
def test_large_cloud_on_the_capped_grids(packed):
    _need_gpu()
    scene, cam = _large()
    got = _flags_agree(FOV, scene, cam, packed=packed)
    assert got["vis_list"].numel() > 256 * 12 * 64 + 256 * 8 * 64  # (every wave has a slab, and a second one in most, under both sizes)


@gpu
def test_walk_paths():
    """A frame-filling splat (walked by the whole workgroup after the slab loop: the stride is the workgroup's thread count, the
    waves' share of s_gitem its wave count) and splats of a few hundred tiles (walked by a whole wave)"""
    _need_gpu()
    from tests.abi_forward import BIG, GIANT, visibility_case
    for P in (37, 1037):
        scene, cam = visibility_case(FOV, P)
        scene["scales"][20:24] = (0.3, 0.35, 0.3)  # (some more whole-wave splats)
        want = orc.forward(FOV, scene, cam)
        got = _flags_agree(FOV, scene, cam, want)
        r = got["radii"].cpu().numpy()
        assert r[GIANT] * 2 > max(cam["image_width"], cam["image_height"]) and r[BIG] > 32
        n = (got["ranges"].view(-1, 2)[:, 1] - got["ranges"].view(-1, 2)[:, 0]).cpu().numpy()
        assert (n > 0).sum() >= 1024  # the giant splat lands in a workgroup-wide walk's worth of tiles (FR_GIANT_TNUM)


# ---- tile clear ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", ("one workgroup", "half the resident count", "the capped grid"))
def test_two_level_tiles_are_cleared(which):
    """The shared geometry's k_project clears the two-level tiles of a NaN-filled image: P = 40 (one workgroup for all 920 tiles of
    640 x 360), P = 131 072 (128 workgroups, half of what a lone frame keeps resident on 256 CUs: 2048 waves for 920 tiles), and the
    large cloud on the shared geometry's capped grid"""
    _need_gpu()
    from tests.abi_forward import need_both_kinds_of_tiles
    if which == "the capped grid":
        scene, cam = _large()
    else:
        scene, cam = small_case(FOV, P=40 if which == "one workgroup" else 131072, seed=9, bg=BG, gaze=(0.5, 0.5), width=640, height=360)
    got = _frame(FOV, scene, cam, 3, image_fill=NAN)
    need_both_kinds_of_tiles(got)
    assert got["tile_blend"].numel() == 920
    zero = _frame(FOV, scene, cam, 3, image_fill=0.0)
    assert not bool(torch.isnan(got["color"]).any())
    _same(got, zero, "NaN / zero-filled image")
    _same(got, _frame(FOV, scene, cam, 0, image_fill=NAN), "flags 3 / 0 into NaN")


# ---- overlapped frames ---------------------------------------------------------------------------------------------------------------
@gpu
def test_overlapped_frames_equal_serial_frames():
    """Six successive render() calls (overlap on: every frame's flag is 3) at 20 000 / 640 x 360 into allocator blocks left full of
    NaN equal the serial path's frames (flag 1) bit for bit"""
    _need_gpu()
    from fov3dgs_amd import rasterizer as rz
    from fov3dgs_amd.gaussian_renderer_fov import render
    from tests.abi_forward import dirty_allocator
    dev, W, H = "cuda:0", 640, 360
    cpu = small_cloud(20000, 3)
    fov = syn.foveation_layers(cpu, seed=4)
    cloud, cam = cpu.to(dev), small_camera(W, H).to(dev)
    kw = dict(alpha=0.05, blending=True, highest_levels=fov[0].to(dev), shs_dcs=fov[1].to(dev), opacities=fov[2].to(dev))
    bg = torch.tensor(BG, device=dev)
    flags, begin = [], rz._begin_call

    def spy(lib, a, *rest):
        flags.append(int(a.no_helper_streams))
        return begin(lib, a, *rest)
    rz._begin_call = spy
    try:
        serial = []
        with torch.no_grad(), rz.serial_frames():
            for gaze in GAZES:
                out = render(cam, cloud, bg, gazeArray=gaze, **kw)
                serial.append((out["render"].clone(), out["radii"].clone()))
        torch.cuda.synchronize()
        assert set(flags) == {1}, flags
        assert not torch.equal(serial[0][0], serial[1][0]) and not torch.equal(serial[1][0], serial[2][0])
        assert rz.OVERLAP_SUCCESSIVE_FRAMES
        del flags[:]
        dirty_allocator(W, H)
        with torch.no_grad():
            got = []
            for i in range(6):
                out = render(cam, cloud, bg, gazeArray=GAZES[i % 3], **kw)
                got.append((out["render"].clone(), out["radii"].clone()))
                out["render"].fill_(NAN)
                del out
            torch.cuda.synchronize()
        assert set(flags) == {3}, flags
    finally:
        rz._begin_call = begin
    for i, (img, radii) in enumerate(got):
        assert torch.equal(img, serial[i % 3][0]) and torch.equal(radii, serial[i % 3][1]), i
