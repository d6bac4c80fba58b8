"""A forward call through the C ABI itself (include/fovraster.h: fr_forward / fr_forward_ext_call on a hand-filled
_native.ForwardArgs), with output buffers the TEST owns and pre-fills: what the library leaves unwritten stays visible."""
import ctypes as C

import numpy as np
import torch

from fov3dgs_amd import _native
from fov3dgs_amd.rasterizer import _Workspaces, pack_model

TENSORS = ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp", "shs_dcs", "highest_levels")
STATS = ("pcheck_obb_sum", "pcheck_obb_max", "pcheck_obb_loss_weighted_max_count")
LEVELS = ("fov_pcheck_obb", "naive_pcheck_obb", "mmfr_pcheck_obb")


def _t(x, dev):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(dev)


def dirty_allocator(W, H, dev="cuda:0", n=4):
    """Leave the caching allocator's free blocks of an image's size full of NaN (what torch.empty hands out next)."""
    for t in [torch.full((3, H, W), float("nan"), device=dev) for _ in range(n)]:
        del t
    torch.cuda.synchronize()


def abi_forward(variant, scene, cam, dev="cuda:0", image_fill=float("nan"), visibility_fill=None, packed=False, debug=0):
    """-> dict(color [3,H,W], radii [P], num_rendered, visibility (uint8 [P], when visibility_fill is given), tile_blend (bool [T],
    variants with tile levels)), all torch tensors on `dev`, after a device synchronisation.
    image_fill: what out_color holds before the call. visibility_fill: a byte -> the call goes through fr_forward_ext_call with
    a visibility buffer that holds it everywhere."""
    lib = _native.load()
    vid = _native.VARIANT_IDS[variant]
    tens = {k: _t(scene.get(k), dev) for k in TENSORS}
    small = {k: _t(cam[k], dev) for k in ("bg", "viewmatrix", "projmatrix", "campos")}
    P = int(tens["means3D"].shape[0])
    W, H = int(cam["image_width"]), int(cam["image_height"])
    a = _native.ForwardArgs()
    keep = [tens, small]
    a.variant, a.P, a.D = vid, P, int(cam["sh_degree"])
    a.M = 0 if tens["shs"] is None else int(tens["shs"].shape[1])
    a.W, a.H, a.prefiltered, a.debug = W, H, 0, int(debug)
    a.tanfovx, a.tanfovy, a.scale_modifier = float(cam["tanfovx"]), float(cam["tanfovy"]), float(cam.get("scale_modifier", 1.0))
    gaze = cam.get("gaze", (0.5, 0.5))
    a.gaze_x, a.gaze_y, a.alpha, a.cur_level = float(gaze[0]), float(gaze[1]), float(cam.get("alpha", 0.05)), float(cam.get("cur_level", 0.0))
    a.stream = torch.cuda.current_stream(dev).cuda_stream
    a.background, a.viewmatrix, a.projmatrix, a.campos = (small[k].data_ptr() for k in ("bg", "viewmatrix", "projmatrix", "campos"))
    for k in TENSORS:
        if tens[k] is not None and tens[k].numel() > 0:
            setattr(a, k, tens[k].data_ptr())
    color = torch.full((3, H, W), image_fill, dtype=torch.float32, device=dev)
    radii = torch.full((P,), -7, dtype=torch.int32, device=dev)
    a.out_color, a.radii = color.data_ptr(), radii.data_ptr() if P else None
    if variant in STATS:
        counts, contribs = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.float32, device=dev)
        a.gaussians_count, a.contributions = counts.data_ptr(), contribs.data_ptr()
        keep.append((counts, contribs))
    if variant == "pcheck_obb_loss_weighted_max_count":
        lm = _t(scene["loss_map"], dev)
        a.loss_map = lm.data_ptr()
        keep.append(lm)
    if packed:
        pk = pack_model(tens["means3D"], tens["scales"], tens["rotations"], tens["opacities"], shs=tens["shs"],
                        shs_dcs=tens["shs_dcs"], highest_levels=tens["highest_levels"])
        a.packed_geom, a.packed_colour, a.packed_cull = pk.geom.data_ptr(), pk.colour.data_ptr(), pk.cull.data_ptr()
        keep.append(pk)
    ws = _Workspaces(torch.device(dev))
    a.geometry_resize, a.binning_resize, a.image_resize = ws.cbs[0], ws.cbs[1], ws.cbs[2]
    out = {"color": color, "radii": radii, "_keep": keep, "_ws": ws}
    with torch.cuda.device(dev):
        if visibility_fill is None:
            rc = lib.fr_forward(C.byref(a))
        else:
            vis = torch.full((P,), int(visibility_fill), dtype=torch.uint8, device=dev)
            ext = _native.ForwardExt(C.sizeof(_native.ForwardExt), vis.data_ptr() if P else None)
            rc = lib.fr_forward_ext_call(C.byref(a), C.byref(ext))
            out["visibility"] = vis
        assert rc == 0, _native.last_error()
        torch.cuda.synchronize()
    out["num_rendered"] = int(a.num_rendered)
    if variant in LEVELS and P > 0:
        T = ((W + 15) // 16) * ((H + 15) // 16)
        img = ws.buf[2]
        off = lib.fr_image_tile_levels(W, H, img.data_ptr()) - img.data_ptr()
        assert 0 <= off and off + 20 * T <= img.numel()
        out["tile_blend"] = img[off:off + 20 * T].view(torch.float32).reshape(5, T)[4] != 0
        off = lib.fr_image_ranges(vid, W, H, img.data_ptr()) - img.data_ptr()
        assert 0 <= off and off + 8 * T <= img.numel()
        out["ranges"] = img[off:off + 8 * T].view(torch.int32).reshape(T, 2)
    return out


def need_both_kinds_of_tiles(out):
    """The frame has two-level tiles (their two level states are added into the image) AND single-level tiles (stored)."""
    tb = out["tile_blend"]
    assert bool(tb.any()) and bool((~tb).any()), f"{int(tb.sum())} two-level tiles of {tb.numel()}"


# ---- the clouds of tests/test_visibility_gpu.py ---------------------------------------------------------------------------------------
VIS_W, VIS_H = 768, 432  # 48 x 27 = 1296 tiles: room for a splat on the workgroup-wide path (>= 1024 tiles)
BEHIND, OFF_SCREEN, BIG, GIANT, FILTERED = slice(0, 5), slice(5, 10), 10, 11, slice(12, 18)


def visibility_case(variant, P, seed=31, gaze=(0.1, 0.9)):
    """small_case's cloud with rows 0..17 placed by hand: behind the camera, off screen, one splat of a few hundred tiles, one that
    covers the frame, and (foveated model) six small ones of highest level 0 at the centre of a frame whose gaze is in a corner --
    every tile they reach has a level above theirs."""
    from tests.helpers import small_case
    scene, cam = small_case(variant, P=P, seed=seed, bg=(0.3, 0.6, 0.9), gaze=gaze, width=VIS_W, height=VIS_H)
    vm = np.asarray(cam["viewmatrix"])
    right, fwd = vm[:3, 0], vm[:3, 2]
    m, s = scene["means3D"], scene["scales"]
    centre = np.array([0.0, 0.0, 4.0], np.float32)  # (what small_camera looks at)
    m[BEHIND] -= 12.0 * fwd
    m[OFF_SCREEN] += 15.0 * right
    m[BIG], s[BIG] = centre, (0.35, 0.3, 0.3)
    m[GIANT], s[GIANT] = centre + 0.5 * fwd, (6.0, 4.0, 5.0)
    scene["opacities"][GIANT] = 0.99
    m[FILTERED], s[FILTERED] = centre + np.linspace(-0.3, 0.3, 6, dtype=np.float32)[:, None] * right, 0.02
    if "highest_levels" in scene:
        scene["highest_levels"][[BIG, GIANT]] = 3.0
        scene["highest_levels"][FILTERED] = 0.0
    return scene, cam
