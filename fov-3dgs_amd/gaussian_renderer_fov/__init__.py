"""render() for the foveated rasterizer (reference: fov3dgs/gaussian_renderer_fov/__init__.py:19-105)."""
import contextlib
import math
import weakref

import torch

from ..diff_gaussian_rasterization_fov_pcheck_obb import FoveationSettings, GaussianRasterizationSettings, GaussianRasterizer  # noqa: F401
from .. import _native
from ..rasterizer import PackedModel, _forward_begin, depth_of, pack_model, serial_frames, visibility_of, zero_points_like


class _PackState:
    __slots__ = ("refs", "versions", "ptrs", "packed")

    def __init__(self, tensors):
        self.refs = [weakref.ref(t) for t in tensors]
        self.versions = [t._version for t in tensors]
        self.ptrs = [t.data_ptr() for t in tensors]  # `t.data = other` keeps the object and the version, not the storage
        self.packed = None

    def matches(self, tensors):
        return len(self.refs) == len(tensors) and all(
            r() is t and v == t._version and p == t.data_ptr() for r, v, p, t in zip(self.refs, self.versions, self.ptrs, tensors))


def invalidate_packed(pc):
    """Drop the packed copy render(packed="auto") cached on the model `pc` (after a write the autograd version
    counters cannot see: `.data` writes, raw-pointer kernels, DLPack aliases)."""
    if getattr(pc, "_fovraster_pack_state", None) is not None:
        pc._fovraster_pack_state = None


def _auto_packed(pc, means3D, scales, rotations, opacity, shs_rest, shs_dcs, highest_levels, foveation=None):
    """The packed layout of a static model (rasterizer.pack_model), made once and kept on the model object.
    A model counts as static when a call hands over the very same tensor objects, unmodified (autograd version
    counters), as the call before it: the second such call packs, later ones reuse. Models whose getters build new
    tensors on every call (activations evaluated per call) never match and render from the ordinary tensors."""
    tensors = (means3D, scales, rotations, opacity, shs_rest, shs_dcs, highest_levels)
    if foveation is not None and int(FoveationSettings(*foveation).levels) > 4:
        return None  # (the packed layout has four level slots: more layers render from the ordinary tensors)
    if any(t is None or not t.is_cuda for t in tensors) or (torch.is_grad_enabled() and any(t.requires_grad for t in tensors)):
        return None
    st = getattr(pc, "_fovraster_pack_state", None)
    if st is not None and st.matches(tensors):
        if st.packed is None:
            st.packed = pack_model(means3D, scales, rotations, opacity, shs=shs_rest, shs_dcs=shs_dcs,
                                   highest_levels=highest_levels)
        return st.packed
    try:
        pc._fovraster_pack_state = _PackState(tensors)
    except AttributeError:
        pass
    return None


def render(viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0, alpha=None, gazeArray=None,
           blending=None, starter=None, ender=None, highest_levels=None, shs_dcs=None, opacities=None, packed=None,
           foveation=None, appearance_only=False, differentiable=False, want_depth=False):
    """Render the scene for one gaze. Background tensor (bg_color) must be on the GPU.
    want_depth (extension, opt-in, inference): the result gains "depth" and "coverage", [1,H,W] float32 each and without gradient --
    what a compositor merges the frame with its other layers by and reprojects it with. They are the blend's own quantities: over
    the (pixel, Gaussian) pairs the image accumulates, depth = sum of alpha T z (z: the Gaussian's view-space depth) and coverage =
    1 - the final transmittance; in a two-level tile both are mixed with the image's two shares. The background takes no part, a
    pixel no Gaussian reaches holds 0 in both, and nothing is divided: the expected depth is depth / coverage.clamp_min(eps). The
    image and radii are those of the call without the flag, bit for bit. Refused together with appearance_only / differentiable.
    differentiable (extension, opt-in): with autograd on, the image is differentiable in everything a fine-tune step of the composed
    model moves -- pc.get_xyz, get_scaling, get_rotation, get_rest_features and the per-level `shs_dcs` [P,L,3] / `opacities` [P,L]
    (fr_backward_fov; at most 4 layers) -- and "viewspace_points".grad is populated as the plain renderer populates it (what
    densify.add_densification_stats reads). `highest_levels` must not require grad; refused together with appearance_only, with
    packed=, and with more than 4 layers. The derivative is the appearance pass's (blend weights and level decisions are constants).
    appearance_only (extension, opt-in): with autograd on, the image is differentiable in the per-level appearance parameters --
    `opacities` [P,L] and `shs_dcs` [P,L,3] (fr_backward_fov_appearance; at most 4 layers) -- so the composed model can be fine-tuned
    through the renderer that ships it, e.g. against MetamericLoss at the frame's gaze. What the model `pc` hands over (positions,
    scales, rotations, rest SH coefficients) is detached, as the reference's masking render detaches it
    (gaussian_renderer/__init__.py:71-82); `highest_levels` must not require grad; packed= is refused. Without the flag (default)
    the call is the reference's: inference-only, no gradient for anything.
    foveation (extension): a FoveationSettings -- the layer count L of the composed model (opacities [P,L], shs_dcs [P,L,3]) and
    the display geometry; None (default) = the reference's constants, exactly today's call. A model whose width does not match is
    refused.
    packed (extension, opt-in; the image is bit-identical either way): None (default) = render from the ordinary tensors,
    exactly the reference's interface; a rasterizer.PackedModel of this model made by pack_model(); or "auto" = made and
    cached here once the model is seen to be static (_auto_packed: same tensor objects, same storage address, same
    autograd version on two consecutive calls). "auto" costs 336 B per Gaussian (2 GB at 6 M) and cannot see writes that
    bypass the version counter (`t.data.copy_()`, raw-pointer kernels, DLPack aliases): call invalidate_packed(pc) after
    such a write."""
    xyz = pc.get_xyz
    if want_depth and (appearance_only or differentiable):
        raise ValueError("want_depth: depth / coverage are outputs of the inference frame, not of the state-keeping forwards "
                         "(appearance_only / differentiable)")
    if differentiable:
        if appearance_only:
            raise ValueError("differentiable and appearance_only exclude each other: appearance_only detaches what differentiable trains")
        if packed is not None:
            raise ValueError("differentiable: a packed model is inference-only -- training renders from the ordinary tensors (packed=None)")
        if foveation is not None and int(FoveationSettings(*foveation).levels) > 4:
            raise ValueError("differentiable: the backward pass keeps one row of sums per Gaussian, i.e. at most 4 levels, "
                             f"not {int(FoveationSettings(*foveation).levels)}")
    if appearance_only:
        if packed is not None:
            raise ValueError("appearance_only: a packed model is inference-only -- training renders from the ordinary tensors (packed=None)")
        xyz = xyz.detach()
        screenspace_points = zero_points_like(xyz)  # (no gradient of the 2D means in this mode)
    elif torch.is_grad_enabled():
        screenspace_points = torch.zeros_like(xyz, dtype=xyz.dtype, requires_grad=True, device=xyz.device) + 0
        try:
            screenspace_points.retain_grad()
        except Exception:
            pass
    else:
        screenspace_points = zero_points_like(xyz)

    tanfovx = math.tan(viewpoint_camera.FoVx * 0.5)
    tanfovy = math.tan(viewpoint_camera.FoVy * 0.5)
    raster_settings = GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height),
        image_width=int(viewpoint_camera.image_width),
        tanfovx=tanfovx,
        tanfovy=tanfovy,
        bg=bg_color,
        scale_modifier=scaling_modifier,
        viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform,
        sh_degree=pc.active_sh_degree,
        campos=viewpoint_camera.camera_center,
        prefiltered=False,
        debug=False,
    )
    rasterizer = GaussianRasterizer(raster_settings=raster_settings)

    means3D = xyz
    means2D = screenspace_points
    act = getattr(pc, "get_activated", None)  # extension: the three activations as one fused pass (activations.py)
    if act is not None:
        scales, rotations, opacity = act
        if opacities is not None:
            opacity = opacities
    else:
        opacity = pc.get_opacity if opacities is None else opacities
        scales = pc.get_scaling
        rotations = pc.get_rotation
    shs_rest = pc.get_rest_features
    if appearance_only:
        scales, rotations, shs_rest = scales.detach(), rotations.detach(), shs_rest.detach()
        if opacities is None:
            opacity = opacity.detach()  # (the model's own opacity is not the composed model's per-level tensor: pass `opacities`)

    if isinstance(packed, str):
        packed = _auto_packed(pc, means3D, scales, rotations, opacity, shs_rest, shs_dcs, highest_levels, foveation)
    if starter is not None:
        starter.record()
    # (successive inference calls overlap on the GPU -- rasterizer.OVERLAP_SUCCESSIVE_FRAMES; a caller that brackets the call with its
    # own events measures the call's own kernels: that call runs on the caller's stream alone)
    with (serial_frames() if (starter is not None or ender is not None) else contextlib.nullcontext()):
        rendered_image, radii = rasterizer(
            means3D=means3D, means2D=means2D, shs_rest=shs_rest, colors_precomp=None, opacities=opacity, scales=scales,
            rotations=rotations, cov3D_precomp=None, shs_dcs=shs_dcs, highest_levels=highest_levels,
            gazeArray=gazeArray, alpha=alpha, blending=blending, packed=packed, foveation=foveation,
            **({"appearance_only": True} if appearance_only else {}), **({"differentiable": True} if differentiable else {}),
            **({"want_depth": True} if want_depth else {}))
    if ender is not None:
        ender.record()

    # (`radii > 0` as the kernels that write the radii left it: no pass of torch's over the radii behind the frame)
    result = {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": visibility_of(radii),
              "radii": radii}
    if want_depth:
        result["depth"], result["coverage"] = depth_of(radii)
    return result


class PendingRender:
    """A foveated frame between the two halves of its native call (render_begin): finish() -> the dict render() returns."""

    def __init__(self, frame, points):
        self._frame, self._points = frame, points

    def finish(self):
        frame = self._frame
        res = frame.finish()
        radii = res[2]
        if getattr(radii, "_fovraster_visibility", None) is not None:
            visible = visibility_of(radii)  # written beside `radii`, on the frame's stream
        else:
            with torch.cuda.device(frame.device), torch.cuda.stream(frame.stream):  # `radii` is written on the frame's stream
                visible = radii > 0
        return {"render": res[1], "viewspace_points": self._points, "visibility_filter": visible, "radii": radii}


def render_begin(viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0, alpha=None, gazeArray=None,
                 blending=None, highest_levels=None, shs_dcs=None, opacities=None, packed=None, stream=None, foveation=None):
    """Throughput mode (extension, inference only): enqueue the HEAD of a foveated frame -- tile levels, cull pass, projection,
    tile counts, tile scan -- on `stream` (default: the current one) and return without waiting for its instance count;
    PendingRender.finish() waits for the count and enqueues emission, sort, colours and blend. A host that alternates two
    streams -- begin(n + 1) before finish(n) -- keeps two frames in flight: the latency-bound head of one runs beside the sort
    and the blend of the other (csrc/api.hip). Every stream has its own workspaces; the image of a frame is valid once its
    stream has reached the end of finish()'s work (synchronise the stream, or make the consumer's stream wait for it). Same
    arguments and result as render(). The model's and the camera's tensors must be complete on `stream` (tensors made on another
    stream: make `stream` wait for it first); the copies this package caches itself -- the packed model of packed="auto", the
    contiguous copies of transposed camera matrices -- are handed from stream to stream with events (rasterizer._Produced) or
    kept per stream."""
    with torch.no_grad(), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(pc.get_xyz.device)):
        xyz = pc.get_xyz
        rs = GaussianRasterizationSettings(
            image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
            tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5), bg=bg_color,
            scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
            projmatrix=viewpoint_camera.full_proj_transform, sh_degree=pc.active_sh_degree,
            campos=viewpoint_camera.camera_center, prefiltered=False, debug=False)
        act = getattr(pc, "get_activated", None)
        if act is not None:
            scales, rotations, opacity = act
            if opacities is not None:
                opacity = opacities
        else:
            opacity = pc.get_opacity if opacities is None else opacities
            scales, rotations = pc.get_scaling, pc.get_rotation
        shs_rest = pc.get_rest_features
        if isinstance(packed, str):
            packed = _auto_packed(pc, xyz, scales, rotations, opacity, shs_rest, shs_dcs, highest_levels, foveation)
        if gazeArray is None:
            raise Exception("gazeArray is required by the foveated rasterizer")
        gaze = gazeArray.detach().flatten().tolist() if isinstance(gazeArray, torch.Tensor) else list(gazeArray)
        empty = torch.Tensor([])
        frame = _forward_begin(_native.VARIANT_FOV_PCHECK_OBB, rs, xyz, shs_rest, empty, opacity, scales, rotations, empty,
                               shs_dcs, highest_levels, (float(gaze[0]), float(gaze[1])), float(alpha), persistent=True,
                               packed=packed, foveation=foveation)
        return PendingRender(frame, zero_points_like(xyz))
