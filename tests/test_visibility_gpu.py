"""fr_forward_ext.visibility (include/fovraster.h): the mask `radii > 0`, written by the kernels that write the radii -- k_project
where it zeroes a chunk's radii, k_bin at each of its three stores (the projection's result, an item that landed in no tile, a
frame-sized splat that landed in none). The buffer starts as 0xFF everywhere: a byte nobody wrote is neither 0 nor 1. The clouds
(tests/abi_forward.py: visibility_case) hold Gaussians behind the camera and off screen, a splat on the whole-wave path and one on
the whole-workgroup path, and -- foveated model -- Gaussians the level filter removes from every tile they reach."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import small_camera, small_cloud, syn
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

FOV = "fov_pcheck_obb"
FR_BIG_TNUM, FR_GIANT_TNUM = 64, 1024  # csrc/common.h


def _need_gpu():
    if not torch.cuda.is_available():  # only reached by an explicit -m gpu run (tests/conftest.py skips otherwise)
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


@functools.lru_cache(maxsize=None)
def _case(variant, P):
    """the cloud, and what the oracle says of it: it holds what the docstring promises"""
    from tests.abi_forward import BEHIND, BIG, GIANT, OFF_SCREEN, visibility_case
    scene, cam = visibility_case(variant, P)
    want = orc.forward(variant, scene, cam)
    h = np.concatenate([scene["means3D"], np.ones((P, 1), np.float32)], 1)
    depth, clip = (h @ np.asarray(cam["viewmatrix"]))[:, 2], h @ np.asarray(cam["projmatrix"])
    assert (depth[BEHIND] <= 0.2).all()  # (the near plane of the reference's frustum test)
    assert (depth[OFF_SCREEN] > 0.2).all() and (clip[OFF_SCREEN, 0] / clip[OFF_SCREEN, 3] > 1.3).all()
    assert (want["radii"][BEHIND] == 0).all() and (want["radii"][OFF_SCREEN] == 0).all()
    # (tiles the splat ends up in: no more than the tiles of the rectangle the binning kernel walks for it)
    assert FR_BIG_TNUM <= want["tiles_touched"][BIG] < FR_GIANT_TNUM <= want["tiles_touched"][GIANT]
    assert 0 < (want["radii"] > 0).sum() < P
    return scene, cam, want


@pytest.mark.parametrize("P", (37, 1037))
@pytest.mark.parametrize("packed", (False, True), ids=("tensors", "packed"))
@pytest.mark.parametrize("variant", ("original", "pcheck_obb_sum", FOV))
def test_visibility_is_radii_positive(variant, packed, P):
    _need_gpu()
    from tests.abi_forward import FILTERED, abi_forward
    scene, cam, want = _case(variant, P)
    got = abi_forward(variant, scene, cam, image_fill=0.0, visibility_fill=0xFF, packed=packed)
    vis, radii = got["visibility"], got["radii"]
    assert int(vis.max()) <= 1, "a byte was left unwritten"
    assert torch.equal(vis.view(torch.bool), radii > 0)
    assert 0 < int(vis.sum()) < P
    assert int(vis.sum()) == int((want["radii"] > 0).sum())
    if variant == FOV:
        # the level filter bites: rows with a radius in the plain frame of the same camera that the foveated frame leaves without one
        plain_scene, plain_cam, _ = _case("pcheck_obb", P)
        plain = abi_forward("pcheck_obb", plain_scene, plain_cam, image_fill=0.0, visibility_fill=0xFF)
        assert torch.equal(plain["visibility"].view(torch.bool), plain["radii"] > 0)
        lost = (plain["radii"] > 0) & (radii == 0)
        assert bool(lost[FILTERED].all()) and int(lost.sum()) >= 6
        assert not bool(vis[lost].any())


@functools.lru_cache(maxsize=None)
def _model():
    dev = "cuda:0"
    cpu = small_cloud(3000, 3)
    fov = [t.to(dev) for t in syn.foveation_layers(cpu, seed=4)]
    return cpu.to(dev), small_camera(203, 131).to(dev), torch.tensor([0.3, 0.6, 0.9], device=dev), fov


def _is_the_mask(out, P):
    vis = out["visibility_filter"]
    assert vis.dtype == torch.bool and tuple(vis.shape) == (P,)
    torch.cuda.synchronize()
    assert torch.equal(vis, out["radii"] > 0) and 0 < int(vis.sum()) < P


@pytest.mark.parametrize("grad", (False, True), ids=("no_grad", "grad"))
def test_through_the_plain_renderer(grad):
    _need_gpu()
    from fov3dgs_amd import _native
    from fov3dgs_amd.gaussian_renderer import render
    assert _native.has_forward_ext()
    cloud, cam, bg, _ = _model()

    class Pipe:
        debug = False
    with (torch.enable_grad() if grad else torch.no_grad()):
        model = small_cloud(3000, 3).to(bg.device).requires_grad_(True) if grad else cloud
        out = render(cam, model, Pipe(), bg, cuda_type="pcheck_obb_sum")
        _is_the_mask(out, 3000)
        assert getattr(out["radii"], "_fovraster_visibility", None) is out["visibility_filter"]  # (the kernels' mask, not a comparison's)
        if grad:
            out["render"].sum().backward()  # (the mask beside the radii does not disturb the graph)
            assert model._xyz.grad is not None and bool(torch.isfinite(model._xyz.grad).all())


@pytest.mark.parametrize("overlap", (True, False), ids=("overlapped", "serial"))
def test_through_the_foveated_renderer(overlap):
    _need_gpu()
    from fov3dgs_amd import rasterizer as rz
    from fov3dgs_amd.gaussian_renderer_fov import render
    cloud, cam, bg, fov = _model()
    kw = dict(alpha=0.05, blending=True, highest_levels=fov[0], shs_dcs=fov[1], opacities=fov[2])
    assert rz.OVERLAP_SUCCESSIVE_FRAMES
    outs = []
    with torch.no_grad(), (rz.serial_frames() if not overlap else torch.no_grad()):
        for gaze in ((0.5, 0.5), (0.05, 0.95), (0.25, 0.75), (0.5, 0.5)):
            outs.append(render(cam, cloud, bg, gazeArray=gaze, **kw))
    for out in outs:
        _is_the_mask(out, 3000)
        assert getattr(out["radii"], "_fovraster_visibility", None) is out["visibility_filter"]
    assert not torch.equal(outs[0]["visibility_filter"], outs[1]["visibility_filter"])  # (the gaze moves the level boxes)


def test_through_render_begin_and_finish():
    _need_gpu()
    from fov3dgs_amd.gaussian_renderer_fov import render_begin
    cloud, cam, bg, fov = _model()
    kw = dict(alpha=0.05, blending=True, highest_levels=fov[0], shs_dcs=fov[1], opacities=fov[2])
    streams = [torch.cuda.Stream(bg.device), torch.cuda.Stream(bg.device)]
    pa = render_begin(cam, cloud, bg, gazeArray=(0.05, 0.95), stream=streams[0], **kw)
    pb = render_begin(cam, cloud, bg, gazeArray=(0.5, 0.5), stream=streams[1], **kw)
    for out in (pa.finish(), pb.finish()):
        _is_the_mask(out, 3000)
        assert getattr(out["radii"], "_fovraster_visibility", None) is out["visibility_filter"]
