"""The foveated frame without an image fill (csrc/api.hip, k_project): the two level states of a two-level tile are ADDED into
out_color, so those tiles' pixels must have been cleared -- by k_project's waves, tile by tile -- and every other pixel is stored
outright. Every case renders into a buffer full of NaN through the C ABI (or, through the renderers, into whatever the caching
allocator hands out, which the test has left full of NaN and of other gazes' images): a pixel nobody cleared or stored, or a
two-level tile that kept a stale value, cannot equal the same frame rendered into zeros. Each case first checks, from the
tile-level map the library keeps, that the frame has both kinds of tiles."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import cam_dict, scene_dict, small_camera, small_case, small_cloud, syn
from tests.checks import check_image
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

FOV = "fov_pcheck_obb"
BG = (0.3, 0.6, 0.9)
NAN = float("nan")


def _need_gpu():
    if not torch.cuda.is_available():  # only reached by an explicit -m gpu run (tests/conftest.py skips otherwise)
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


@functools.lru_cache(maxsize=None)
def _ragged(gaze):
    """203 x 131: 13 x 9 tiles, the last column 11 pixels wide, the last row 3 pixels high; W is no multiple of four"""
    scene, cam = small_case(FOV, P=3000, seed=3, bg=BG, gaze=gaze, width=203, height=131)
    return scene, cam, orc.forward(FOV, scene, cam)


def _check(variant, scene, cam, want=None, two_kinds=True, **kw):
    from tests.abi_forward import abi_forward, need_both_kinds_of_tiles
    got = abi_forward(variant, scene, cam, image_fill=NAN, **kw)
    if two_kinds:
        need_both_kinds_of_tiles(got)
    zero = abi_forward(variant, scene, cam, image_fill=0.0, **kw)
    assert not bool(torch.isnan(got["color"]).any())
    assert torch.equal(got["color"], zero["color"])
    assert torch.equal(got["radii"], zero["radii"]) and got["num_rendered"] == zero["num_rendered"]
    if want is not None:
        assert got["num_rendered"] == want["num_rendered"]
        check_image(got["color"].cpu().numpy(), want["color"], name=f"{variant} into NaN")
    return got


@pytest.mark.parametrize("gaze", ((0.5, 0.5), (0.05, 0.95), (0.25, 0.75)))
def test_ragged_frame(gaze):
    _need_gpu()
    scene, cam, want = _ragged(gaze)
    _check(FOV, scene, cam, want)


@pytest.mark.parametrize("mode", ("packed", "debug"))
def test_packed_layout_and_debug_mode(mode):
    """k_project<..., true> is another instantiation; debug = 1 takes the frame off the helper streams and checks every launch"""
    _need_gpu()
    scene, cam, want = _ragged((0.25, 0.75))
    _check(FOV, scene, cam, want, packed=mode == "packed", debug=int(mode == "debug"))


def test_one_workgroup_clears_every_tile():
    """P = 40: k_project's grid is one workgroup of 16 waves, which share out the 920 tiles of a 640 x 360 frame (W % 4 == 0: the
    float4 stores)"""
    _need_gpu()
    scene, cam = small_case(FOV, P=40, seed=9, bg=BG, gaze=(0.5, 0.5), width=640, height=360)
    want = orc.forward(FOV, scene, cam)
    assert want["tile_blend"].size == 920
    _check(FOV, scene, cam, want)


def test_two_level_tiles_nothing_reaches_show_the_background():
    """A cloud in the left third of a 320 x 200 frame: the two-level tiles to its right have empty lists, and their two halves
    bg * w1 + bg * (1 - w1) must come out as the background itself (they do in the reference's arithmetic for this background:
    checked against the oracle's image below as well)."""
    _need_gpu()
    W, H = 320, 200
    scene, cam = small_case(FOV, P=4000, seed=5, bg=BG, gaze=(0.5, 0.5), width=W, height=H)
    n = len(scene["means3D"])
    scene["means3D"] = (scene["means3D"] - 2.0 * np.asarray(cam["viewmatrix"])[:3, 0]).astype(np.float32)  # two units to the camera's left
    h = np.concatenate([scene["means3D"], np.ones((n, 1), np.float32)], 1) @ np.asarray(cam["projmatrix"])
    keep = (h[:, 0] / (h[:, 3] + 1e-7) < -0.55) & (h[:, 3] > 0.5) & (scene["scales"].max(1) < 0.1)
    scene = {k: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in scene.items()}
    assert keep.sum() > 1000
    want = orc.forward(FOV, scene, cam)
    got = _check(FOV, scene, cam, want)
    gx = (W + 15) // 16
    two, ranges = got["tile_blend"].cpu().numpy(), got["ranges"].cpu().numpy()
    listed = ranges[:, 1] > ranges[:, 0]
    assert (np.nonzero(listed)[0] % gx).max() * 16 + 16 <= W / 3  # the cloud keeps to the left third ...
    assert (two & listed).sum() >= 10 and (two & ~listed).sum() >= 10  # ... and there are two-level tiles on either side
    img, bg = got["color"].cpu().numpy(), np.asarray(BG, np.float32)[:, None, None]
    for t in np.nonzero(two & ~listed)[0]:
        ty, tx = divmod(int(t), gx)
        assert (img[:, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] == bg).all(), (tx, ty)


def test_nothing_to_render():
    """A cloud behind the camera (every Gaussian culled, num_rendered == 0: the blend still runs over every tile), and P == 0 (the
    library returns the reference's zero image from a fill of its own, before any kernel or workspace: there is no tile map)"""
    _need_gpu()
    from tests.abi_forward import abi_forward
    scene, cam = small_case(FOV, P=500, seed=9, bg=BG, gaze=(0.5, 0.5), width=203, height=131)
    scene["means3D"] = (scene["means3D"] - 14.0 * np.asarray(cam["viewmatrix"])[:3, 2]).astype(np.float32)
    got = _check(FOV, scene, cam)
    assert got["num_rendered"] == 0 and not bool((got["radii"] != 0).any())
    assert (got["color"].cpu().numpy() == np.asarray(BG, np.float32)[:, None, None]).all()
    empty = {k: (v[:0] if isinstance(v, np.ndarray) and v.shape[:1] == (500,) else v) for k, v in scene.items()}
    none = abi_forward(FOV, empty, cam, image_fill=NAN)
    assert none["num_rendered"] == 0 and not bool((none["color"] != 0).any())


def test_shared_and_multi_model_frames_store_every_tile():
    """SMFR and MMFR share k_project's foveated instantiation and the tile-level map, but their blend stores every tile: nothing of
    theirs is cleared, and nothing needs to be -- the image equals the one rendered into zeros (and the oracle's, within tolerance)"""
    _need_gpu()
    scene_f, cam = small_case(FOV, P=3000, seed=23, bg=BG, gaze=(0.25, 0.75), width=203, height=131)
    plain, _ = small_case("pcheck_obb", P=3000, seed=23, width=203, height=131)
    scene = dict(plain, highest_levels=scene_f["highest_levels"])
    _check("naive_pcheck_obb", scene, cam, orc.forward("naive_pcheck_obb", scene, cam))
    scene = dict(plain, highest_levels=np.zeros((3000, 1), np.float32))
    cam = dict(cam, cur_level=1.0)
    _check("mmfr_pcheck_obb", scene, cam, orc.forward("mmfr_pcheck_obb", scene, cam))


GAZES = ((0.5, 0.5), (0.05, 0.95), (0.25, 0.75))


@functools.lru_cache(maxsize=None)
def _model():
    """The ragged frame's cloud as a model for the renderers, and the serial single-frame image of each gaze"""
    from fov3dgs_amd import rasterizer as rz
    from fov3dgs_amd.gaussian_renderer_fov import render
    from tests.abi_forward import abi_forward, need_both_kinds_of_tiles
    dev = "cuda:0"
    cpu = small_cloud(3000, 3)
    fov = syn.foveation_layers(cpu, seed=4)
    for gaze in GAZES:  # (the same model and camera through the C ABI: the tile map)
        need_both_kinds_of_tiles(abi_forward(FOV, scene_dict(cpu, FOV, fov), cam_dict(small_camera(203, 131), bg=BG, gaze=gaze)))
    cloud, cam = cpu.to(dev), small_camera(203, 131).to(dev)
    kw = dict(alpha=0.05, blending=True, highest_levels=fov[0].to(dev), shs_dcs=fov[1].to(dev), opacities=fov[2].to(dev))
    bg = torch.tensor(BG, device=dev)
    serial = []
    with torch.no_grad(), rz.serial_frames():
        for gaze in GAZES:
            serial.append(render(cam, cloud, bg, gazeArray=gaze, **kw)["render"].clone())
    torch.cuda.synchronize()
    assert not torch.equal(serial[0], serial[1]) and not torch.equal(serial[1], serial[2])
    return cloud, cam, bg, kw, serial


def test_successive_frames_into_dirty_blocks():
    """Six frames cycling three gazes through render(), successive frames overlapping on the internal streams. The allocator's
    free blocks hold NaN to begin with; every image is filled with NaN before it is dropped, so the next frames on its stream are
    handed blocks full of NaN, where an image of another gaze stood before."""
    _need_gpu()
    from fov3dgs_amd import rasterizer as rz
    from fov3dgs_amd.gaussian_renderer_fov import render
    from tests.abi_forward import dirty_allocator
    cloud, cam, bg, kw, serial = _model()
    assert rz.OVERLAP_SUCCESSIVE_FRAMES
    dirty_allocator(203, 131)
    with torch.no_grad():
        for rnd in range(2):
            got = []
            for i in range(6):
                img = render(cam, cloud, bg, gazeArray=GAZES[i % 3], **kw)["render"]
                got.append(img.clone())
                img.fill_(NAN)
                del img
            torch.cuda.synchronize()
            for i, img in enumerate(got):
                assert torch.equal(img, serial[i % 3]), (rnd, i)


def test_two_frames_in_flight_into_dirty_blocks():
    """The same through render_begin / finish on two streams, the head of one frame enqueued before the other's tail"""
    _need_gpu()
    from fov3dgs_amd.gaussian_renderer_fov import render_begin
    from tests.abi_forward import dirty_allocator
    cloud, cam, bg, kw, serial = _model()
    dev = bg.device
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for st in streams:
        with torch.cuda.stream(st):
            dirty_allocator(203, 131)
    order = ((0, 1), (2, 0), (1, 2))
    for rnd in range(2):
        for ga, gb in order:
            pa = render_begin(cam, cloud, bg, gazeArray=GAZES[ga], stream=streams[0], **kw)
            pb = render_begin(cam, cloud, bg, gazeArray=GAZES[gb], stream=streams[1], **kw)
            ra, rb = pa.finish(), pb.finish()
            torch.cuda.synchronize()
            for res, g, st in ((ra, ga, streams[0]), (rb, gb, streams[1])):
                assert torch.equal(res["render"], serial[g]), (rnd, ga, gb, g)
                with torch.cuda.stream(st):
                    res["render"].fill_(NAN)
            del ra, rb, res
            torch.cuda.synchronize()
