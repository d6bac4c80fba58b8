"""Host state that survives from one call to the next (round 6), where it could hand a frame somebody else's numbers:

  * the process-wide pool of pinned totals blocks and the frames' sequence tags (csrc/api.hip): two host threads rendering on one
    device take turns on the same blocks, and a frame must never read the totals another thread's frame left there;
  * the argument struct an internal stream of the successive-frame overlap uses again (rasterizer._forward_overlapped): it points at
    converted copies of the camera tensors, and a host that builds a camera per frame hands over NEW tensors at recurring ids and
    addresses.

Every frame is compared bit for bit with the same call made from the main thread inside serial_frames()."""
import threading

import pytest
import torch

from tests.helpers import cam_dict, scene_dict, small_camera, small_cloud, syn
from tests import parity_report
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAZES = [(0.1 + 0.15 * i, 0.9 - 0.14 * i) for i in range(6)]
BG = (0.1, 0.2, 0.3)


def _need_gpu():
    if not torch.cuda.is_available():  # only reached by an explicit -m gpu run (tests/conftest.py skips otherwise)
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


class _Pipe:
    debug = False


class _Frozen:
    """the static model of test_successive_inference_frames_overlap_and_stay_identical: the same tensor objects at every call"""

    def __init__(self, c):
        with torch.no_grad():
            self.get_xyz, self.get_scaling, self.get_rotation = c.get_xyz.detach(), c.get_scaling.detach(), c.get_rotation.detach()
            self.get_opacity, self.get_rest_features = c.get_opacity.detach(), c.get_rest_features.detach().contiguous()
        self.active_sh_degree = 3


def _ring(index, W=640, H=360):
    """cameras on a ring BEHIND the identity camera of scene_1k's cloud (which sits around (0, 0, 4)): indices 10 .. 14 of 16 see it"""
    return syn.camera_ring(index, 16, W, H)


class _FovScene:
    """scene_1k(P=20000) at 640x360 through the foveated rasterizer -- the model of the overlap test"""

    def __init__(self):
        from fov3dgs_amd.gaussian_renderer_fov import render as render_fov
        self.render_fov = render_fov
        self.cpu = syn.scene_1k(P=20000, seed=4)
        self.layers_cpu = syn.foveation_layers(self.cpu, seed=5)
        self.pc = _Frozen(self.cpu.to(DEV))
        self.highest, self.shs_dcs, self.opac = [t.to(DEV) for t in self.layers_cpu]
        self.bg = torch.tensor(BG, device=DEV)

    def frame(self, cam, gaze):
        return self.render_fov(cam, self.pc, self.bg, alpha=0.05, gazeArray=gaze, blending=True, highest_levels=self.highest,
                               shs_dcs=self.shs_dcs, opacities=self.opac)

    def oracle_count(self, cam, gaze):
        scene = scene_dict(self.cpu, "fov_pcheck_obb", self.layers_cpu)
        return int(orc.forward("fov_pcheck_obb", scene, cam_dict(cam, bg=BG, gaze=gaze))["num_rendered"])


class _PlainScene:
    """small_cloud(P=3000) at 320x200 through pcheck_obb, two cameras taking turns"""

    def __init__(self):
        from fov3dgs_amd.gaussian_renderer import render
        self.render = render
        self.cpu = small_cloud(P=3000)
        self.pc = self.cpu.to(DEV)
        self.bg = torch.tensor(BG, device=DEV)

    def frame(self, cam, gaze=None):
        return self.render(cam, self.pc, _Pipe(), self.bg, cuda_type="pcheck_obb")

    def oracle_count(self, cam, gaze=None):
        return int(orc.forward("pcheck_obb", scene_dict(self.cpu, "pcheck_obb"), cam_dict(cam, bg=BG))["num_rendered"])


_counts = {}  # thread ident -> the num_rendered of every frame that thread finished, in order


@pytest.fixture
def count_spy(monkeypatch):
    """render() does not return num_rendered: FrameInFlight.finish is watched (unchanged otherwise) and keeps the count per thread"""
    from fov3dgs_amd import rasterizer as rz
    orig = rz.FrameInFlight.finish

    def finish(self, *a, **kw):
        res = orig(self, *a, **kw)
        _counts.setdefault(threading.get_ident(), []).append(int(res[0]))
        return res
    monkeypatch.setattr(rz.FrameInFlight, "finish", finish)
    _counts.clear()
    yield _counts
    _counts.clear()


def _last_count():
    return _counts[threading.get_ident()][-1]


@pytest.fixture(scope="module")
def cases():
    """what the tests of this module share -- the models on the GPU, the cameras, the oracle's counts --, made once by the first test that
    needs it and released with the module"""
    cache = {}
    yield cache
    cache.clear()


def _fov_scene(cases):
    if "_fov" not in cases:
        cases["_fov"] = _FovScene()
    return cases["_fov"]


def _two_thread_case(cases, kind):
    """-> (calls of thread A, calls of thread B, oracle counts of frame 0 of each): six calls per thread, each a function of no
    arguments; made once and shared by the two tests that use it"""
    if kind in cases:
        return cases[kind]
    fov = _fov_scene(cases)
    if kind == "two kinds":
        if "_plain" not in cases:
            cases["_plain"] = _PlainScene()
        plain = cases["_plain"]
        cam_a = syn.camera_1k(640, 360).to(DEV)
        cams_b = [syn.camera_1k(320, 200).to(DEV), small_camera(320, 200).to(DEV)]
        calls_a = [(lambda g=g: fov.frame(cam_a, g)) for g in GAZES]
        calls_b = [(lambda c=cams_b[i % 2]: plain.frame(c)) for i in range(6)]
        oracle = (fov.oracle_count(syn.camera_1k(640, 360), GAZES[0]), plain.oracle_count(syn.camera_1k(320, 200)))
    else:  # the same kind of frame (P, W, H, variant) through two cameras of the ring: only the counts differ
        cam_a, cam_b = _ring(11).to(DEV), _ring(13).to(DEV)
        calls_a = [(lambda g=g: fov.frame(cam_a, g)) for g in GAZES]
        calls_b = [(lambda g=g: fov.frame(cam_b, g)) for g in GAZES]
        oracle = (fov.oracle_count(_ring(11), GAZES[0]), fov.oracle_count(_ring(13), GAZES[0]))
    cases[kind] = (calls_a, calls_b, oracle)
    return cases[kind]


def _references(calls):
    """every call from the main thread, on the caller's stream alone -> [(image, radii, num_rendered)]"""
    from fov3dgs_amd import rasterizer as rz
    out = []
    with torch.no_grad(), rz.serial_frames():
        for call in calls:
            o = call()
            out.append((o["render"].clone(), o["radii"].clone(), _last_count()))
    torch.cuda.synchronize()
    return out


def _run_two_threads(calls_a, calls_b, frames, handshake):
    """Two fresh threads on cuda:0, `frames` frames each (frame i = call i mod 6). handshake: A1, B1, A2, B2, ... strictly in turn.
    -> ([(call index, image, radii, num_rendered)] of A, the same of B); a thread's exception is raised here."""
    n = frames
    a_done = [threading.Event() for _ in range(n)]
    b_done = [threading.Event() for _ in range(n)]
    outs, errors = ([], []), []

    def body(which, calls, wait_for, done):
        try:
            torch.cuda.set_device(0)
            with torch.no_grad():
                for i in range(n):
                    if handshake and wait_for(i) is not None and not wait_for(i).wait(40):
                        raise RuntimeError(f"thread {which}: the other thread never finished its turn before frame {i}")
                    o = calls[i % len(calls)]()
                    outs[which].append((i % len(calls), o["render"], o["radii"], _last_count()))
                    done[i].set()
            torch.cuda.synchronize()
        except BaseException as ex:  # noqa: BLE001 -- raised again in the main thread
            errors.append(ex)
            for e in a_done + b_done:  # (the other thread must not wait for a turn that will not come)
                e.set()

    ta = threading.Thread(target=body, args=(0, calls_a, lambda i: b_done[i - 1] if i else None, a_done), daemon=True)
    tb = threading.Thread(target=body, args=(1, calls_b, lambda i: a_done[i], b_done), daemon=True)
    ta.start()
    tb.start()
    ta.join(50)  # (together below the test's own time limit: a stuck thread is reported by the assertion below)
    tb.join(50)
    if errors:
        raise errors[0]
    assert not ta.is_alive() and not tb.is_alive(), "a render thread did not finish"
    assert len(outs[0]) == n and len(outs[1]) == n
    return outs


def _check_two_threads(cases, kind, frames, handshake):
    calls_a, calls_b, oracle = _two_thread_case(cases, kind)
    want = (_references(calls_a), _references(calls_b))
    # the test proves nothing unless a frame that took the other thread's totals would show: the two threads' counts differ, frame by frame
    for (_, _, na), (_, _, nb) in zip(*want):
        assert na != nb and na > 0 and nb > 0, (na, nb)
    assert want[0][0][2] == oracle[0] and want[1][0][2] == oracle[1], (want[0][0][2], want[1][0][2], oracle)
    got = _run_two_threads(calls_a, calls_b, frames, handshake)
    for which in (0, 1):
        for k, (i, img, rad, n) in enumerate(got[which]):
            wi, wr, wn = want[which][i]
            assert n == wn, ("num_rendered", "AB"[which], k, n, wn)
            assert torch.equal(rad, wr), ("radii", "AB"[which], k)
            assert torch.equal(img, wi), ("image", "AB"[which], k)
        first = next(n for i, _, _, n in got[which] if i == 0)
        assert first == oracle[which], ("oracle count", "AB"[which], first, oracle[which])
    for (_, _, _, na), (_, _, _, nb) in zip(*got):
        assert na != nb


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", ("two kinds", "same kind"))
def test_two_threads_taking_turns_keep_their_own_totals(kind, cases, count_spy):
    """Two host threads on one device, strictly in turn (A1, B1, A2, B2, ...: six inference frames each, from a fresh pair of threads).
    The pool of pinned totals blocks is one per process, so B's k-th frame takes the block A's k-th frame has just given back. With a
    sequence tag counted per THREAD that block already held B's own tag -- k -- and B's poll passed before its tile scan had written:
    B took A's instance count, binning capacity and sort class counts. The tags are counted per process now (and an idle block's tag
    is cleared when it is handed out), so every frame is the one the main thread rendered alone: image, radii and num_rendered, the
    latter also against the oracle. "two kinds": a foveated 640x360 frame of 20000 Gaussians and a pcheck_obb 320x200 frame of 3000;
    "same kind": P, W, H and variant equal, two cameras -- only the counts differ."""
    _need_gpu()
    _check_two_threads(cases, kind, 6, True)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", ("two kinds", "same kind"))
def test_two_threads_running_free_keep_their_own_totals(kind, cases, count_spy):
    """The same two threads without the handshake, 30 frames each: frames of both threads in flight at once, blocks of the pool going
    back and forth in whatever order the threads get there."""
    _need_gpu()
    _check_two_threads(cases, kind, 30, False)


# ---- a fresh camera per frame -----------------------------------------------------------------------------------------------------

CAM_GAZES = GAZES[:4]


def _camera_references(fov, indices):
    """ring camera index -> [(image, radii)] over CAM_GAZES, rendered on the caller's stream alone"""
    from fov3dgs_amd import rasterizer as rz
    want = {}
    with torch.no_grad(), rz.serial_frames():
        for idx in indices:
            cam = _ring(idx).to(DEV)
            want[idx] = []
            for g in CAM_GAZES:
                o = fov.frame(cam, g)
                want[idx].append((o["render"].clone(), o["radii"].clone()))
    torch.cuda.synchronize()
    return want


def _four_frames_through_a_new_camera(fov, idx):
    """the camera lives in this function alone: when it returns, its tensors' ids and addresses are free for the next camera"""
    cam = _ring(idx).to(DEV)
    with torch.no_grad():
        return [fov.frame(cam, g) for g in CAM_GAZES]


def test_a_new_camera_at_a_dead_cameras_identity_is_not_rendered_with_the_old_one(cases, monkeypatch):
    """The argument struct an internal stream uses again is keyed on (id, version, address, shape, stride) of the inputs -- all of which
    a NEW tensor can repeat once the old one is gone -- and points at the converted copy of the old camera's transposed view matrix.
    Here the collision is forced: the signature keeps only version, shape and stride, so that every camera of the same geometry has
    the key of the one before it; what must still tell them apart is the weak-reference test of `same`, the module's own contract.
    Four frames through camera A, four through B (A dropped), four through C (built inside a function): with three internal streams the
    second to fourth frame after a change are the ones a struct of an older camera would still be waiting for. Every frame is the
    serial render of ITS camera, bit for bit, and A's and B's frames differ."""
    _need_gpu()
    from fov3dgs_amd import rasterizer as rz
    assert rz.OVERLAP_SUCCESSIVE_FRAMES and rz.OVERLAP_SLOTS == 3
    fov = _fov_scene(cases)
    want = _camera_references(fov, (11, 12, 13))
    monkeypatch.setattr(rz, "_input_signature", lambda tensors: tuple((t._version, tuple(t.shape), t.stride()) for t in tensors))
    got = {}
    with torch.no_grad():
        cam = _ring(11).to(DEV)
        got[11] = [fov.frame(cam, g) for g in CAM_GAZES]
        del cam
        cam = _ring(12).to(DEV)
        got[12] = [fov.frame(cam, g) for g in CAM_GAZES]
    got[13] = _four_frames_through_a_new_camera(fov, 13)
    torch.cuda.synchronize()
    for (ia, _), (ib, _) in zip(want[11], want[12]):
        assert float((ia - ib).abs().max()) > 1e-3  # the cameras matter
    for idx in (11, 12, 13):
        for k, (o, (wi, wr)) in enumerate(zip(got[idx], want[idx])):
            assert torch.equal(o["radii"], wr), ("radii", idx, k)
            assert torch.equal(o["render"], wi), ("image", idx, k)


def test_a_camera_built_and_dropped_per_frame(cases, monkeypatch):
    """The same without forcing anything: twelve frames, each through a camera built and dropped inside a function, as a host that
    makes its camera per frame does. How many frames met the key of the frame three calls earlier (the previous frame of their
    internal stream) is recorded (tests/parity_report.py), not judged: it depends on the allocator and on CPython's ids."""
    _need_gpu()
    from fov3dgs_amd import rasterizer as rz
    fov = _fov_scene(cases)
    indices = (10, 11, 12, 13)  # frame i and frame i - 3 never share a camera
    want = _camera_references(fov, indices)
    keys, begin = [], rz._forward_begin

    def watched(*a, **kw):
        keys.append(kw.get("reuse_key"))
        return begin(*a, **kw)
    monkeypatch.setattr(rz, "_forward_begin", watched)

    def one_frame(i):
        cam = _ring(indices[i % 4]).to(DEV)
        with torch.no_grad():
            return fov.frame(cam, CAM_GAZES[i % 4])
    got = [one_frame(i) for i in range(12)]
    torch.cuda.synchronize()
    assert len(keys) == 12 and all(k is not None for k in keys)
    recurring = sum(1 for i in range(3, 12) if keys[i] == keys[i - 3])
    parity_report.record("info", "test_a_camera_built_and_dropped_per_frame: frames whose reuse key equals that of three calls earlier",
                         recurring=recurring, frames=12)
    for i, o in enumerate(got):
        wi, wr = want[indices[i % 4]][i % 4]
        assert torch.equal(o["radii"], wr), ("radii", i)
        assert torch.equal(o["render"], wi), ("image", i)
