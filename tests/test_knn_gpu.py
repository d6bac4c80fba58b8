"""simple_knn.distCUDA2 on the MI355X (csrc/knn.hip): bit-equal to the exact k-d tree reference (tests/knn_exact.c) on
uniform clouds at every leaf / level boundary, on degenerate and clustered sets and on the S-6M positions; the calling
conventions of the reference's distCUDA2; and a model initialised from a storePly-layout point cloud that trains one step."""
import math
import os

import numpy as np
import pytest
import torch

from tests import knn_ref as R
import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import synthetic as syn
from fov3dgs_amd.simple_knn._C import distCUDA2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def exact(tmp_path_factory):
    d = tmp_path_factory.mktemp("knn_exact")
    exe = R.build_exact(d)
    return lambda pts: R.run_exact(exe, pts, d)


def _gpu(x):
    return distCUDA2(torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)).cpu().numpy()


def _same(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert bad.size == 0, f"{bad.size} of {got.size} differ, first {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 63, 64, 65, 127, 4095, 4096, 4097, 262143, 262144, 262145])
def test_uniform_bit_exact(exact, P):
    x = R.uniform_cloud(P, seed=1000 + P, lo=-3.0, hi=5.0)
    _same(_gpu(x), exact(x))


@pytest.mark.parametrize("name", list(R.degenerate_clouds(64).keys()))
def test_degenerate_bit_exact(exact, name):
    x = R.degenerate_clouds(20_000)[name]
    got = _gpu(x)
    _same(got, exact(x))
    if name == "identical":
        assert np.all(got == 0)


@pytest.mark.parametrize("P", [200_000, 1_000_000])
def test_clustered_bit_exact(exact, P):
    x = syn.points_colmap_like(P).numpy()
    _same(_gpu(x), exact(x))


def test_bicycle_scale_positions_bit_exact(exact):
    x = syn.scene_bicycle_scale().get_xyz.numpy()
    _same(_gpu(x), exact(x))


def test_calling_conventions():
    x = torch.from_numpy(R.uniform_cloud(50_000, seed=5)).to(DEV)
    a = distCUDA2(x)
    assert a.dtype == torch.float32 and a.device == x.device and tuple(a.shape) == (50_000,) and not a.requires_grad
    assert torch.equal(a, distCUDA2(x))                            # no float atomics: the same bits every call
    x4 = torch.cat([x, torch.randn(50_000, 1, device=DEV)], 1)
    assert not x4[:, :3].is_contiguous()
    assert torch.equal(distCUDA2(x4[:, :3]), a)                    # .contiguous() of the reference
    xg = x.clone().requires_grad_(True)
    g = distCUDA2(xg)
    assert not g.requires_grad and g.grad_fn is None and torch.equal(g, a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b = distCUDA2(x)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(a, b)
    e = distCUDA2(torch.zeros(0, 3, device=DEV))
    assert e.shape == (0,) and e.dtype == torch.float32 and e.device == x.device
    with pytest.raises(RuntimeError, match="float32"):
        distCUDA2(x.double())
    with pytest.raises(RuntimeError, match=r"\[P, 3\]"):
        distCUDA2(x4)
    with pytest.raises(RuntimeError, match=r"\[P, 3\]"):
        distCUDA2(x.reshape(-1))


def test_non_finite_points_are_nobodys_neighbour(exact):
    x = R.uniform_cloud(20_000, seed=9)
    bad = np.zeros(x.shape[0], bool)
    bad[::997] = True
    y = x.copy()
    y[bad] = np.array([[np.nan, 0, 0], [np.inf, 1, 1], [0, -np.inf, 2]], np.float32)[np.arange(bad.sum()) % 3]
    got = _gpu(y)
    assert np.all(np.isnan(got[bad]))
    _same(got[~bad], exact(x[~bad]))


def _store_ply(path, xyz, rgb):
    """storePly's layout (fov3dgs/scene/dataset_readers.py:115-130), written without plyfile."""
    dt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
          ("red", "u1"), ("green", "u1"), ("blue", "u1")]
    a = np.zeros(xyz.shape[0], dtype=dt)
    for k, n in enumerate("xyz"):
        a[n] = xyz[:, k]
    for k, n in enumerate(("red", "green", "blue")):
        a[n] = rgb[:, k]
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\n" + f"element vertex {xyz.shape[0]}\n".encode())
        for n, t in dt:
            f.write(f"property {'uchar' if t == 'u1' else 'float'} {n}\n".encode())
        f.write(b"end_header\n" + a.tobytes())


def test_model_from_points3d_ply_trains_one_step(exact, tmp_path):
    from fov3dgs_amd import loss_utils, model_io
    from fov3dgs_amd.gaussian_renderer import render

    P = 50_000
    xyz = syn.points_colmap_like(P, seed=12).numpy()
    rgb = np.random.default_rng(3).integers(0, 256, size=(P, 3), dtype=np.uint8)
    path = os.path.join(tmp_path, "points3D.ply")
    _store_ply(path, xyz, rgb)
    v = model_io.read_ply_vertices(path)
    pts = np.vstack([v["x"], v["y"], v["z"]]).T                          # fetchPly
    cols = np.vstack([v["red"], v["green"], v["blue"]]).T / 255.0
    cloud = model_io.cloud_from_points(pts, cols, sh_degree=3, device=DEV)

    # create_from_pcd restated in torch, fed the exact reference's dist2
    C0 = 0.28209479177387814
    fused = (torch.tensor(cols).float().to(DEV) - 0.5) / C0
    feats = torch.zeros((P, 3, 16), device=DEV)
    feats[:, :3, 0] = fused
    dist2 = torch.clamp_min(torch.from_numpy(exact(pts.astype(np.float32))).to(DEV), 0.0000001)
    want = {"_xyz": torch.tensor(pts).float().to(DEV), "_features_dc": feats[:, :, 0:1].transpose(1, 2),
            "_features_rest": feats[:, :, 1:].transpose(1, 2), "_scaling": torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3),
            "_rotation": torch.tensor([1.0, 0, 0, 0], device=DEV).expand(P, 4),
            "_opacity": torch.log(torch.full((P, 1), 0.1, device=DEV) / (1 - torch.full((P, 1), 0.1, device=DEV)))}
    for k, t in want.items():
        got = getattr(cloud, k)
        assert got.dtype == torch.float32 and got.shape == t.shape, k
        assert torch.equal(got, t), k
    assert cloud.active_sh_degree == 0 and cloud.max_sh_degree == 3

    cloud.requires_grad_(True)
    cam = syn.camera_ring(0, width=192, height=128, radius=25.0, height_above=5.0, device=DEV)

    class Pipe:
        debug = False
    out = render(cam, cloud, Pipe(), torch.zeros(3, device=DEV), cuda_type="pcheck_obb_sum")
    img = out["render"]
    assert torch.isfinite(img).all() and img.abs().sum() > 0
    gt = torch.rand(img.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    loss = loss_utils.l1_ssim_loss(img, gt)
    loss.backward()
    assert math.isfinite(loss.item())
    for name in ("_xyz", "_features_dc", "_scaling", "_rotation", "_opacity"):
        g = getattr(cloud, name).grad
        assert g is not None and torch.isfinite(g).all(), name
    rest = cloud._features_rest.grad
    assert rest is None or torch.isfinite(rest).all()
    assert cloud._xyz.grad.abs().sum() > 0 and cloud._opacity.grad.abs().sum() > 0
