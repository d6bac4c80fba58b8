"""CPU checks of the nearest-neighbour feature (simple_knn.distCUDA2, include/fovraster.h fr_knn_mean_dist2): the exact
C reference the GPU tests compare against, the module's argument checks and the host-side workspace size."""
import numpy as np
import pytest
import torch

from tests import knn_ref as R
from fov3dgs_amd import _native


@pytest.fixture(scope="module")
def exact(tmp_path_factory):
    d = tmp_path_factory.mktemp("knn_exact")
    exe = R.build_exact(d)
    return lambda pts: R.run_exact(exe, pts, d)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 100, 3000])
def test_exact_reference_equals_brute_force_uniform(exact, P):
    x = R.uniform_cloud(P, seed=P)
    a, b = exact(x), R.brute_force(x)
    assert np.array_equal(a, b)
    if P <= 2:
        assert np.all(np.isposinf(a))
    if P == 3:
        assert np.all(a >= np.float32(np.finfo(np.float32).max / 3) * np.float32(0.999999))


@pytest.mark.parametrize("name", list(R.degenerate_clouds(64).keys()))
def test_exact_reference_equals_brute_force_degenerate(exact, name):
    x = R.degenerate_clouds(3000)[name]
    a, b = exact(x), R.brute_force(x)
    assert np.array_equal(a, b)
    if name == "identical":
        assert np.all(a == 0)


def test_exact_reference_matches_ckdtree():
    spatial = pytest.importorskip("scipy.spatial")
    x = R.uniform_cloud(200_000, seed=11)
    tree = spatial.cKDTree(x.astype(np.float64))
    _, nn = tree.query(x.astype(np.float64), k=17)
    cand = x[nn]                                   # [P,17,3], self among them (or a duplicate at distance 0)
    dx = cand[:, :, 0] - x[:, None, 0]
    dy = cand[:, :, 1] - x[:, None, 1]
    dz = cand[:, :, 2] - x[:, None, 2]
    d = (dx * dx + dy * dy) + dz * dz
    d[nn == np.arange(x.shape[0])[:, None]] = np.inf
    b = np.sort(d, axis=1)[:, :3]
    want = ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3.0)
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        got = R.run_exact(R.build_exact(td), x, td)
    assert np.array_equal(got, want)


def test_distcuda2_module_exists_and_checks_arguments():
    from fov3dgs_amd.simple_knn._C import distCUDA2
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        distCUDA2(torch.zeros(8, 3))
    with pytest.raises(RuntimeError):
        distCUDA2(torch.zeros(8, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        distCUDA2(torch.zeros(8, 4))


def test_knn_workspace_bytes_is_host_computable_and_monotone():
    lib = _native.load()
    assert lib.fr_knn_workspace_bytes(0) == 0
    sizes = [lib.fr_knn_workspace_bytes(P) for P in (1, 63, 64, 65, 4095, 4096, 4097, 262145, 1_000_000, 6_000_000, 2**31 - 1)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert sizes[-3] >= 1_000_000 * 24  # the keys / values and the sorted points
    assert lib.fr_knn_mean_dist2(-1, None, None, None, None) == -1
    assert "knn" in _native.last_error()
    assert lib.fr_knn_mean_dist2(0, None, None, None, None) == 0
