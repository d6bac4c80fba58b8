"""The per-tile sort's dispatch: lists of every length at which launch_tile_sort (csrc/binning.hip) changes its path.

Two or three launches sort a frame's tile lists: k_tile_msort (one wave per list of <= 511 entries, four lists per workgroup;
256 threads per list of 512..2047), k_tile_msort_direct<512, 8> (a workgroup per list of 2048..8191 entries that picks 8 or 16
keys per thread from the list's length, in LDS that the host sizes from the frame's class counts) and, in frames that have
them, k_tile_msort_direct<1024, 16> for the lists of 8192..16383 entries; lists
of >= 16384 entries are regrouped first. The scenes below put an exact number of tiny Gaussians on the centre of chosen
tiles of a 128 x 64 image (32 tiles; every Gaussian touches one tile), so that the lists sit on both sides of every seam, and
compare `ranges` and `point_list` bit for bit with the CPU oracle; the expected order is also derived a second time in numpy
as the argsort on (depth bits, Gaussian index) inside every tile.
"""
import math

import numpy as np
import pytest
import torch

from tests.helpers import cam_dict, scene_dict, syn
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

W, H = 128, 64
TILES_X, TILES_Y = W // 16, H // 16
VARIANTS = ("pcheck_obb_sum", "fov_pcheck_obb")

SEAMS = (0, 1, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384)
# frames with only some of the classes: the long kernel's LDS takes each of its sizes (8 keys per thread, 16, and the
# 1024-thread launch), and each launch is also left out once
SPARSE = {
    "short_only": (1, 100, 511, 0, 37),                    # no workgroup-per-list class at all
    "up_to_4095": (1, 513, 2049, 4095, 2048),              # long kernel with the LDS of 8 keys per thread
    "up_to_8191": (0, 511, 2048, 4097, 8191, 4096),        # ... of 16 keys per thread
    "only_8192_up": (8192, 16383, 8193),                   # the 1024-thread launch alone, no short list but the empty tiles
    "long_and_split": (16384, 8193, 2047, 16500),          # the regrouped lists beside one list of each other launch
    "one_wave_tail": (511, 300, 2, 1, 5, 512),             # 26 + 5 lists of the one-wave class: the last workgroup is not full
}


def _need_gpu():
    if not torch.cuda.is_available():  # only reached by an explicit -m gpu run (tests/conftest.py skips otherwise)
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _cloud(lengths, seed, equal_depth=()):
    """A cloud that puts lengths[t] Gaussians on tile t (row-major), all of them within 2 pixels of the tile's centre and a
    few hundredths of a pixel wide; tiles listed in equal_depth get ONE depth for all their Gaussians. The Gaussians of the
    tiles are interleaved in index order."""
    rng = np.random.default_rng(seed)
    tile = np.repeat(np.arange(len(lengths)), lengths)
    rng.shuffle(tile)
    P = tile.size
    tx, ty = tile % TILES_X, tile // TILES_X
    px = tx * 16 + 8 + rng.uniform(-2.0, 2.0, P)
    py = ty * 16 + 8 + rng.uniform(-2.0, 2.0, P)
    z = rng.uniform(2.0, 6.0, P)
    for t in equal_depth:
        z[tile == t] = 3.0 + 0.125 * t
    tan = math.tan(math.radians(60.0) * 0.5)  # syn.camera_1k: identity pose, 60 degrees both ways
    xyz = np.stack([((2 * px + 1) / W - 1) * tan * z, ((2 * py + 1) / H - 1) * tan * z, z], 1).astype(np.float32)
    g = torch.Generator().manual_seed(seed)
    rot = torch.zeros(P, 4); rot[:, 0] = 1.0
    return syn.GaussianCloud(torch.from_numpy(xyz), torch.randn(P, 1, 3, generator=g), 0.1 * torch.randn(P, 15, 3, generator=g),
                             torch.full((P, 3), math.log(1e-3)), rot, torch.full((P, 1), -2.0)), tile


def _case(variant, lengths, seed, equal_depth=()):
    lengths = list(lengths) + [0] * (TILES_X * TILES_Y - len(lengths))
    cloud, tile = _cloud(lengths, seed, equal_depth)
    fov = None
    if variant == "fov_pcheck_obb":
        # every Gaussian exists at every level with the same opacity: the level filter keeps the lists as placed
        _, shs_dcs, _ = syn.foveation_layers(cloud, seed=seed + 1)
        P = len(cloud)
        fov = (torch.full((P, 1), 3.0), shs_dcs, torch.full((P, 4), float(torch.sigmoid(torch.tensor(-2.0)))))
    scene, cam = scene_dict(cloud, variant, fov), cam_dict(syn.camera_1k(W, H))
    return scene, cam, np.asarray(lengths), tile


_WANT = {}


def _oracle(key, variant, lengths, seed, equal_depth=()):
    """The oracle's frame of a case, computed once and shared (read-only) by the tests that need it."""
    if key not in _WANT:
        scene, cam, lengths, tile = _case(variant, lengths, seed, equal_depth)
        want = orc.forward(variant, scene, cam)
        n = want["ranges"][:, 1].astype(np.int64) - want["ranges"][:, 0]
        np.testing.assert_array_equal(n, lengths)  # the scene does what it was built for
        for a in want.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _WANT[key] = (scene, cam, want, tile)
    return _WANT[key]


def _argsort_order(want, tile):
    """Second derivation of point_list: inside every tile (tiles in index order, as the ranges are laid out) the Gaussians by
    (bits of the view depth, index)."""
    bits = want["depths"].astype(np.float32).view(np.uint32).astype(np.uint64)
    key = bits << np.uint64(32) | np.arange(tile.size, dtype=np.uint64)
    order = np.lexsort((key, tile))  # tile first, then the 64-bit key
    return order.astype(np.uint32)


def _check(variant, scene, cam, want, tile):
    from tests.gpu_helpers import hip_forward
    got = hip_forward(variant, scene, cam)
    assert got["num_rendered"] == want["num_rendered"] == tile.size
    np.testing.assert_array_equal(got["ranges"], want["ranges"])
    np.testing.assert_array_equal(want["point_list"], _argsort_order(want, tile))
    np.testing.assert_array_equal(got["point_list"], want["point_list"])
    # and as a training frame launches it: the counts through the pinned totals block, the short lists' kernel on the helper
    # stream beside the long lists' (debug mode above keeps everything on one stream and copies the counts)
    got = hip_forward(variant, scene, cam, debug=False)
    np.testing.assert_array_equal(got["ranges"], want["ranges"])
    np.testing.assert_array_equal(got["point_list"], want["point_list"])


@pytest.mark.parametrize("variant", VARIANTS)
def test_mixed_frame_has_a_list_at_every_seam(variant):
    _need_gpu()
    # the seam lengths on tiles 0..15 in a scrambled order (tile_order is by length, not by tile), a few ordinary lists behind them
    lengths = list(np.random.default_rng(5).permutation(SEAMS)) + [100, 700, 3000, 0, 40, 1500, 5, 0, 64, 1024, 0, 9, 6000, 0, 0, 250]
    _check(variant, *_oracle(("mixed", variant), variant, lengths, seed=11))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("frame", sorted(SPARSE))
def test_sparse_frame(frame, variant):
    _need_gpu()
    _check(variant, *_oracle((frame, variant), variant, SPARSE[frame], seed=23))


@pytest.mark.parametrize("variant", VARIANTS)
def test_lists_of_one_depth(variant):
    """Every entry of a tile at ONE depth (far more than FR_BUCKET_SORT_MAX_OCC = 40 equal keys in a bucket): the interpolation
    sort hands over to the merge passes, in each branch of the two kernels; the order is the Gaussian index's."""
    _need_gpu()
    lengths = (300, 41, 1500, 3000, 6000, 9000, 2048, 511, 700)
    scene, cam, want, tile = _oracle(("walls", variant), variant, lengths, seed=31, equal_depth=(0, 1, 2, 3, 4, 5, 6, 7))
    for t in range(8):
        assert np.unique(want["depths"][tile == t]).size == 1
    _check(variant, scene, cam, want, tile)
