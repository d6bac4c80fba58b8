"""The per-tile sort's dispatch: lists of every length at which launch_tile_sort (csrc/binning.hip) changes its path.

Two or three launches sort a frame's tile lists: k_tile_msort (one wave per list of <= 511 entries, four lists per workgroup;
256 threads per list of 512..2047), k_tile_msort_direct<512, 8> (a workgroup per list of 2048..8191 entries that picks 8 or 16
keys per thread from the list's length, in LDS that the host sizes from the frame's class counts) and, in frames that have
them, k_tile_msort_direct<1024, 16> for the lists of 8192..16383 entries; lists
of >= 16384 entries are regrouped first. The scenes (tests/tile_sort_scenes.py) put an exact number of tiny Gaussians on the
centre of chosen tiles of a 128 x 64 image (32 tiles; every Gaussian touches one tile), so that the lists sit on both sides of
every seam, and the tests compare `ranges` and `point_list` bit for bit with the CPU oracle; the expected order is also derived
a second time in numpy as the argsort on (depth bits, Gaussian index) inside every tile.

The depths here are uniform in [2, 6], or one depth per list. What depends on the DEPTH DISTRIBUTION inside a list -- the
regrouped lists' oversized chunks, the clamp bucket and the streamed split, and the interpolation sort on skewed distinct depths
-- is in test_tile_sort_depths_gpu.py (its scenes' conditions without a GPU: test_tile_sort_depths_cpu.py).
"""
import numpy as np
import pytest

from tests.tile_sort_scenes import VARIANTS, _check, _need_gpu, _oracle

pytestmark = pytest.mark.gpu

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
