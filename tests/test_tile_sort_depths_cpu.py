"""The scenes of test_tile_sort_depths_gpu.py do what they were built for: on the oracle's frame alone (nothing here runs the
library), every list has its designed length and depths, the oracle's own order is the argsort on (depth bits, index), and the
depths put every list on the path of the sort it is named for (tests/tile_sort_scenes.py: frame_a_conditions, frame_b_conditions).
"""
import numpy as np
import pytest

from tests import tile_sort_scenes as scenes
from tests.tile_sort_scenes import VARIANTS, _argsort_order


def _designed(scene, want, tile, lengths, depths):
    # identity pose: the view depth is z bit for bit, so the designed bit patterns are the sort's keys
    np.testing.assert_array_equal(want["depths"], scene["means3D"][:, 2])
    for t, d in depths.items():
        np.testing.assert_array_equal(np.asarray(want["depths"])[tile == t].view(np.uint32), d.view(np.uint32))
    assert want["num_rendered"] == tile.size == sum(lengths)  # (the ranges' lengths: asserted by _oracle)
    np.testing.assert_array_equal(want["point_list"], _argsort_order(want, tile))


@pytest.mark.parametrize("variant", VARIANTS)
def test_frame_a_reaches_the_regroup_paths(variant):
    scene, cam, want, tile = scenes.frame_a(variant)
    _designed(scene, want, tile, scenes.A_LENGTHS, scenes.A_DEPTHS)
    empty_tail = scenes.frame_a_conditions(want, tile)
    assert "wall" in empty_tail  # one bucket: the chunks are [0, n) and [n, n)
    # the streamed form of split_list: more than 16 x 1024 keys; 32768 is the last length of two rounds
    n = dict(zip(scenes.A_NAMES, scenes.A_LENGTHS))
    assert n["uniform_16385"] == 16 * 1024 + 1 and n["uniform_32768"] == 2 * 16 * 1024 and n["uniform_32769"] == 2 * 16 * 1024 + 1
    # every launch of launch_tile_sort: one wave, 256 threads, <512, 8> with both capacities, <1024, 16>, the split
    for lo, hi in ((1, 512), (512, 2048), (2048, 4096), (4096, 8192), (8192, 16384), (16384, 1 << 30)):
        assert any(lo <= v < hi for v in scenes.A_LENGTHS), (lo, hi)


@pytest.mark.parametrize("variant", VARIANTS)
def test_frame_b_skews_every_one_workgroup_class(variant):
    scene, cam, want, tile = scenes.frame_b(variant)
    _designed(scene, want, tile, scenes.B_LENGTHS, scenes.B_DEPTHS)
    occ = scenes.frame_b_conditions(want, tile)
    assert len(occ) == 15
    for (n, design), (lo, hi) in occ.items():
        # hand-over to the merge sort, or odd-even rounds in the tens: never the 2..8 of a uniform list
        assert lo > scenes.BUCKET_SORT_MAX_OCC or 8 <= lo <= hi <= scenes.BUCKET_SORT_MAX_OCC, (n, design)


def test_chunk_rule_on_hand_made_lists():
    """The numpy restatement of depth_bucket and of the chunk rule on lists small enough to do by hand."""
    f = scenes.f32_from_bits
    np.testing.assert_array_equal(scenes.depth_bucket(f([0x3E4CCCCD, 0x3E4CCCCD + 65535, 0x3E4CCCCD + 65536])), [0, 0, 1])
    np.testing.assert_array_equal(scenes.depth_bucket(np.float32([0.1, 0.2, 0.4, 13000.0, 13200.0, 1e30])), [0, 0, 128, 2046, 2047, 2047])
    # 959 keys in bucket 128, 1 in bucket 256, 960 in bucket 384: the count reaches 960 at bucket 384's start, 1920 at the end
    counts, chunks = scenes.split_chunks(np.float32([0.4] * 959 + [0.8] + [1.6] * 960))
    assert counts[128] == 959 and counts[256] == 1 and counts[384] == 960
    np.testing.assert_array_equal(chunks, [960, 960, 0])
    counts, chunks = scenes.split_chunks(np.float32([0.4] * 959 + [1.6] * 960))
    np.testing.assert_array_equal(chunks, [1919, 0])  # no bucket is cut: the crossing is seen behind the last key
    counts, chunks = scenes.split_chunks(np.float32([0.4] * 400 + [1.6] * 400))
    np.testing.assert_array_equal(chunks, [800])
