"""The per-tile sort on lists whose DEPTH DISTRIBUTION is what matters (test_tile_sort_classes_gpu.py varies the lengths, with
depths uniform in [2, 6] or a wall of one depth below the split).

Frame A: the lists of >= 16384 entries, which k_split_long regroups by depth (split_list, csrc/tile_sort.h) and
k_tile_msort_chunks sorts chunk by chunk: depths over nearly all 2048 depth buckets and the clamp bucket, everything in the
clamp bucket, 20000 distinct depths in ONE bucket (one chunk, sorted by the 32768-wide bitonic network in global memory with n
no power of two), a wall of 17000 equal depths, an oversized chunk among ordinary ones, a first chunk of exactly 2048 (LDS) and
2049 (global network) keys, a thread of split_list whose two buckets both start a chunk, lists that end in the empty chunk
[n, n) (msort_list with n == 0), and the streamed form of split_list at 16385, 32768, 32769 and 33000 entries. A list of every
other class lies beside them.

Frame B: lists of 300, 1500, 3000, 6000 and 12000 entries -- one per class that a single workgroup sorts with the interpolation
sort (sort_keys_lds) --, each with a cluster of neighbouring bit patterns plus a far outlier (nearly every key in one bucket,
the hand-over to the merge sort with DISTINCT depths), with groups of 16 neighbouring bit patterns (8 <= occ <= 32: odd-even
rounds in the tens) and with two interleaved walls.

`ranges` and `point_list` equal the CPU oracle's bit for bit; the oracle's order is also derived a second time as the argsort
on (depth bits, Gaussian index). That every list reaches what it is named for is asserted on the oracle's depths first
(tests/tile_sort_scenes.py; test_tile_sort_depths_cpu.py asserts the same without a GPU).

Broken by hand once (each break only misorders valid entries): msort_list's global network skipped -> frame A fails on the six
lists with an oversized chunk, and no test of test_tile_sort_classes_gpu.py does; keys above depth_bucket's clamp sent to bucket
0 -> frame A fails on the log-uniform list alone (clamping to 2046 instead is still a monotone map: the order cannot change, and
does not); the last streamed round of split_list reading the round before it again -> frame A fails on every regrouped list;
the odd-even rounds of sort_keys_lds capped at 8 -> frame B fails, nothing else does.
"""
import pytest

from tests import tile_sort_scenes as scenes
from tests.checks import check_image
from tests.tile_sort_scenes import VARIANTS, _check, _need_gpu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", VARIANTS)
def test_frame_a_regrouped_lists(variant):
    _need_gpu()
    scene, cam, want, tile = scenes.frame_a(variant)
    empty_tail = scenes.frame_a_conditions(want, tile)
    assert empty_tail, "msort_list with n == 0 is not reached"
    got = _check(variant, scene, cam, want, tile)
    check_image(got["color"], want["color"])


@pytest.mark.parametrize("variant", VARIANTS)
def test_frame_b_skewed_lists(variant):
    _need_gpu()
    scene, cam, want, tile = scenes.frame_b(variant)
    assert len(scenes.frame_b_conditions(want, tile)) == 15
    got = _check(variant, scene, cam, want, tile)
    check_image(got["color"], want["color"])
