"""Scenes of the per-tile sort's tests: an exact number of tiny Gaussians on the centre of chosen tiles of a 128 x 64 image
(32 tiles; every Gaussian touches one tile), seen by the identity camera, so that a tile's list has a chosen length and --
the view depth of a Gaussian is its z bit for bit -- chosen float32 depths.

test_tile_sort_classes_gpu.py varies the LENGTHS (every seam of launch_tile_sort's dispatch); test_tile_sort_depths_cpu.py /
_gpu.py vary the DEPTH DISTRIBUTION inside a list (frames A and B below). The conditions that show that a frame reaches the
code it was built for are functions of the ORACLE's depths, restated in numpy from what csrc/tile_sort.h documents:
depth_bucket and the chunk rule of split_list, and the bucket width of sort_keys_lds.
"""
import math

import numpy as np
import pytest
import torch

from tests.helpers import cam_dict, scene_dict, syn
from oracle import oracle as orc

W, H = 128, 64
TILES_X, TILES_Y = W // 16, H // 16
VARIANTS = ("pcheck_obb_sum", "fov_pcheck_obb")


def _need_gpu():
    if not torch.cuda.is_available():  # only reached by an explicit -m gpu run (tests/conftest.py skips otherwise)
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _cloud(lengths, seed, equal_depth=(), depths=None):
    """A cloud that puts lengths[t] Gaussians on tile t (row-major), all of them within 2 pixels of the tile's centre and a
    few hundredths of a pixel wide; tiles listed in equal_depth get ONE depth for all their Gaussians, tiles that are keys of
    `depths` get depths[t][j] (float32) for their j-th Gaussian in index order, the others uniform depths in [2, 6]. The
    Gaussians of the tiles are interleaved in index order."""
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
    for t, d in (depths or {}).items():
        d = np.asarray(d)
        assert d.dtype == np.float32 and d.shape == (lengths[t],)
        z[tile == t] = d  # float32 -> float64 -> float32 below: the bit pattern survives
    tan = math.tan(math.radians(60.0) * 0.5)  # syn.camera_1k: identity pose, 60 degrees both ways
    xyz = np.stack([((2 * px + 1) / W - 1) * tan * z, ((2 * py + 1) / H - 1) * tan * z, z], 1).astype(np.float32)
    g = torch.Generator().manual_seed(seed)
    rot = torch.zeros(P, 4); rot[:, 0] = 1.0
    return syn.GaussianCloud(torch.from_numpy(xyz), torch.randn(P, 1, 3, generator=g), 0.1 * torch.randn(P, 15, 3, generator=g),
                             torch.full((P, 3), math.log(1e-3)), rot, torch.full((P, 1), -2.0)), tile


def _case(variant, lengths, seed, equal_depth=(), depths=None):
    lengths = list(lengths) + [0] * (TILES_X * TILES_Y - len(lengths))
    cloud, tile = _cloud(lengths, seed, equal_depth, depths)
    fov = None
    if variant == "fov_pcheck_obb":
        # every Gaussian exists at every level with the same opacity: the level filter keeps the lists as placed
        _, shs_dcs, _ = syn.foveation_layers(cloud, seed=seed + 1)
        P = len(cloud)
        fov = (torch.full((P, 1), 3.0), shs_dcs, torch.full((P, 4), float(torch.sigmoid(torch.tensor(-2.0)))))
    scene, cam = scene_dict(cloud, variant, fov), cam_dict(syn.camera_1k(W, H))
    return scene, cam, np.asarray(lengths), tile


_WANT = {}


def _oracle(key, variant, lengths, seed, equal_depth=(), depths=None):
    """The oracle's frame of a case, computed once and shared (read-only) by the tests that need it."""
    if key not in _WANT:
        scene, cam, lengths, tile = _case(variant, lengths, seed, equal_depth, depths)
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
    """-> the frame of the first (debug) run, for what a caller compares beyond the lists."""
    from tests.gpu_helpers import hip_forward
    first = got = hip_forward(variant, scene, cam)
    assert got["num_rendered"] == want["num_rendered"] == tile.size
    np.testing.assert_array_equal(got["ranges"], want["ranges"])
    np.testing.assert_array_equal(want["point_list"], _argsort_order(want, tile))
    np.testing.assert_array_equal(got["point_list"], want["point_list"])
    # and as a training frame launches it: the counts through the pinned totals block, the short lists' kernel on the helper
    # stream beside the long lists' (debug mode above keeps everything on one stream and copies the counts)
    got = hip_forward(variant, scene, cam, debug=False)
    np.testing.assert_array_equal(got["ranges"], want["ranges"])
    np.testing.assert_array_equal(got["point_list"], want["point_list"])
    return first


# ---- what csrc/tile_sort.h documents, in numpy -------------------------------------------------------------------------
FINE_BUCKETS, CHUNK_TARGET, CHUNK_LDS_KEYS = 2048, 960, 2048  # k_tile_msort_chunks<256, 8>: 2048 keys fit its LDS
BUCKET_SORT_MAX_OCC = 40


def _bits(depths):
    d = np.ascontiguousarray(depths, np.float32)
    assert (d > 0).all()  # the bit pattern of a positive float orders like its value
    return d.view(np.uint32).astype(np.int64)


def depth_bucket(depths):
    """split_list's depth bucket: 128 per octave from 0.2 up, the rest clamped into the last one."""
    return np.minimum(FINE_BUCKETS - 1, np.maximum(0, _bits(depths) - 0x3E4CCCCD) >> 16)


def split_chunks(depths):
    """-> (entries per depth bucket, chunk lengths in depth order) of a long list: a chunk starts at bucket 0 and at every bucket
    whose exclusive offset is in another multiple of 960 than the previous bucket's; the last chunk ends at n."""
    counts = np.bincount(depth_bucket(depths), minlength=FINE_BUCKETS)
    excl = np.cumsum(counts) - counts
    first = np.ones(FINE_BUCKETS, bool)
    first[1:] = excl[1:] // CHUNK_TARGET != excl[:-1] // CHUNK_TARGET
    return counts, np.diff(np.append(excl[first], len(depths)))


def interpolation_width(depths, capacity):
    """Depth bit patterns per bucket of sort_keys_lds: (dmax - dmin + 1) / NB, NB = twice the capacity of the list's class."""
    b = _bits(depths)
    return (int(b.max()) - int(b.min()) + 1) / (2 * capacity)


def f32_from_bits(bits):
    return np.asarray(bits, np.int64).astype(np.uint32).view(np.float32)


BITS_2, BITS_3 = 0x40000000, 0x40400000  # 2.0f, 3.0f


# ---- frame A: the lists that are regrouped by depth (>= 16384 entries) ---------------------------------------------------
def _frame_a():
    rng = np.random.default_rng(101)
    f32 = np.float32

    def mixed(*parts):
        d = np.concatenate([np.asarray(p, f32) for p in parts])
        rng.shuffle(d)
        return d

    lists = [
        # (name, length, depths or None = uniform in [2, 6])
        ("log_uniform", 40000, np.clip(np.exp(rng.uniform(math.log(0.21), math.log(30000.0), 40000)), 0.21, 30000.0).astype(f32)),
        ("one_bucket_distinct", 20000, f32_from_bits(BITS_3 + rng.permutation(41943)[:20000])),  # 3.0 .. 3.01, no two alike
        ("wall", 17000, np.full(17000, 3.5, f32)),
        ("wall_inside", 20000, mixed(rng.uniform(2.0, 6.0, 15000), np.full(5000, 4.25))),
        ("clamped", 18000, rng.uniform(14000.0, 60000.0, 18000).astype(f32)),
        ("uniform_16385", 16385, None),
        ("uniform_32768", 32768, None),
        ("uniform_32769", 32769, None),
        ("uniform_33000", 33000, None),
        ("first_chunk_2048", 2048 + 15000, mixed(np.full(2048, 2.0), rng.uniform(2.5, 6.0, 15000))),
        ("first_chunk_2049", 2049 + 15000, mixed(np.full(2049, 2.0), rng.uniform(2.5, 6.0, 15000))),
        # 1000 keys in each of the depth buckets 435 (2.0 is its 13107th bit pattern) and 436: one thread's two buckets
        ("two_starts", 2000 + 15000, mixed(np.full(1000, f32_from_bits(BITS_2 + 52428)), np.full(1000, f32_from_bits(BITS_2 + 52429)),
                                           rng.uniform(2.5, 6.0, 15000))),
        # one list of every other class beside them: the frame launches every sort kernel
        ("class_1024x16", 8193, None), ("class_512x16", 5000, None), ("class_512x8", 2100, None), ("class_256", 2047, None),
        ("class_wave", 300, None),
    ]
    names = [l[0] for l in lists]
    return names, [l[1] for l in lists], {t: l[2] for t, l in enumerate(lists) if l[2] is not None}


A_NAMES, A_LENGTHS, A_DEPTHS = _frame_a()
A_OVERSIZED = ("log_uniform", "one_bucket_distinct", "wall", "wall_inside", "clamped", "first_chunk_2049")
A_CLAMPED = ("log_uniform", "clamped")
A_UNIFORM = ("uniform_16385", "uniform_32768", "uniform_32769", "uniform_33000")


def frame_a(variant):
    return _oracle(("depths_a", variant), variant, A_LENGTHS, seed=41, depths=A_DEPTHS)


def frame_a_conditions(want, tile):
    """The oracle's depths put every list of frame A on the path it is named for."""
    d = {name: np.asarray(want["depths"])[tile == t] for t, name in enumerate(A_NAMES)}
    split = {name: split_chunks(d[name]) for name in A_NAMES if d[name].size >= 16384}
    assert set(A_OVERSIZED + A_UNIFORM + ("first_chunk_2048", "two_starts")) == set(split)
    for name, (counts, chunks) in split.items():
        assert chunks.sum() == d[name].size and (chunks[:-1] > 0).all(), name
    for name in A_OVERSIZED:  # a bucket is never cut: its chunk is sorted by the network in global memory
        assert split[name][0].max() > CHUNK_LDS_KEYS and split[name][1].max() > CHUNK_LDS_KEYS, name
    for name in A_CLAMPED:
        assert split[name][0][FINE_BUCKETS - 1] > CHUNK_LDS_KEYS, name
    assert (split["clamped"][0][:FINE_BUCKETS - 1] == 0).all()
    assert (split["log_uniform"][0] > 0).sum() >= 2000
    # ordinary chunks beside the oversized ones
    assert ((split["log_uniform"][1] > 0) & (split["log_uniform"][1] <= CHUNK_LDS_KEYS)).sum() >= 30
    c = split["wall_inside"][1]
    big = int(np.argmax(c))
    assert c[big] >= 5000 and 0 < big < len(c) - 1 and (np.delete(c, big) <= CHUNK_LDS_KEYS).all()
    assert np.unique(d["one_bucket_distinct"]).size == 20000 and (split["one_bucket_distinct"][0] > 0).sum() == 1
    assert np.unique(d["wall"]).size == 1
    assert split["first_chunk_2048"][1][0] == 2048 and split["first_chunk_2048"][1].max() == 2048
    assert split["first_chunk_2049"][1][0] == 2049 and np.sort(split["first_chunk_2049"][1])[-2] <= CHUNK_LDS_KEYS
    for name in A_UNIFORM:
        assert split[name][1].max() <= CHUNK_LDS_KEYS, name
    # split_list emits the chunk [n, n) when the count crosses a multiple of 960 at the list's last entry: msort_list with n == 0
    empty_tail = [name for name, (_, chunks) in split.items() if chunks[-1] == 0]
    assert empty_tail, "no list of frame A ends in an empty chunk"
    # a thread of split_list owns buckets 2 i and 2 i + 1: both start a chunk somewhere
    starts = {name: np.flatnonzero(np.diff((np.cumsum(cn) - cn) // CHUNK_TARGET, prepend=-1)) for name, (cn, _) in split.items()}
    s = starts["two_starts"]
    assert ((s[1:] == s[:-1] + 1) & (s[:-1] % 2 == 0)).any(), "no thread starts two chunks"
    assert split["two_starts"][1].max() <= CHUNK_LDS_KEYS
    return empty_tail


# ---- frame B: skewed depths in the classes that one workgroup sorts ------------------------------------------------------
B_CLASSES = ((300, 64 * 8), (1500, 256 * 8), (3000, 512 * 8), (6000, 512 * 16), (12000, 1024 * 16))  # (length, capacity)
B_DESIGNS = ("outlier", "groups", "two_walls")


def _frame_b():
    rng = np.random.default_rng(202)
    lengths, depths = [], {}
    for n, _ in B_CLASSES:
        # a cluster of n - 1 neighbouring bit patterns from 3.0 up, shuffled over the indices, and one key at 900.0
        d = f32_from_bits(BITS_3 + rng.permutation(n - 1))
        outlier = np.insert(d, int(rng.integers(n)), np.float32(900.0))
        # groups of 16 neighbouring bit patterns, 2^16 bit patterns from one group's start to the next's
        j = rng.permutation(n)
        groups = f32_from_bits(BITS_2 + (j // 16 << 16) + j % 16)
        # two walls, interleaved in index order, the far one first
        walls = np.where(np.arange(n) % 2 == 0, np.float32(5.0), np.float32(3.0)).astype(np.float32)
        for d in (outlier, groups, walls):
            depths[len(lengths)] = d
            lengths.append(n)
    return lengths, depths


B_LENGTHS, B_DEPTHS = _frame_b()


def frame_b(variant):
    return _oracle(("depths_b", variant), variant, B_LENGTHS, seed=43, depths=B_DEPTHS)


def frame_b_conditions(want, tile):
    """The oracle's depths give sort_keys_lds the fullest bucket (`occ`) every design of frame B is named for. -> {(length,
    design): (lower, upper) bound of occ}."""
    occ = {}
    for c, (n, cap) in enumerate(B_CLASSES):
        d = {name: np.asarray(want["depths"])[tile == 3 * c + k] for k, name in enumerate(B_DESIGNS)}
        assert all(v.size == n <= cap for v in d.values()) and (cap == 64 * 8 or n > cap // 2)  # the class of this length
        # design 1: the cluster is n - 1 distinct neighbouring bit patterns, the range is the outlier's. The kernel's bucket
        # index is monotone in the depth, so the cluster fills consecutive buckets from 0 to at most floor(2 (n - 2) / w):
        # the factor 2 is the margin for the float rounding of the index
        b = np.sort(_bits(d["outlier"]))
        w = interpolation_width(d["outlier"], cap)
        assert b[-1] == _bits(np.float32(900.0)) and (np.diff(b[:-1]) == 1).all() and b[0] == BITS_3
        buckets = math.floor(2 * (n - 2) / w) + 1
        occ[n, "outlier"] = (math.ceil((n - 1) / buckets), n - 1)
        if n <= 3000:
            # the whole cluster inside ONE bucket's width (from 6000 up a bucket of this range is narrower than n - 1 neighbouring
            # bit patterns: the cluster takes a few buckets, thousands of keys each)
            assert n - 1 < w and occ[n, "outlier"][0] >= (n - 1) / 2
        assert occ[n, "outlier"][0] > BUCKET_SORT_MAX_OCC
        # design 2: a group (16 bit patterns) falls into at most two buckets, a bucket meets at most two groups
        b = np.sort(_bits(d["groups"]))
        w = interpolation_width(d["groups"], cap)
        np.testing.assert_array_equal(b, BITS_2 + (np.arange(n) // 16 << 16) + np.arange(n) % 16)
        assert 32 <= w and 2 * w <= 1 << 16
        occ[n, "groups"] = (8, 32)
        assert 2 < occ[n, "groups"][0] and occ[n, "groups"][1] <= BUCKET_SORT_MAX_OCC
        # design 3: index order disagrees with depth order at every other key
        v = d["two_walls"]
        assert (v[0::2] == 5.0).all() and (v[1::2] == 3.0).all()
        occ[n, "two_walls"] = (n // 2, n // 2)
        assert n // 2 > BUCKET_SORT_MAX_OCC
    return occ
