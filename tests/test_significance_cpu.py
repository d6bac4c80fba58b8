"""LightGaussian's global-significance pruning, what can be checked without a GPU: the numpy replay the GPU tests compare the counting
render with (tests/significance_ref.py) against the oracle it replays; the new exports; the refusals that validation makes before
anything is launched; the shim's field list; the index arithmetic of the reference's two percentile expressions."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native, lightgaussian
from fov3dgs_amd import compress_diff_gaussian_rasterization as cdgr
from tests import significance_ref as sref
from tests.helpers import cam_dict, scene_dict, small_camera, small_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fr_select_kth", "fr_mask_le", "fr_volume", "fr_v_importance")


def scene_c():
    cloud = small_cloud(1500, 7, 0.0)
    with torch.no_grad():
        cloud._opacity += 1.0
    return scene_dict(cloud, "original"), cam_dict(small_camera(104, 72), bg=(0.1, 0.2, 0.3))


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=("fp32", "fp64"))
def test_replay_reproduces_the_oracle_it_replays(dtype):
    scene, cam = scene_c()
    rep = sref.validated(scene, cam, dtype)  # n_contrib equal, final_T to 1e-6
    hits = rep["hits"]
    assert hits.shape == (1500,) and hits.min() >= 0 and hits.sum() > 0
    # every accumulated pair is counted once: a pixel's n_contrib is the list position of its last pair, so it bounds the pixel's pairs
    assert hits.sum() <= int(rep["n_contrib"].astype(np.int64).sum())
    # a Gaussian that is in no tile list has no hits
    listed = np.zeros(1500, bool)
    listed[rep["fwd"]["point_list"]] = True
    assert not hits[~listed].any()
    if dtype is np.float32:  # the figures the GPU test's scene C was chosen by
        assert (int((hits > 0).sum()), int(hits.sum()), rep["longest"]) == (1465, 52437, 749) and rep["saturated"] > 0


def test_header_library_and_exports_carry_the_new_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fovraster.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fr_[a-z_0-9A-Z]+)\s*\(", txt))
    lib = _native.load()
    for n in NEW:
        assert n in declared and n in _native.EXPORTS and hasattr(lib, n), n
    assert lib.fr_abi_version() == _native.ABI_VERSION == 12  # (added symbols; fr_forward_args is unchanged)


def test_native_refuses_bad_arguments_without_launching():
    lib = _native.load()
    p = 4096  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails validation first

    def bad(rc, *words):
        assert rc == -1 and all(w in lib.fr_last_error() for w in words), (rc, lib.fr_last_error())
    # the counting render is ORIGINAL with BOTH statistics pointers: one alone is refused, and the message names them
    for one in ("gaussians_count", "contributions"):
        a = _native.ForwardArgs()
        a.variant, a.P, a.W, a.H, a.out_color = _native.VARIANT_ORIGINAL, 0, 16, 16, p
        setattr(a, one, p)
        bad(lib.fr_forward(C.byref(a)), b"gaussians_count", b"contributions")
        a.P = 10
        bad(lib.fr_forward(C.byref(a)), b"gaussians_count", b"contributions")
    a = _native.ForwardArgs()
    a.variant, a.P, a.W, a.H, a.out_color, a.no_stats = _native.VARIANT_ORIGINAL, 10, 16, 16, p, 1
    for f in ("means3D", "opacities", "viewmatrix", "projmatrix", "campos", "background", "radii", "shs", "scales", "rotations",
              "gaussians_count", "contributions"):
        setattr(a, f, p)
    a.M = 16
    noop = _native.RESIZE_FN(lambda user, n: None)
    a.geometry_resize = a.binning_resize = a.image_resize = noop
    bad(lib.fr_forward(C.byref(a)), b"no_stats")  # (still pcheck_obb_sum's alone)
    # select
    bad(lib.fr_select_kth(-1, p, 0, 0, p, p, None), b"P=-1")
    bad(lib.fr_select_kth(10, p, 0, -1, p, p, None), b"k=-1")
    bad(lib.fr_select_kth(10, p, 0, 10, p, p, None), b"k=10")
    bad(lib.fr_select_kth(0, p, 0, 0, p, p, None), b"k=0")  # (no element of any rank)
    bad(lib.fr_select_kth(10, p, 2, 3, p, p, None), b"dtype")
    bad(lib.fr_select_kth(10, p, -1, 3, p, p, None), b"dtype")
    bad(lib.fr_select_kth(10, p, 1, 3, p, None, None), b"null")
    bad(lib.fr_select_kth(10, None, 0, 3, p, p, None), b"null")
    bad(lib.fr_select_kth(10, p, 0, 3, None, p, None), b"null")
    bad(lib.fr_select_kth(10, p, 0, 3, p, p + 4, None), b"aligned")
    # mask, volume, score
    bad(lib.fr_mask_le(-1, p, 0, p, p, None), b"P=-1")
    bad(lib.fr_mask_le(10, p, 3, p, p, None), b"dtype")
    bad(lib.fr_mask_le(10, p, 0, None, p, None), b"null")
    bad(lib.fr_mask_le(10, p, 0, p, None, None), b"null")
    assert lib.fr_mask_le(0, None, 1, None, None, None) == 0
    bad(lib.fr_volume(-1, p, 0, p, None), b"P=-1")
    bad(lib.fr_volume(10, None, 0, p, None), b"null")
    bad(lib.fr_volume(10, p, 1, None, None), b"null")
    assert lib.fr_volume(0, None, 0, None, None) == 0
    bad(lib.fr_v_importance(-1, p, p, 0.1, p, p, None), b"P=-1")
    bad(lib.fr_v_importance(10, p, None, 0.1, p, p, None), b"null")
    bad(lib.fr_v_importance(10, p, p, 0.1, None, p, None), b"null")
    assert lib.fr_v_importance(0, None, None, 0.1, None, None, None) == 0


def test_shim_has_the_reference_settings():
    assert cdgr.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix", "sh_degree", "campos",
        "prefiltered", "debug", "f_count")
    for name in ("GaussianRasterizer", "rasterize_gaussians"):
        assert hasattr(cdgr, name), name
    rs = cdgr.GaussianRasterizationSettings(*range(12), f_count=True)
    assert rs.f_count is True and rs[12] is True and cdgr.GaussianRasterizer(rs).raster_settings is rs


@pytest.mark.parametrize("P", (1, 2, 10, 1161358))
def test_index_arithmetic_is_the_references(P):
    # prune.py:122-124: sorted_volume[int(len(volume) * 0.9)] of the DESCENDING sort = the ascending rank P - 1 - that
    asc = torch.arange(P)
    index = int(len(asc) * 0.9)
    assert 0 <= lightgaussian.volume_index(P) < P
    assert int(torch.flip(asc, (0,))[index]) == int(asc[lightgaussian.volume_index(P)])
    # gaussian_model.py:779
    for percent in (0, 0.3, 0.66, 1):
        assert lightgaussian.percentile_index(P, percent) == int(percent * (asc.shape[0] - 1))
        assert 0 <= lightgaussian.percentile_index(P, percent) <= P - 1


def test_no_cpu_fallback_and_argument_checks():
    v = torch.rand(10)
    for call in (lambda: lightgaussian.kth_value(v, 3), lambda: lightgaussian.percentile_mask(v, 0.5),
                 lambda: lightgaussian.volume_of(torch.rand(10, 3)),
                 lambda: lightgaussian.calculate_v_imp_score(None, v, 0.1, scaling=torch.rand(10, 3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="prune_type"):
        lightgaussian.global_significance_prune(None, [], None, None, 0.5, prune_type="HDBSCAN")
    assert lightgaussian.PRUNE_TYPES == ("important_score", "v_important_score", "max_v_important_score", "count", "opacity")
