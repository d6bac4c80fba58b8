"""ctypes binding of libfovraster_hip.so (C ABI declared in include/fovraster.h).

There is NO CPU fallback: if the HIP library is missing or cannot be loaded, every rasterizer
call raises. Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C fov-3dgs_amd/csrc``.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# (FOVRASTER_LIB: an experiment build of the library, tools/ab_build.sh -- never a different implementation: same ABI check)
LIB_PATH = os.environ.get("FOVRASTER_LIB") or os.path.join(HERE, "libfovraster_hip.so")
ABI_VERSION = 12

VARIANT_ORIGINAL, VARIANT_PCHECK_OBB_SUM, VARIANT_PCHECK_OBB, VARIANT_FOV_PCHECK_OBB = 0, 1, 2, 3
VARIANT_PCHECK_OBB_MAX, VARIANT_PCHECK_OBB_LWMC, VARIANT_NAIVE_FOV_PCHECK_OBB, VARIANT_MMFR_PCHECK_OBB = 4, 5, 6, 7
STAGES = ("tile_levels", "project", "bin", "tile_scan", "emit", "tile_sort", "render")
NUM_STAGE_EVENTS = len(STAGES) + 1
VARIANT_IDS = {"original": 0, "pcheck_obb_sum": 1, "pcheck_obb": 2, "fov_pcheck_obb": 3, "pcheck_obb_max": 4,
               "pcheck_obb_loss_weighted_max_count": 5, "naive_pcheck_obb": 6, "mmfr_pcheck_obb": 7}

RESIZE_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)

_FP = C.c_void_p  # device pointers are passed as raw addresses


class ForwardArgs(C.Structure):
    _fields_ = [
        ("variant", C.c_int32), ("P", C.c_int32), ("D", C.c_int32), ("M", C.c_int32),
        ("W", C.c_int32), ("H", C.c_int32), ("prefiltered", C.c_int32), ("debug", C.c_int32),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
        ("gaze_x", C.c_float), ("gaze_y", C.c_float), ("alpha", C.c_float),
        ("stream", C.c_void_p),
        ("background", _FP), ("means3D", _FP), ("shs", _FP), ("colors_precomp", _FP), ("opacities", _FP),
        ("scales", _FP), ("rotations", _FP), ("cov3D_precomp", _FP), ("viewmatrix", _FP), ("projmatrix", _FP),
        ("campos", _FP), ("shs_dcs", _FP), ("highest_levels", _FP),
        ("out_color", _FP), ("radii", _FP), ("gaussians_count", _FP), ("contributions", _FP),
        ("geometry_resize", RESIZE_FN), ("binning_resize", RESIZE_FN), ("image_resize", RESIZE_FN),
        ("resize_user", C.c_void_p * 3),
        ("num_rendered", C.c_int32), ("max_tile_instances", C.c_int32),
        ("stage_events", C.POINTER(C.c_void_p)),
        ("loss_map", _FP),
        ("shs_rest", _FP),
        ("packed_geom", _FP), ("packed_colour", _FP), ("packed_cull", _FP),
        ("cur_level", C.c_float),
        ("raw_activations", C.c_int32),
        ("num_candidates", C.c_int32),
        ("list_consumed", _FP),
        ("no_stats", C.c_int32),
        ("blend_pairs", _FP),
        ("no_helper_streams", C.c_int32),
    ]


class ForwardExt(C.Structure):
    """fr_forward_ext: optional outputs of fr_forward_begin_ext / fr_forward_ext_call"""
    _fields_ = [("size", C.c_uint32), ("visibility", _FP)]


class ForwardAux(C.Structure):
    """fr_forward_aux: the per-pixel depth / coverage planes of fr_forward_begin_aux / fr_forward_aux_call (both [H*W] float32)"""
    _fields_ = [("size", C.c_uint32), ("depth", _FP), ("coverage", _FP)]


class Foveation(C.Structure):
    """fr_foveation: the layer count and display geometry of one foveated call (fr_forward_begin_fov / fr_forward_fov_call)"""
    _fields_ = [("size", C.c_uint32), ("levels", C.c_int32), ("max_pooling_size", C.c_float), ("real_image_width", C.c_float),
                ("real_viewing_distance", C.c_float), ("start_blend", C.c_float), ("blend_width", C.c_float)]


class FovState(C.Structure):
    """fr_fov_state: what the state-keeping foveated forward (fr_forward_begin_fov_keep) leaves for fr_backward_fov_appearance"""
    _fields_ = [("size", C.c_uint32), ("variant", C.c_int32), ("P", C.c_int32), ("W", C.c_int32), ("H", C.c_int32),
                ("levels", C.c_int32), ("num_rendered", C.c_int32), ("num_items", C.c_int32),
                ("start_blend", C.c_float), ("blend_width", C.c_float),
                ("geometry", C.c_void_p), ("binning", C.c_void_p), ("image", C.c_void_p)]


class BackwardFovArgs(C.Structure):
    """fr_backward_fov_args"""
    _fields_ = [("size", C.c_uint32), ("debug", C.c_int32), ("state", C.POINTER(FovState)),
                ("background", _FP), ("dL_dpix", _FP), ("dL_dopacities", _FP), ("dL_dshs_dcs", _FP), ("dL_dlevel_colours", _FP),
                ("stream", C.c_void_p), ("stage_events", C.POINTER(C.c_void_p)), ("blend_pairs", _FP)]


class BackwardFovFullArgs(C.Structure):
    """fr_backward_fov_full_args"""
    _fields_ = [("size", C.c_uint32), ("debug", C.c_int32), ("state", C.POINTER(FovState)),
                ("P", C.c_int32), ("M", C.c_int32), ("sh_degree", C.c_int32),
                ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
                ("means3D", _FP), ("scales", _FP), ("rotations", _FP), ("shs_rest", _FP),
                ("viewmatrix", _FP), ("projmatrix", _FP), ("campos", _FP), ("background", _FP), ("dL_dpix", _FP),
                ("dL_dopacities", _FP), ("dL_dshs_dcs", _FP), ("dL_dlevel_colours", _FP),
                ("dL_dshs_rest", _FP), ("dL_dmeans3D", _FP), ("dL_dscales", _FP), ("dL_drotations", _FP), ("dL_dmeans2D", _FP),
                ("dL_dconic", _FP),
                ("stream", C.c_void_p), ("stage_events", C.POINTER(C.c_void_p)), ("blend_pairs", _FP)]


class BackwardArgs(C.Structure):
    _fields_ = [
        ("variant", C.c_int32), ("P", C.c_int32), ("D", C.c_int32), ("M", C.c_int32), ("R", C.c_int32),
        ("W", C.c_int32), ("H", C.c_int32), ("debug", C.c_int32),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
        ("stream", C.c_void_p),
        ("background", _FP), ("means3D", _FP), ("shs", _FP), ("colors_precomp", _FP), ("opacities", _FP),
        ("scales", _FP), ("rotations", _FP), ("cov3D_precomp", _FP), ("viewmatrix", _FP), ("projmatrix", _FP),
        ("campos", _FP),
        ("radii", _FP), ("geometry", _FP), ("binning", _FP), ("image", _FP), ("dL_dpix", _FP),
        ("dL_dmean2D", _FP), ("dL_dconic", _FP), ("dL_dopacity", _FP), ("dL_dcolor", _FP), ("dL_dmean3D", _FP),
        ("dL_dcov3D", _FP), ("dL_dsh", _FP), ("dL_dscale", _FP), ("dL_drot", _FP),
        ("stage_events", C.POINTER(C.c_void_p)),
        ("shs_rest", _FP),
        ("dL_dsh_rest", _FP),
        ("raw_activations", C.c_int32),
        ("row_sparse", C.c_int32),
        ("blend_pairs", _FP),
        ("outputs_zeroed", C.c_int32),
        ("num_ranges", C.c_int32),
        ("range_done", C.c_void_p),   # RANGE_FN, set through ctypes.cast (a NULL function pointer is the default)
        ("range_user", C.c_void_p),
    ]


RANGE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32, C.c_int32)  # fr_backward_args.range_done(user, k, row_lo, row_hi)


class LpipsArgs(C.Structure):
    """fr_lpips_args"""
    _fields_ = [("size", C.c_uint32), ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("debug", C.c_int32),
                ("x", _FP), ("y", _FP), ("packed", _FP), ("workspace", _FP), ("out", _FP), ("out_taps", _FP),
                ("out_features", _FP * 5), ("stream", C.c_void_p), ("stage_events", C.POINTER(C.c_void_p))]


class LpipsKeepArgs(C.Structure):
    """fr_lpips_keep_args"""
    _fields_ = [("size", C.c_uint32), ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("debug", C.c_int32),
                ("x", _FP), ("y", _FP), ("packed", _FP), ("workspace", _FP), ("keep", _FP), ("out", _FP), ("out_taps", _FP),
                ("stream", C.c_void_p), ("stage_events", C.POINTER(C.c_void_p))]


class LpipsBackwardArgs(C.Structure):
    """fr_lpips_backward_args"""
    _fields_ = [("size", C.c_uint32), ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("debug", C.c_int32),
                ("packed_backward", _FP), ("keep", _FP), ("workspace", _FP), ("grad_out", _FP), ("grad_x", _FP),
                ("stream", C.c_void_p), ("stage_events", C.POINTER(C.c_void_p))]


ADAM_MAX_TENSORS = 16
ADAM_DENSE, ADAM_EXACT, ADAM_LAZY = 0, 1, 2


class AdamTensor(C.Structure):
    _fields_ = [
        ("param", _FP), ("exp_avg", _FP), ("exp_avg_sq", _FP), ("grad", _FP), ("rows", _FP), ("row_map", _FP),
        ("numel", C.c_int64), ("n_rows", C.c_int64), ("width", C.c_int32), ("mode", C.c_int32),
        ("one_minus_beta1", C.c_float), ("beta2", C.c_float), ("one_minus_beta2", C.c_float),
        ("bias_correction2_sqrt", C.c_float), ("eps", C.c_float), ("neg_step_size", C.c_float),
    ]


class AdamArgs(C.Structure):
    _fields_ = [("num_tensors", C.c_int32), ("reserved", C.c_int32), ("tensors", AdamTensor * ADAM_MAX_TENSORS)]


COMPACT_MAX_TENSORS = 32
PRUNE_MAX_COMP_EFFICIENCY, PRUNE_CONTRIB = 0, 1


class CompactTensor(C.Structure):
    _fields_ = [("src", _FP), ("dst", _FP), ("row_words", C.c_int32), ("dst_rows", C.c_int32)]


class CompactArgs(C.Structure):
    _fields_ = [("P", C.c_int32), ("num_tensors", C.c_int32), ("invert", C.c_int32), ("reserved", C.c_int32),
                ("mask", _FP), ("workspace", _FP), ("tensors", CompactTensor * COMPACT_MAX_TENSORS)]


DENSIFY_CLONE_MASK, DENSIFY_SPLIT_MASK, DENSIFY_CLONE_GRAD, DENSIFY_SPLIT_GRAD, DENSIFY_AND_PRUNE = 0, 1, 2, 3, 4
DENSIFY_COPY, DENSIFY_ZERO_NEW, DENSIFY_XYZ, DENSIFY_SCALING = 0, 1, 2, 3


class DensifyPlanArgs(C.Structure):
    _fields_ = [("P", C.c_int32), ("mode", C.c_int32), ("N", C.c_int32), ("use_world_size", C.c_int32),
                ("n_grad", C.c_int32), ("reserved", C.c_int32),
                ("max_grad", C.c_float), ("min_opacity", C.c_float), ("t_dense", C.c_float), ("t_world", C.c_float),
                ("accum", _FP), ("denom", _FP), ("scaling", _FP), ("opacity", _FP), ("mask", _FP),
                ("counts_out", _FP), ("workspace", _FP)]


class DensifyTensor(C.Structure):
    _fields_ = [("src", _FP), ("dst", _FP), ("row_words", C.c_int32), ("role", C.c_int32)]


class DensifyRowsArgs(C.Structure):
    _fields_ = [("P", C.c_int32), ("N", C.c_int32), ("num_tensors", C.c_int32), ("reserved", C.c_int32),
                ("n_keep", C.c_int32), ("n_clone", C.c_int32), ("n_split", C.c_int32), ("n_child", C.c_int32),
                ("scaling", _FP), ("rotation", _FP), ("noise", _FP), ("workspace", _FP),
                ("tensors", DensifyTensor * COMPACT_MAX_TENSORS)]


EXPORTS = ("fr_abi_version", "fr_last_error", "fr_event_create", "fr_event_destroy", "fr_event_elapsed_ms", "fr_forward", "fr_backward", "fr_mark_visible", "fr_pack_geom", "fr_pack_colour", "fr_pack_cull", "fr_activate_forward", "fr_activate_backward", "fr_l1_ssim_blocks", "fr_l1_ssim_forward", "fr_l1_ssim_finish", "fr_l1_ssim_backward",
           "fr_geometry_bytes", "fr_image_bytes", "fr_binning_bytes", "fr_image_ranges",
           "fr_binning_point_list", "fr_image_final_T", "fr_image_n_contrib", "fr_image_tile_levels", "fr_geometry_records",
           "fr_geometry_vis_list", "fr_geometry_vis_count", "fr_geometry_walk_records", "fr_geometry_level_colours",
           "fr_geometry_level_ranges", "fr_forward_begin", "fr_forward_finish", "fr_forward_abandon", "fr_backward_prefill",
           "fr_knn_workspace_bytes", "fr_knn_mean_dist2", "fr_adam_step",
           "fr_prune_workspace_bytes", "fr_prune_metric_max", "fr_prune_select_lowest", "fr_compact_plan", "fr_compact_rows",
           "fr_densify_workspace_bytes", "fr_densify_stats", "fr_densify_plan", "fr_densify_rows",
           "fr_forward_begin_ext", "fr_forward_ext_call", "fr_backward_appearance",
           "fr_forward_begin_fov", "fr_forward_fov_call", "fr_geometry_bytes_fov", "fr_geometry_level_colours_hi", "fr_pack_colour_fov",
           "fr_hvs_workspace_floats", "fr_hvs_forward", "fr_hvs_backward",
           "fr_hvs_forward_resized", "fr_hvs_backward_resized", "fr_hvs_resized_backward_floats",
           "fr_hvs_fov_workspace_floats", "fr_hvs_fov_forward", "fr_hvs_fov_backward", "fr_hvs_fov_backward_plan",
           "fr_quality_blocks", "fr_quality_forward", "fr_quality_finish",
           "fr_scale_decay_blocks", "fr_scale_decay_forward", "fr_scale_decay_backward", "fr_opacity_cap",
           "fr_select_kth", "fr_mask_le", "fr_volume", "fr_v_importance",
           "fr_vq_workspace_bytes", "fr_vq_nearest", "fr_vq_gather", "fr_vq_update", "fr_vq_replace", "fr_pack_bits", "fr_unpack_bits",
           "fr_forward_begin_fov_keep", "fr_forward_fov_keep_call", "fr_geometry_bytes_fov_keep", "fr_image_bytes_fov_keep",
           "fr_image_fov_state_T", "fr_image_fov_state_n", "fr_backward_fov_appearance",
           "fr_forward_begin_fov_keep_full", "fr_forward_fov_keep_full_call", "fr_geometry_bytes_fov_keep_full", "fr_backward_fov",
           "fr_forward_begin_aux", "fr_forward_aux_call",
           "fr_lpips_packed_bytes", "fr_lpips_pack_weights", "fr_lpips_workspace_bytes", "fr_lpips_forward",
           "fr_lpips_backward_packed_bytes", "fr_lpips_pack_backward_weights", "fr_lpips_keep_workspace_bytes",
           "fr_lpips_keep_activation_offset", "fr_lpips_forward_keep", "fr_lpips_backward",
           "fr_hvs_metamer_workspace_floats", "fr_hvs_metamer", "fr_hvs_metamer_roundtrip",
           "fr_hvs_metamer_loss_workspace_doubles", "fr_hvs_metamer_loss_forward", "fr_hvs_metamer_loss_backward")
# added without an ABI bump: a library of the same ABI version built before them loads too (tools/ab_run.sh swaps libraries under one
# Python); has_forward_ext() says which, and the callers fall back (rasterizer.py: visibility = radii > 0)
EXT_EXPORTS = ("fr_forward_begin_ext", "fr_forward_ext_call")
# ... and the foveation settings (fr_foveation): has_foveation(); without them only the reference's constants render
FOVEATION_EXPORTS = ("fr_forward_begin_fov", "fr_forward_fov_call", "fr_geometry_bytes_fov", "fr_geometry_level_colours_hi", "fr_pack_colour_fov")
# ... and the foveated renderer's appearance backward pass: has_fov_backward(); without it appearance_only on that renderer raises
FOV_BACKWARD_EXPORTS = ("fr_forward_begin_fov_keep", "fr_forward_fov_keep_call", "fr_geometry_bytes_fov_keep", "fr_image_bytes_fov_keep",
                        "fr_image_fov_state_T", "fr_image_fov_state_n", "fr_backward_fov_appearance")
# ... and its full backward pass (geometry, rest SH): has_fov_full_backward(); without it differentiable=True on that renderer raises
FOV_FULL_BACKWARD_EXPORTS = ("fr_forward_begin_fov_keep_full", "fr_forward_fov_keep_full_call", "fr_geometry_bytes_fov_keep_full", "fr_backward_fov")
# ... and the inference renderers' depth / coverage outputs (fr_forward_aux): has_forward_aux(); without them want_depth=True raises
FORWARD_AUX_EXPORTS = ("fr_forward_begin_aux", "fr_forward_aux_call")
OPTIONAL_EXPORTS = EXT_EXPORTS + FOVEATION_EXPORTS + FOV_BACKWARD_EXPORTS + FOV_FULL_BACKWARD_EXPORTS + FORWARD_AUX_EXPORTS
FOV_STATE_FULL = 0x100  # FR_FOV_STATE_FULL: set in fr_fov_state.variant by the _full forward

_lib = None


class NativeLibraryError(RuntimeError):
    pass


def load():
    """Load (once) and return the HIP library; raise NativeLibraryError if that is impossible."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"fovraster: {LIB_PATH} not found -- the HIP extension is not built and there is no CPU fallback. "
            "Run `make -C fov-3dgs_amd/csrc` (or __graft_entry__.build()).")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # missing ROCm runtime, wrong arch, ...
        raise NativeLibraryError(f"fovraster: cannot load {LIB_PATH}: {e}") from e
    for name in EXPORTS:
        if not hasattr(lib, name) and name not in OPTIONAL_EXPORTS:
            raise NativeLibraryError(f"fovraster: {LIB_PATH} does not export {name}")
    lib.fr_abi_version.restype = C.c_int
    lib.fr_last_error.restype = C.c_char_p
    lib.fr_event_create.restype = C.c_void_p
    lib.fr_event_destroy.argtypes = [C.c_void_p]
    lib.fr_event_destroy.restype = None
    lib.fr_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    lib.fr_event_elapsed_ms.restype = C.c_int
    lib.fr_forward.argtypes = [C.POINTER(ForwardArgs)]
    lib.fr_forward.restype = C.c_int
    lib.fr_backward.argtypes = [C.POINTER(BackwardArgs)]
    lib.fr_backward.restype = C.c_int
    lib.fr_backward_appearance.argtypes = [C.POINTER(BackwardArgs)]
    lib.fr_backward_appearance.restype = C.c_int
    lib.fr_mark_visible.argtypes = [C.c_int32, _FP, _FP, _FP, _FP, C.c_void_p]
    lib.fr_mark_visible.restype = C.c_int
    lib.fr_pack_geom.argtypes = [C.c_int32, _FP, _FP, _FP, _FP, C.c_int32, _FP, _FP, C.c_void_p]
    lib.fr_pack_geom.restype = C.c_int
    lib.fr_pack_colour.argtypes = [C.c_int32, _FP, _FP, _FP, _FP, C.c_void_p]
    lib.fr_pack_colour.restype = C.c_int
    lib.fr_pack_cull.argtypes = [C.c_int32, _FP, _FP, _FP, _FP, C.c_void_p]
    lib.fr_pack_cull.restype = C.c_int
    lib.fr_activate_forward.argtypes = [C.c_int32] + [_FP] * 6 + [C.c_void_p]
    lib.fr_activate_forward.restype = C.c_int
    lib.fr_activate_backward.argtypes = [C.c_int32] + [_FP] * 9 + [C.c_void_p]
    lib.fr_activate_backward.restype = C.c_int
    lib.fr_l1_ssim_blocks.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.fr_l1_ssim_blocks.restype = C.c_int64
    lib.fr_l1_ssim_forward.argtypes = [C.c_int32, C.c_int32, C.c_int32, _FP, _FP, _FP, _FP, C.c_void_p]
    lib.fr_l1_ssim_forward.restype = C.c_int
    lib.fr_l1_ssim_finish.argtypes = [C.c_int32, C.c_int32, C.c_int32, _FP, C.c_float, _FP, C.c_void_p]
    lib.fr_l1_ssim_finish.restype = C.c_int
    lib.fr_l1_ssim_backward.argtypes = [C.c_int32, C.c_int32, C.c_int32, _FP, _FP, _FP, C.c_float, C.c_float, _FP, _FP, C.c_void_p]
    lib.fr_l1_ssim_backward.restype = C.c_int
    lib.fr_hvs_workspace_floats.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32]
    lib.fr_hvs_workspace_floats.restype = C.c_int64
    lib.fr_hvs_forward.argtypes = [C.c_int32, C.c_int32, C.c_double] + [C.c_int32] * 4 + [_FP] * 7 + [C.c_void_p]
    lib.fr_hvs_forward.restype = C.c_int
    lib.fr_hvs_backward.argtypes = [C.c_int32, C.c_int32, C.c_double] + [C.c_int32] * 4 + [_FP] * 6 + [C.c_void_p]
    lib.fr_hvs_backward.restype = C.c_int
    lib.fr_hvs_forward_resized.argtypes = [C.c_int32] * 4 + [C.c_double] + [C.c_int32] * 4 + [_FP] * 7 + [C.c_void_p]
    lib.fr_hvs_forward_resized.restype = C.c_int
    lib.fr_hvs_backward_resized.argtypes = [C.c_int32] * 4 + [C.c_double] + [C.c_int32] * 4 + [_FP] * 6 + [C.c_void_p]
    lib.fr_hvs_backward_resized.restype = C.c_int
    lib.fr_hvs_resized_backward_floats.argtypes = [C.c_int32] * 4 + [C.c_double, C.c_int32, C.c_int32]
    lib.fr_hvs_resized_backward_floats.restype = C.c_int64
    lib.fr_hvs_fov_workspace_floats.argtypes = [C.c_int32] * 7
    lib.fr_hvs_fov_workspace_floats.restype = C.c_int64
    _fov = [C.c_int32] * 4 + [C.c_double] * 3 + [C.c_int32, C.c_double, C.c_double] + [C.c_int32] * 4
    lib.fr_hvs_fov_forward.argtypes = _fov + [_FP] * 6 + [C.c_int32, _FP, _FP, C.c_void_p]
    lib.fr_hvs_fov_forward.restype = C.c_int
    lib.fr_hvs_fov_backward.argtypes = _fov + [_FP] * 7 + [C.c_void_p]
    lib.fr_hvs_fov_backward.restype = C.c_int
    lib.fr_hvs_fov_backward_plan.argtypes = [C.c_int32] * 6 + [C.POINTER(C.c_int64)]
    lib.fr_hvs_fov_backward_plan.restype = C.c_int
    lib.fr_hvs_metamer_workspace_floats.argtypes = [C.c_int32] * 5
    lib.fr_hvs_metamer_workspace_floats.restype = C.c_int64
    lib.fr_hvs_metamer.argtypes = [C.c_int32] * 2 + [C.c_double] * 3 + [C.c_int32, C.c_double, C.c_double] + [C.c_int32] * 3 + [_FP] * 5 + [C.c_void_p]
    lib.fr_hvs_metamer.restype = C.c_int
    lib.fr_hvs_metamer_roundtrip.argtypes = [C.c_int32] * 5 + [_FP] * 4 + [C.c_void_p]
    lib.fr_hvs_metamer_roundtrip.restype = C.c_int
    lib.fr_hvs_metamer_loss_workspace_doubles.argtypes = [C.c_int64]
    lib.fr_hvs_metamer_loss_workspace_doubles.restype = C.c_int64
    lib.fr_hvs_metamer_loss_forward.argtypes = [C.c_int64, C.c_int32] + [_FP] * 4 + [C.c_void_p]
    lib.fr_hvs_metamer_loss_forward.restype = C.c_int
    lib.fr_hvs_metamer_loss_backward.argtypes = [C.c_int64, C.c_int32] + [_FP] * 4 + [C.c_void_p]
    lib.fr_hvs_metamer_loss_backward.restype = C.c_int
    for n in ("fr_geometry_bytes",):
        getattr(lib, n).argtypes = [C.c_int32, C.c_int32]
        getattr(lib, n).restype = C.c_size_t
    lib.fr_image_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.fr_image_bytes.restype = C.c_size_t
    lib.fr_binning_bytes.argtypes = [C.c_int32, C.c_int64]
    lib.fr_binning_bytes.restype = C.c_size_t
    for n in ("fr_image_ranges", "fr_image_final_T", "fr_image_n_contrib"):
        getattr(lib, n).argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        getattr(lib, n).restype = C.c_void_p
    lib.fr_binning_point_list.argtypes = [C.c_int32, C.c_int64, C.c_void_p]
    lib.fr_binning_point_list.restype = C.c_void_p
    lib.fr_geometry_records.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
    lib.fr_geometry_records.restype = C.c_void_p
    for n in ("fr_geometry_vis_list", "fr_geometry_vis_count", "fr_geometry_walk_records"):
        getattr(lib, n).argtypes = [C.c_int32, C.c_int32, C.c_void_p]
        getattr(lib, n).restype = C.c_void_p
    for n in ("fr_geometry_level_colours", "fr_geometry_level_ranges"):
        getattr(lib, n).argtypes = [C.c_int32, C.c_void_p]
        getattr(lib, n).restype = C.c_void_p
    lib.fr_image_tile_levels.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
    lib.fr_image_tile_levels.restype = C.c_void_p
    lib.fr_forward_begin.argtypes = [C.POINTER(ForwardArgs), C.POINTER(C.c_void_p)]
    lib.fr_forward_begin.restype = C.c_int
    if has_forward_ext(lib):
        lib.fr_forward_begin_ext.argtypes = [C.POINTER(ForwardArgs), C.POINTER(ForwardExt), C.POINTER(C.c_void_p)]
        lib.fr_forward_begin_ext.restype = C.c_int
        lib.fr_forward_ext_call.argtypes = [C.POINTER(ForwardArgs), C.POINTER(ForwardExt)]
        lib.fr_forward_ext_call.restype = C.c_int
    if has_foveation(lib):
        lib.fr_forward_begin_fov.argtypes = [C.POINTER(ForwardArgs), C.POINTER(ForwardExt), C.POINTER(Foveation), C.POINTER(C.c_void_p)]
        lib.fr_forward_begin_fov.restype = C.c_int
        lib.fr_forward_fov_call.argtypes = [C.POINTER(ForwardArgs), C.POINTER(ForwardExt), C.POINTER(Foveation)]
        lib.fr_forward_fov_call.restype = C.c_int
        lib.fr_geometry_bytes_fov.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        lib.fr_geometry_bytes_fov.restype = C.c_size_t
        lib.fr_geometry_level_colours_hi.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
        lib.fr_geometry_level_colours_hi.restype = C.c_void_p
        lib.fr_pack_colour_fov.argtypes = [C.c_int32, _FP, _FP, C.c_int32, _FP, C.c_void_p]
        lib.fr_pack_colour_fov.restype = C.c_int
    if has_forward_aux(lib):
        lib.fr_forward_begin_aux.argtypes = [C.POINTER(ForwardArgs), C.POINTER(ForwardExt), C.POINTER(Foveation), C.POINTER(ForwardAux),
                                             C.POINTER(C.c_void_p)]
        lib.fr_forward_begin_aux.restype = C.c_int
        lib.fr_forward_aux_call.argtypes = [C.POINTER(ForwardArgs), C.POINTER(ForwardExt), C.POINTER(Foveation), C.POINTER(ForwardAux)]
        lib.fr_forward_aux_call.restype = C.c_int
    if has_fov_backward(lib):
        lib.fr_forward_begin_fov_keep.argtypes = [C.POINTER(ForwardArgs), C.POINTER(ForwardExt), C.POINTER(Foveation), C.POINTER(FovState),
                                                  C.POINTER(C.c_void_p)]
        lib.fr_forward_begin_fov_keep.restype = C.c_int
        lib.fr_forward_fov_keep_call.argtypes = [C.POINTER(ForwardArgs), C.POINTER(ForwardExt), C.POINTER(Foveation), C.POINTER(FovState)]
        lib.fr_forward_fov_keep_call.restype = C.c_int
        lib.fr_geometry_bytes_fov_keep.argtypes = [C.c_int32, C.c_int32]
        lib.fr_geometry_bytes_fov_keep.restype = C.c_size_t
        lib.fr_image_bytes_fov_keep.argtypes = [C.c_int32, C.c_int32]
        lib.fr_image_bytes_fov_keep.restype = C.c_size_t
        for n in ("fr_image_fov_state_T", "fr_image_fov_state_n"):
            getattr(lib, n).argtypes = [C.c_int32, C.c_int32, C.c_void_p]
            getattr(lib, n).restype = C.c_void_p
        lib.fr_backward_fov_appearance.argtypes = [C.POINTER(BackwardFovArgs)]
        lib.fr_backward_fov_appearance.restype = C.c_int
    if has_fov_full_backward(lib):
        lib.fr_forward_begin_fov_keep_full.argtypes = lib.fr_forward_begin_fov_keep.argtypes
        lib.fr_forward_begin_fov_keep_full.restype = C.c_int
        lib.fr_forward_fov_keep_full_call.argtypes = lib.fr_forward_fov_keep_call.argtypes
        lib.fr_forward_fov_keep_full_call.restype = C.c_int
        lib.fr_geometry_bytes_fov_keep_full.argtypes = [C.c_int32, C.c_int32]
        lib.fr_geometry_bytes_fov_keep_full.restype = C.c_size_t
        lib.fr_backward_fov.argtypes = [C.POINTER(BackwardFovFullArgs)]
        lib.fr_backward_fov.restype = C.c_int
    lib.fr_forward_finish.argtypes = [C.c_void_p]
    lib.fr_forward_finish.restype = C.c_int
    lib.fr_backward_prefill.argtypes = [C.POINTER(BackwardArgs), C.c_void_p]
    lib.fr_backward_prefill.restype = C.c_int
    lib.fr_forward_abandon.argtypes = [C.c_void_p]
    lib.fr_forward_abandon.restype = C.c_int
    lib.fr_knn_workspace_bytes.argtypes = [C.c_int32]
    lib.fr_knn_workspace_bytes.restype = C.c_size_t
    lib.fr_knn_mean_dist2.argtypes = [C.c_int32, _FP, _FP, C.c_void_p, C.c_void_p]
    lib.fr_knn_mean_dist2.restype = C.c_int
    lib.fr_adam_step.argtypes = [C.POINTER(AdamArgs), C.c_void_p]
    lib.fr_adam_step.restype = C.c_int
    lib.fr_prune_workspace_bytes.argtypes = [C.c_int32]
    lib.fr_prune_workspace_bytes.restype = C.c_size_t
    lib.fr_prune_metric_max.argtypes = [C.c_int32, C.c_int32, _FP, _FP, _FP, C.c_void_p]
    lib.fr_prune_metric_max.restype = C.c_int
    lib.fr_prune_select_lowest.argtypes = [C.c_int32, _FP, C.c_int64, _FP, C.c_void_p, C.c_void_p]
    lib.fr_prune_select_lowest.restype = C.c_int
    lib.fr_compact_plan.argtypes = [C.c_int32, _FP, C.c_int32, _FP, C.c_void_p, C.c_void_p]
    lib.fr_compact_plan.restype = C.c_int
    lib.fr_compact_rows.argtypes = [C.POINTER(CompactArgs), C.c_void_p]
    lib.fr_compact_rows.restype = C.c_int
    lib.fr_densify_workspace_bytes.argtypes = [C.c_int32]
    lib.fr_densify_workspace_bytes.restype = C.c_size_t
    lib.fr_densify_stats.argtypes = [C.c_int32, _FP, _FP, _FP, _FP, C.c_void_p]
    lib.fr_densify_stats.restype = C.c_int
    lib.fr_densify_plan.argtypes = [C.POINTER(DensifyPlanArgs), C.c_void_p]
    lib.fr_densify_plan.restype = C.c_int
    lib.fr_densify_rows.argtypes = [C.POINTER(DensifyRowsArgs), C.c_void_p]
    lib.fr_densify_rows.restype = C.c_int
    lib.fr_quality_blocks.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.fr_quality_blocks.restype = C.c_int64
    lib.fr_quality_forward.argtypes = [C.c_int32] * 4 + [_FP, _FP, _FP, C.c_void_p]
    lib.fr_quality_forward.restype = C.c_int
    lib.fr_quality_finish.argtypes = [C.c_int32] * 4 + [_FP, _FP, C.c_int32, C.c_int32, _FP, C.c_void_p]
    lib.fr_quality_finish.restype = C.c_int
    lib.fr_scale_decay_blocks.argtypes = [C.c_int32]
    lib.fr_scale_decay_blocks.restype = C.c_int64
    lib.fr_scale_decay_forward.argtypes = [C.c_int32, _FP, _FP, C.c_int32, C.c_int32, _FP, _FP, C.c_void_p]
    lib.fr_scale_decay_forward.restype = C.c_int
    lib.fr_scale_decay_backward.argtypes = [C.c_int32, _FP, _FP, C.c_int32, C.c_int32, _FP, _FP, C.c_void_p]
    lib.fr_scale_decay_backward.restype = C.c_int
    lib.fr_opacity_cap.argtypes = [C.c_int32, _FP, C.c_float, C.c_float, _FP, _FP, _FP, C.c_void_p]
    lib.fr_opacity_cap.restype = C.c_int
    lib.fr_select_kth.argtypes = [C.c_int32, _FP, C.c_int32, C.c_int64, _FP, C.c_void_p, C.c_void_p]
    lib.fr_select_kth.restype = C.c_int
    lib.fr_mask_le.argtypes = [C.c_int32, _FP, C.c_int32, _FP, _FP, C.c_void_p]
    lib.fr_mask_le.restype = C.c_int
    lib.fr_volume.argtypes = [C.c_int32, _FP, C.c_int32, _FP, C.c_void_p]
    lib.fr_volume.restype = C.c_int
    lib.fr_v_importance.argtypes = [C.c_int32, _FP, _FP, C.c_float, _FP, _FP, C.c_void_p]
    lib.fr_v_importance.restype = C.c_int
    lib.fr_vq_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.fr_vq_workspace_bytes.restype = C.c_size_t
    _rows = [C.c_int64, C.c_int32, C.c_int32, _FP, C.c_int64, _FP, C.c_int32]  # n, K, D, feats, N, rows, rows64
    lib.fr_vq_nearest.argtypes = _rows + [_FP, _FP, _FP, C.c_void_p]
    lib.fr_vq_nearest.restype = C.c_int
    lib.fr_vq_gather.argtypes = _rows + [_FP, _FP, C.c_int32, _FP, _FP, _FP, C.c_float, _FP, C.c_void_p]
    lib.fr_vq_gather.restype = C.c_int
    lib.fr_vq_update.argtypes = _rows + [_FP, _FP, C.c_float, C.c_float, _FP, _FP, _FP, C.c_void_p]
    lib.fr_vq_update.restype = C.c_int
    lib.fr_vq_replace.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, _FP, C.c_int64, _FP, C.c_int32, _FP, _FP, _FP, _FP, C.c_void_p]
    lib.fr_vq_replace.restype = C.c_int
    lib.fr_pack_bits.argtypes = [C.c_int64, C.c_int32, _FP, _FP, C.c_void_p]
    lib.fr_pack_bits.restype = C.c_int
    lib.fr_unpack_bits.argtypes = [C.c_int64, C.c_int32, _FP, _FP, C.c_void_p]
    lib.fr_unpack_bits.restype = C.c_int
    lib.fr_lpips_packed_bytes.argtypes = []
    lib.fr_lpips_packed_bytes.restype = C.c_size_t
    lib.fr_lpips_pack_weights.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]
    lib.fr_lpips_pack_weights.restype = C.c_int
    lib.fr_lpips_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.fr_lpips_workspace_bytes.restype = C.c_int64
    lib.fr_lpips_forward.argtypes = [C.POINTER(LpipsArgs)]
    lib.fr_lpips_forward.restype = C.c_int
    lib.fr_lpips_backward_packed_bytes.argtypes = []
    lib.fr_lpips_backward_packed_bytes.restype = C.c_size_t
    lib.fr_lpips_pack_backward_weights.argtypes = [C.POINTER(C.c_void_p), C.c_void_p]
    lib.fr_lpips_pack_backward_weights.restype = C.c_int
    lib.fr_lpips_keep_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.fr_lpips_keep_workspace_bytes.restype = C.c_int64
    lib.fr_lpips_keep_activation_offset.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.fr_lpips_keep_activation_offset.restype = C.c_int64
    lib.fr_lpips_forward_keep.argtypes = [C.POINTER(LpipsKeepArgs)]
    lib.fr_lpips_forward_keep.restype = C.c_int
    lib.fr_lpips_backward.argtypes = [C.POINTER(LpipsBackwardArgs)]
    lib.fr_lpips_backward.restype = C.c_int
    if lib.fr_abi_version() != ABI_VERSION:
        raise NativeLibraryError(f"fovraster: ABI version mismatch ({lib.fr_abi_version()} != {ABI_VERSION})")
    _lib = lib
    return lib


def has_forward_ext(lib=None):
    """the loaded library writes fr_forward_ext.visibility (else: compute it from radii)"""
    lib = load() if lib is None else lib
    return all(hasattr(lib, n) for n in EXT_EXPORTS)


def has_foveation(lib=None):
    """the loaded library takes fr_foveation settings (else: only the reference's constants, and anything else is refused)"""
    lib = load() if lib is None else lib
    return all(hasattr(lib, n) for n in FOVEATION_EXPORTS)


def has_forward_aux(lib=None):
    """the loaded library writes the inference renderers' depth / coverage planes (fr_forward_aux)"""
    lib = load() if lib is None else lib
    return all(hasattr(lib, n) for n in FORWARD_AUX_EXPORTS)


def has_fov_backward(lib=None):
    """the loaded library has the foveated renderer's appearance backward pass (fr_backward_fov_appearance)"""
    lib = load() if lib is None else lib
    return all(hasattr(lib, n) for n in FOV_BACKWARD_EXPORTS)


def has_fov_full_backward(lib=None):
    """the loaded library has the foveated renderer's full backward pass (fr_backward_fov)"""
    lib = load() if lib is None else lib
    return has_fov_backward(lib) and all(hasattr(lib, n) for n in FOV_FULL_BACKWARD_EXPORTS)


def last_error():
    return load().fr_last_error().decode("utf-8", "replace")
