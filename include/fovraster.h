/*
 * fovraster.h -- C ABI of libfovraster_hip.so, the MI355X (gfx950) rasterizer library.
 *
 * This is the drop-in boundary for the rasterizer hot path of horizon-research/Fov-3DGS.
 * Each entry point replaces one function of the reference's native layer (paths relative to
 * /root/reference/fov3dgs/submodules/):
 *
 *   fr_forward        <-  CudaRasterizer::Rasterizer::forward
 *                           diff-gaussian-rasterization/cuda_rasterizer/rasterizer.h:36-61      ("original")
 *                           diff-gaussian-rasterization_pcheck_obb_sum/cuda_rasterizer/rasterizer.h (RS, + counts)
 *                           diff-gaussian-rasterization_pcheck_obb/cuda_rasterizer/rasterizer.h     (RP)
 *                           diff-gaussian-rasterization_fov_pcheck_obb/cuda_rasterizer/rasterizer.h:31-64 (RF)
 *                         as called by RasterizeGaussiansCUDA (…/rasterize_points.cu:35-115; RS :35-135; RF :35-152)
 *   fr_backward       <-  CudaRasterizer::Rasterizer::backward (…/cuda_rasterizer/rasterizer.h:63-85)
 *                         as called by RasterizeGaussiansBackwardCUDA (…/rasterize_points.cu:117-196)
 *   fr_mark_visible   <-  CudaRasterizer::Rasterizer::markVisible (…/rasterizer.h:24-29; rasterize_points.cu:198-217)
 *   fr_resize_fn      <-  the std::function<char*(size_t)> buffer callbacks (…/rasterize_points.cu:27-33)
 *   fr_adam_step      <-  torch.optim.Adam(l, lr=0.0, eps=1e-15).step() (fov3dgs/scene/gaussian_model.py:289; not a native
 *                         function of the reference: the last step of its training iteration, eff_finetune.py:147)
 *
 * Conventions: every pointer in the argument structs is a DEVICE pointer to fp32/int32 data laid
 * out exactly as the reference's tensors (row-major, contiguous) unless stated otherwise; NULL
 * stands for the reference's "empty tensor". The library never allocates or frees device memory:
 * the three workspaces are obtained through the caller's resize callbacks, exactly like the
 * reference's geometry/binning/image buffers, and must be kept alive by the caller for
 * fr_backward. All work is enqueued on `stream` (a hipStream_t) and on helper streams of the library that fork from / join
 * into it. fr_forward returns num_rendered like the reference, so it waits ONCE for that count (a 32-byte block the tile
 * scan writes into pinned host memory, polled) -- but not for the frame. fr_forward_begin / fr_forward_finish are the two
 * halves of that call around the wait: a host that keeps two frames in flight (two streams, two workspace sets) runs the
 * head of frame n + 1 beside the sort and the blend of frame n. fr_backward never synchronises.
 * All functions return 0 on success or a negative FR_ERR_* code; fr_last_error() gives the message
 * (thread-local).
 */
#ifndef FOVRASTER_H
#define FOVRASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FR_ABI_VERSION 12

/* rasterizer variants (the reference ships them as separate extensions; `cuda_type` strings of
 * fov3dgs/gaussian_wrapper.py:11-23) */
enum {
	FR_VARIANT_ORIGINAL = 0,       /* diff-gaussian-rasterization                    */
	FR_VARIANT_PCHECK_OBB_SUM = 1, /* …_pcheck_obb_sum (training; counts/contributions) */
	FR_VARIANT_PCHECK_OBB = 2,     /* …_pcheck_obb (inference)                        */
	FR_VARIANT_FOV_PCHECK_OBB = 3, /* …_fov_pcheck_obb (foveated inference)           */
	/* pruning-metric variants of the training rasterizer (prune.py / metric_mask_learn.py); forward
	 * statistics differ from …_sum, backward is identical */
	FR_VARIANT_PCHECK_OBB_MAX = 4, /* …_pcheck_obb_max: count per in-support pixel, contributions = max alpha*T */
	FR_VARIANT_PCHECK_OBB_LWMC = 5, /* …_pcheck_obb_loss_weighted_max_count: per-pixel loss credited to its
	                                 * max-contribution Gaussian */
	/* the paper's shared-model foveated baseline ("SMFR", fps/naiveFR): …_naive_pcheck_obb. Tile levels, the level
	 * filter and the instance lists of FOV_PCHECK_OBB, but ONE colour / opacity per Gaussian (shs [P,16,3],
	 * opacities [P,1], highest_levels [P,1]; no shs_dcs), blended per naive forward.cu:258-480 (two-level tiles)
	 * and :482-580 (single-level tiles). Inference only, no packed layout. */
	FR_VARIANT_NAIVE_FOV_PCHECK_OBB = 6,
	/* the paper's multi-model foveated baseline ("MMFR", fps/MMFR-Q): …_mmfr_pcheck_obb. ONE call renders the share of
	 * eccentricity level `cur_level` from that level's own model (plain inputs: shs [P,16,3], opacities [P,1]); the caller
	 * adds the calls of all levels up (gaussian_renderer_fov_mmfr/__init__.py:76-162). Tiles whose tile_min (clamped at 0)
	 * lies outside (cur_level - 0.5, cur_level + 1) are skipped (left zero); two-level tiles weight every pixel by the
	 * smoothstep of its estimated level (mmfr forward.cu:255-420). highest_levels must be given and hold ZEROS [P,1]
	 * (the skip test reuses the level filter). Inference only, no packed layout. */
	FR_VARIANT_MMFR_PCHECK_OBB = 7
};

enum {
	FR_OK = 0,
	FR_ERR_INVALID = -1,   /* bad argument combination (message says which) */
	FR_ERR_HIP = -2,       /* a HIP call or kernel failed */
	FR_ERR_ALLOC = -3,     /* a resize callback returned NULL */
	FR_ERR_PREFILTERED = -4 /* `prefiltered` was set and a Gaussian lies behind the near plane (the reference traps:
	                         * cuda_rasterizer/auxiliary.h:156-160); nothing was rendered */
};

/* Workspace callback: make the buffer at least `bytes` long and return its device address.
 * Same contract as the reference's resizeFunctional lambdas. */
typedef char *(*fr_resize_fn)(void *user, size_t bytes);

typedef struct fr_forward_args {
	int32_t variant;
	int32_t P;            /* number of Gaussians */
	int32_t D;            /* active SH degree (0..3) */
	int32_t M;            /* SH coefficients per Gaussian in `shs` (16; RF: 15 = rest only); 0 if shs == NULL */
	int32_t W, H;         /* image size */
	int32_t prefiltered;  /* the caller promises that no Gaussian is behind the near plane; a violation is FR_ERR_PREFILTERED */
	int32_t debug;        /* != 0: synchronise + check after every launch */
	float tanfovx, tanfovy;
	float scale_modifier;
	/* foveation (RF only) */
	float gaze_x, gaze_y; /* normalised gaze in [0,1]^2 (reference passes gazeArray and .item()s it) */
	float alpha;          /* pooling-size slope (0.05) */
	void *stream;         /* hipStream_t */
	/* inputs */
	const float *background;     /* [3] */
	const float *means3D;        /* [P,3] */
	const float *shs;            /* [P,M,3] or NULL */
	const float *colors_precomp; /* [P,3] or NULL */
	const float *opacities;      /* [P,1]; RF: [P,4] per level ([P,L] with fr_foveation.levels = L) */
	const float *scales;         /* [P,3] or NULL */
	const float *rotations;      /* [P,4] or NULL */
	const float *cov3D_precomp;  /* [P,6] or NULL */
	const float *viewmatrix;     /* [4,4] as the reference passes it (world-to-camera, transposed) */
	const float *projmatrix;     /* [4,4] */
	const float *campos;         /* [3] */
	const float *shs_dcs;        /* RF: [P,4,3] per-level DC coefficient ([P,L,3] with fr_foveation.levels = L) */
	const float *highest_levels; /* RF: [P,1] float */
	/* outputs (caller-allocated; out_color and radii are written in full, they need no initialisation: every pixel by the
	 * blend -- RF: the two-level tiles, whose two level states are ADDED, are cleared by the cull pass first; no fill command
	 * touches the image --, every radius by the cull pass or the projection) */
	float *out_color;            /* [3,H,W] */
	int32_t *radii;              /* [P] */
	int32_t *gaussians_count;    /* RS: [P], else NULL (zeroed by the call, then accumulated) */
	float *contributions;        /* RS: [P], else NULL (zeroed by the call, then accumulated) */
	/* FR_VARIANT_ORIGINAL with BOTH of them set is the counting render of LightGaussian's global-significance pruning
	 * (compress-diff-gaussian-rasterization, count_gaussians / renderCUDA_count, cuda_rasterizer/forward.cu:378-501); exactly
	 * one of them set is FR_ERR_INVALID. Image, radii, final_T and n_contrib are those of the plain call bit for bit, and both
	 * arrays are written in full:
	 *   gaussians_count[i] = the (pixel, Gaussian i) pairs the blend accumulated (past the power > 0, alpha < 1/255 and
	 *                        T (1 - alpha) < 1e-4 tests), exact;
	 *   contributions[i]   = important_score: (float)((double)gaussians_count[i] * (double)opacity[i]), the opacity as the blend
	 *                        used it (through the sigmoid with raw_activations, from packed_geom with the packed layout).
	 * A deviation from the reference on purpose: its two statements (forward.cu:473-474, `gaussian_count[id]++` and
	 * `important_score[id] += con_o.w`) are NON-atomic read-modify-writes from all 256 threads of every tile, so its output
	 * is not a function of its input (lanes that hit the same entry collapse into one increment). Here: what the statements
	 * give when the pixels run one at a time, the same bits on every run (integer atomics only). */
	/* workspaces */
	fr_resize_fn geometry_resize;
	fr_resize_fn binning_resize;
	fr_resize_fn image_resize;
	void *resize_user[3];        /* passed to the three callbacks in that order */
	/* result */
	int32_t num_rendered;        /* out: number of (Gaussian,tile) instances after culling */
	int32_t max_tile_instances;  /* out: longest per-tile list */
	/* optional profiling: HOST pointer to FR_NUM_STAGES + 1 event handles made by fr_event_create() (any of
	 * them may be NULL), or NULL. Event i is recorded on `stream` just before stage i (FR_STAGE_* order), event
	 * FR_NUM_STAGES after the last one; nothing is synchronised. Read the stage durations later with
	 * fr_event_elapsed_ms(ev[i], ev[i+1]). */
	void **stage_events;
	const float *loss_map;       /* LWMC: [>= H*W] per-pixel weights (the reference passes a [3,H,W] map and reads
	                              * its first plane, …_loss_weighted_max_count/cuda_rasterizer/forward.cu:435) */
	/* optional (not RF): the SH coefficients as the two tensors a 3DGS model stores them in, so that the caller
	 * need not concatenate them every step (GaussianModel.get_features, scene/gaussian_model.py:83-86): when
	 * set, `shs` is the DC part [P,1,3] and `shs_rest` the others [P,M-1,3]; M stays their total (16). */
	const float *shs_rest;
	/* optional: the per-Gaussian inputs of a STATIC model in the layout the binning kernel reads fastest (made once,
	 * e.g. when the model is loaded; the reference has no counterpart -- its inputs are the separate tensors above,
	 * which stay mandatory and must hold the same values). The binning kernel reads a candidate's parameters from
	 * five different tensors, i.e. five mostly-unused cache lines per Gaussian, and 180-byte SH rows that straddle
	 * lines; with these it reads one 64-byte row and one aligned 256-byte row instead. Results are bit-identical.
	 *   packed_geom   [P][16]: x y z | sx sy sz | q0 q1 q2 q3 | highest_level (RF, else 0) | 0 | opacity[4]
	 *                          (RF: the four levels; else opacity, 0, 0, 0)         needs scales + rotations
	 *   packed_colour [P][64]: SH coefficients 1..15 [45] | SH coefficient 0 [3] (not RF) | shs_dcs [4][3] (RF) | 0[4]
	 *                                                                             needs shs with M = 16 (RF: 15)
	 *   packed_cull   [P][4] : x y z | bound of the covariance's spectral norm at scale_modifier 1 (max scale^2, times
	 *                          the factor a non-unit quaternion adds): all the conservative cull pass reads
	 * All three or none. fr_pack_geom / fr_pack_colour / fr_pack_cull fill them on the device. */
	const float *packed_geom;
	const float *packed_colour;
	const float *packed_cull;
	float cur_level;             /* MMFR: the level (0..3) this call renders */
	/* optional (variants with one opacity per Gaussian and no levels: ORIGINAL, PCHECK_OBB and the training variants; not
	 * with cov3D_precomp or the packed layout): `scales`, `rotations` and `opacities` hold the model's RAW parameters
	 * (log scale, unnormalised quaternion, opacity logit) and the kernels apply GaussianModel's activations themselves
	 * (exp, x / max(|x|, 1e-12), sigmoid: scene/gaussian_model.py:200-240) -- the same device expressions as
	 * fr_activate_forward, so the image is bit-identical to activating first. Saves the two streaming passes over all P
	 * Gaussians around every training step. */
	int32_t raw_activations;
	int32_t num_candidates;      /* out: entries of the library's list of the Gaussians that survived its cull pass
	                              * (fr_geometry_vis_list): the rows of a row-sparse backward call */
	/* optional diagnostic output (NULL = off, no cost): uint32 [T], per tile the number of entries of its depth-sorted list the
	 * blend FETCHED before every pixel of the tile was finished -- the reference's loop runs in batches of 256 (forward.cu:333-347:
	 * `done` is voted on per batch), this build's in batches of 64, so the figure is the list position rounded up to 64 (capped at
	 * the list's length); two-level RF tiles: the larger of their two level states. Cleared by the call. Sum / num_rendered =
	 * the fraction of the frame's instances the blend consumes (bench.py: config.list_consumed_frac). */
	uint32_t *list_consumed;
	/* optional (PCHECK_OBB_SUM only): != 0 = the caller does not read gaussians_count / contributions (both may be NULL):
	 * eff_finetune.py:107-108 drops gs_count / contribs of every training step. The blend then keeps only what the backward pass
	 * needs (final_T, n_contrib); image, radii, lists and gradients are those of the variant. */
	int32_t no_stats;
	/* optional diagnostic output (NULL = off): uint32 [T], per tile the number of (band of eight rows, list entry) pairs the blend
	 * evaluated -- the entries of the fetched batches that can reach the band at all (the kernels' reach mask), two-level RF tiles
	 * counted per level state. Cleared by the call. The unit the blend kernels' VALU time is proportional to (bench.py /
	 * profiles: vector instructions per blended pair). */
	uint32_t *blend_pairs;
	/* != 0: every kernel and fill of the frame goes to `stream` itself -- no helper streams (by default the library forks the image /
	 * statistics fills and the sort of the short lists onto two helper streams of its own per launch stream, which pays off for ONE
	 * frame at a time). A host that keeps several frames in flight on several streams sets it: a process's streams share a handful of
	 * hardware queues (four by default), and a frame's helper stream that lands in another frame's queue serialises the two.
	 * A bit field: bit 0 (FR_FRAME_NO_HELPER_STREAMS) is the above -- any non-zero value turns the helper streams off --, bit 1
	 * (FR_FRAME_SHARES_GPU, only with bit 0: the value 3) says that the frame runs BESIDE other frames of the same host: its cull and
	 * binning kernels then keep fewer waves resident per CU, which leaves registers and LDS to the neighbouring frame's emission, sort and
	 * blend. Every output is bit-identical whatever the value; a frame alone on the GPU is fastest with bit 1 clear. The environment
	 * variable FOVRASTER_LONE_GEOMETRY=1 (read once) makes the library ignore bit 1. */
	int32_t no_helper_streams;
} fr_forward_args;

/* fr_forward_args.no_helper_streams */
enum { FR_FRAME_NO_HELPER_STREAMS = 1, FR_FRAME_SHARES_GPU = 2 };

enum { FR_STAGE_TILE_LEVELS = 0, FR_STAGE_PROJECT = 1, FR_STAGE_BIN = 2, FR_STAGE_TILE_SCAN = 3, FR_STAGE_EMIT = 4,
	FR_STAGE_TILE_SORT = 5, FR_STAGE_RENDER = 6, FR_NUM_STAGES = 7 };

typedef struct fr_backward_args {
	int32_t variant;             /* ORIGINAL, PCHECK_OBB_SUM, PCHECK_OBB_MAX or PCHECK_OBB_LWMC */
	int32_t P, D, M, R;          /* R = num_rendered of the forward call */
	int32_t W, H;
	int32_t debug;
	float tanfovx, tanfovy;
	float scale_modifier;
	void *stream;
	const float *background, *means3D, *shs, *colors_precomp, *opacities, *scales, *rotations,
		*cov3D_precomp, *viewmatrix, *projmatrix, *campos;
	const int32_t *radii;        /* [P] from forward: the forward call's output UNMODIFIED (the whole-line stores of the narrow gradient
	                              * tensors take `radii > 0` for "this row is written by the per-Gaussian pass": a clamped or edited copy leaves rows unwritten) */
	/* the three workspaces filled by fr_forward. The call accumulates into the geometry workspace's per-Gaussian gradient
	 * sums and clears them again before it ends: calling fr_backward twice over one forward state gives the same
	 * gradients twice (the reference: fresh torch::zeros per call), but two calls must not run concurrently on it. */
	char *geometry;
	const char *binning, *image;
	const float *dL_dpix;        /* [3,H,W] */
	/* outputs: caller-allocated, WRITTEN IN FULL by the call (rows of Gaussians the view does not touch become zero; the
	 * reference allocates them with torch::zeros, rasterize_points.cu:171-179, and only writes the visible rows): no
	 * initialisation needed */
	float *dL_dmean2D;           /* [P,3] */
	float *dL_dconic;            /* [P,2,2]; may be NULL: an intermediate of the reference (its sums are kept per visible-list entry here) */
	float *dL_dopacity;          /* [P,1] */
	float *dL_dcolor;            /* [P,3]; may be NULL unless colors_precomp is given (otherwise an intermediate) */
	float *dL_dmean3D;           /* [P,3] */
	float *dL_dcov3D;            /* [P,6]; may be NULL when cov3D_precomp is NULL (then it is an intermediate nobody reads) */
	float *dL_dsh;               /* [P,M,3] */
	float *dL_dscale;            /* [P,3] */
	float *dL_drot;              /* [P,4] */
	void **stage_events;         /* optional: HOST pointer to 5 event handles (any may be NULL): [0] [1] [2] on `stream` before the
	                              * tile pass (k_render_bwd), between it and the per-Gaussian pass (k_preprocess_bwd), and after that;
	                              * [3] [4] around the zero fill of the gradient tensors, on the helper stream it runs on */
	const float *shs_rest;       /* split SH input, see fr_forward_args.shs_rest ... */
	float *dL_dsh_rest;          /* ... then dL_dsh is [P,1,3] and dL_dsh_rest [P,M-1,3] */
	int32_t raw_activations;     /* as in the forward call: dL_dscale / dL_drot / dL_dopacity are then gradients w.r.t. the RAW
	                              * parameters (what fr_activate_backward would make of them) */
	/* optional (extension; the reference returns dense tensors, rasterize_points.cu:171-179): ROW-SPARSE gradients. The
	 * gradient tensors are then COMPACT -- [C, .] instead of [P, .], C = fr_forward_args.num_candidates of the forward call --
	 * and row i belongs to the Gaussian vis_list[i] (fr_geometry_vis_list: increasing indices; every Gaussian the view touches is
	 * in the list, a candidate that landed in no tile has a zero row). Every row is written, nothing is zero-filled: at 6 M
	 * Gaussians a training step's backward pass otherwise clears 1.5 GB to write 0.5 GB. */
	int32_t row_sparse;
	uint32_t *blend_pairs;       /* optional diagnostic, as fr_forward_args.blend_pairs: [T], pairs k_render_bwd evaluated; cleared by the call */
	/* != 0: the caller has zero-filled the dense gradient tensors itself (fr_backward_prefill, or any other way) and the fill is
	 * complete on `stream`: the call then only writes the rows of the Gaussians the view touches. Lets a host clear the 1.5 GB of a
	 * 6 M-Gaussian model's gradients beside the work BETWEEN its forward and backward calls (the image loss) instead of beside
	 * k_render_bwd, which pays 0.11 ms for the company. */
	int32_t outputs_zeroed;
	/* optional (extension; multi-GPU training): the per-Gaussian half of the call in `num_ranges` > 1 pieces over
	 * increasing, disjoint ranges of ROWS (Gaussian indices) that cover [0, P). As soon as the kernels that complete range k are
	 * enqueued on `stream` -- every gradient tensor's rows [row_lo, row_hi) are then final once the stream gets there, zeros included --
	 * the HOST function range_done(range_user, k, row_lo, row_hi) is called (from inside fr_backward, on the calling thread): a host
	 * records an event there and starts summing those rows over its ranks on a communication stream while the later ranges are still
	 * being computed. Range k starts at row (P k / num_ranges) rounded down to a multiple of 32 (the visible list is in index order,
	 * so a range of rows is a range of list entries): equal shares of the INDEX range, not of the visible Gaussians. At most 16
	 * ranges. The pass runs in ONE piece when num_ranges is 0 or 1 and when P < 64 * num_ranges; range_done, when given, is then
	 * still called, exactly once, as range_done(range_user, 0, 0, P) behind the single launch: a host that sums what it is told
	 * about never misses rows. Dense gradients only: with row_sparse (the rows are not Gaussian indices), with
	 * range_done == NULL and with P == 0 (fr_backward returns at once: there is no row to report) there is no call. */
	int32_t num_ranges;
	void (*range_done)(void *user, int32_t k, int32_t row_lo, int32_t row_hi);
	void *range_user;
} fr_backward_args;

int fr_abi_version(void);
const char *fr_last_error(void);

/* hipEvent wrappers so a host that only speaks the C ABI can time stages on the launch stream */
void *fr_event_create(void);
void fr_event_destroy(void *event);
int fr_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on `stop` */

int fr_forward(fr_forward_args *args);
/* The same call in two halves (fr_forward == begin, then finish):
 *   fr_forward_begin   validates, asks for the geometry and image workspaces, enqueues the head of the frame (small fills, tile levels,
 *                      cull pass, projection, tile counts, tile scan) and returns without waiting for anything; *frame is
 *                      the handle of the frame in flight (NULL on error). `args` must stay alive and unchanged until
 *                      fr_forward_finish(*frame) has returned, which must be called exactly once, by the same host thread.
 *   fr_forward_finish  waits for the instance count (the frame's one host synchronisation), asks for the binning workspace
 *                      (possibly twice: once sized like the largest frame of the kind so far, again if that was too small
 *                      -- the last answer is the one in use), enqueues emission, sort, colours and blend, fills
 *                      args->num_rendered / max_tile_instances and releases the handle (also when it fails).
 * Frames in flight at the same time need their own stream and their own three workspaces each. */
typedef struct fr_frame fr_frame;
int fr_forward_begin(fr_forward_args *args, fr_frame **frame);
int fr_forward_finish(fr_frame *frame);
/* Drop a frame between its halves WITHOUT running its tail (a host that gives up on a frame, e.g. a garbage-collected handle):
 * joins the frame's helper stream into its launch stream, releases the pinned totals block and the handle; no wait, no callback,
 * no launch. out_color is left undefined. */
int fr_forward_abandon(fr_frame *frame);
/* Optional outputs beside fr_forward_args (whose layout FR_ABI_VERSION pins). size = sizeof(fr_forward_ext) as the caller was
 * compiled; the struct is read during the call only.
 *   visibility  [P] bytes, or NULL: 1 where radii > 0, else 0 -- written in full by the kernels that write radii (no initialisation
 *               needed), so a host that wants the reference's `radii > 0` mask needs no pass of its own over radii.
 * fr_forward_begin_ext / fr_forward_ext_call are fr_forward_begin / fr_forward with these outputs; ext == NULL: the same calls. */
typedef struct fr_forward_ext {
	uint32_t size;
	uint8_t *visibility;
} fr_forward_ext;
int fr_forward_begin_ext(fr_forward_args *args, const fr_forward_ext *ext, fr_frame **frame);
int fr_forward_ext_call(fr_forward_args *args, const fr_forward_ext *ext);
/* Foveation settings of one FR_VARIANT_FOV_PCHECK_OBB call (extension): the layer count and the display geometry the reference
 * compiles in as `__device__ const`s (…_fov_pcheck_obb/cuda_rasterizer/auxiliary.h:26-32; its scripts' --layer_num /
 * --max_pooling_size). The defaults are those constants. size = sizeof(fr_foveation) as the caller was compiled; the struct is read
 * during the call only, and its values travel to the kernels as arguments (no state outlives the call).
 *   levels                 L, 2 .. 8 (fov_num): opacities is [P,L], shs_dcs [P,L,3], highest_levels holds values in [0, L-1]; a
 *                          tile's level is capped at float(double(float(L)) - 0.1), a tile blends two levels when
 *                          frac(tile_min) > start_blend and int(tile_min) < L-1, and a Gaussian's level range ends at
 *                          min(hi + 1, L-1) when one of its tiles blends.
 *   max_pooling_size       > 1 (12): the largest pooling size in pixels; the kernels use s = float(sqrt(double(max_pooling_size)))
 *                          (sqrt_max_ps) and the level step float((double(s) - 1.) / double(float(L-1))), formed once on the host.
 *   real_image_width       > 0 (2.0): display width; pixels per unit = W / real_image_width.
 *   real_viewing_distance  > 0 (1.0): the viewer's distance from the display in the same unit: the z component of every view
 *                          direction and of the pixel distance, and major = (tan(a_max) - tan(a_min)) * real_viewing_distance.
 *                          Width 2 seen from 1 is a 90 degree field of view.
 *   start_blend            in (0,1) (0.5) and
 *   blend_width            > 0 (0.5): the weight of the upper level of a two-level tile is smoothstep(x),
 *                          x = clamp(|est - (L1 + start_blend)| / blend_width, 0, 1).
 * fr_forward_begin_fov / fr_forward_fov_call are fr_forward_begin_ext / fr_forward_ext_call with these settings; fov == NULL: the
 * same calls. A bad struct is FR_ERR_INVALID before anything is enqueued (the message names the field): size too small, levels
 * outside 2..8, a non-finite or out-of-range value, or settings with another variant (the SMFR / MMFR baselines keep the
 * reference's constants). levels <= 4 runs the kernels of a call without settings (levels other than 4: the library first copies
 * the level columns into four-wide rows of its geometry workspace); 5 .. 8 runs a second instantiation of the binning kernel
 * with eight level rows per item. The geometry workspace depends on levels (fr_geometry_bytes_fov); the image and binning
 * workspaces and every introspection pointer of the existing entry points do not. */
typedef struct fr_foveation {
	uint32_t size;
	int32_t levels;
	float max_pooling_size;
	float real_image_width;
	float real_viewing_distance;
	float start_blend;
	float blend_width;
} fr_foveation;
int fr_forward_begin_fov(fr_forward_args *args, const fr_forward_ext *ext, const fr_foveation *fov, fr_frame **frame);
int fr_forward_fov_call(fr_forward_args *args, const fr_forward_ext *ext, const fr_foveation *fov);
/* Per-pixel depth and coverage of the two INFERENCE renderers, FR_VARIANT_FOV_PCHECK_OBB and FR_VARIANT_PCHECK_OBB (extension; the
 * reference has neither: what a compositor merges the frame with its other layers by, and reprojects it with). The quantities are the
 * blend's own: a (pixel, Gaussian j) pair takes part exactly when the colour blend accumulates it (the same support test, the same
 * alpha < 1/255 test, the same T (1 - alpha) < 1e-4 stop; the stopping entry is not accumulated). With w_j = alpha_j T_j and z_j the
 * Gaussian's view-space depth (the float whose bits are in the sort key):
 *   depth    [H*W]  sum_j w_j z_j
 *   coverage [H*W]  1 - T_end (the transmittance the pixel ended with)
 *   a two-level tile of the foveated renderer: s1 D1 + s2 D2 and s1 (1 - T1) + s2 (1 - T2) with the shares s1 = w1, s2 = 1 - w1 of
 *   the image (w1 = 1 - smoothstep); a state-1 pixel that starts finished adds nothing, the upper state skips what does not exist at
 *   its level. The two rounded halves meet by float atomicAdd on a cleared pixel (x + y == y + x: no dependence on the order).
 * The background takes no part; a pixel no Gaussian reaches holds depth = 0 and coverage = 0. Nothing is divided: the EXPECTED depth
 * is the caller's depth / max(coverage, eps). Both planes are caller-allocated and written in full by the call (no initialisation
 * needed): every pixel by the blend -- a second instantiation of the blend kernel, launched only by these entry points; the image and
 * radii are those of the call without the outputs bit for bit --, and the two-level tiles of a foveated frame are cleared first by a
 * small tile-wise kernel behind the tile levels (no fill command over the planes). size = sizeof(fr_forward_aux) as the caller was
 * compiled; the struct is read during the begin call only.
 * fr_forward_begin_aux / fr_forward_aux_call are fr_forward_begin_fov / fr_forward_fov_call with these outputs; aux == NULL (or both
 * pointers NULL): the same calls. packed_* inputs, fr_foveation with any legal level count, every value of no_helper_streams and
 * list_consumed / blend_pairs work beside them. FR_ERR_INVALID before anything is enqueued, the message names the cause: size too
 * small; exactly one of the two pointers set; a variant other than the two above. (The state-keeping forwards take no fr_forward_aux:
 * their entry points have no such argument, and the library's common begin path refuses the pair.) */
typedef struct fr_forward_aux {
	uint32_t size;
	float *depth;
	float *coverage;
} fr_forward_aux;
int fr_forward_begin_aux(fr_forward_args *args, const fr_forward_ext *ext, const fr_foveation *fov, const fr_forward_aux *aux, fr_frame **frame);
int fr_forward_aux_call(fr_forward_args *args, const fr_forward_ext *ext, const fr_foveation *fov, const fr_forward_aux *aux);
/* Fill fr_forward_args.packed_geom / packed_colour / packed_cull (device buffers of P*16 / P*64 / P*4 floats) from the tensors of the
 * same names; opacities is [P,levels] with levels = 1 or 4, highest_levels / shs_dcs may be NULL (not RF);
 * shs_rest NULL: shs is [P,16,3] (RF: [P,15,3] = coefficients 1..15 and shs_dcs given), else shs = [P,1,3]. */
int fr_pack_geom(int32_t P, const float *means3D, const float *scales, const float *rotations, const float *opacities,
	int32_t levels, const float *highest_levels, float *packed_geom, void *stream);
int fr_pack_cull(int32_t P, const float *means3D, const float *scales, const float *rotations, float *packed_cull, void *stream);
int fr_pack_colour(int32_t P, const float *shs, const float *shs_rest, const float *shs_dcs, float *packed_colour, void *stream);
/* RF with fr_foveation.levels = 1 .. 4: fr_pack_colour for shs_dcs [P,levels,3] (the missing levels' slots are zero; nobody reads
 * them). fr_pack_geom takes the level count already. The packed layout has room for four levels: none for levels > 4. */
int fr_pack_colour_fov(int32_t P, const float *shs, const float *shs_dcs, int32_t levels, float *packed_colour, void *stream);
int fr_backward(const fr_backward_args *args);
/* Zero-fill the dense gradient tensors named in `args` (the dL_d* pointers with P, M, shs / shs_rest / colors_precomp as fr_backward
 * would be called; nothing else is read) with one kernel on `fill_stream`; pair with fr_backward_args.outputs_zeroed. No-op for
 * row_sparse. */
int fr_backward_prefill(const fr_backward_args *args, void *fill_stream);
/* The backward pass of the mask-learning step (extension; metric_mask_learn.py:213 renders with masking=True, and
 * gaussian_renderer/__init__.py:71-82 then detaches positions, scales, rotations and the rest SH coefficients): gradients of the
 * OPACITY and of the DC COLOUR only, over the forward state fr_backward would use, with the same `args` struct. The tile pass sums
 * four values per (band, entry) pair instead of nine (colour r g b and M00), and a per-Gaussian pass without SH rows or chain rule
 * writes 16 bytes per visible Gaussian.
 *   dL_dopacity  [P,1], required; w.r.t. the raw parameter with raw_activations.
 *   dL_dsh       optional, ALWAYS the DC gradient [P,1,3], whether shs is concatenated [P,M,3] or split (shs_rest given):
 *                SH_C0 * dL/dcolour, zero for a channel the forward pass clamped (backward.cu:20-139). Needs shs.
 *   dL_dcolor    optional, [P,3]: dL/dcolour (with colors_precomp: the input's gradient).
 *   every other dL_d* pointer (dL_dmean2D, dL_dconic, dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot, dL_dsh_rest) must be NULL:
 *   FR_ERR_INVALID, the message names the field.
 * Variants, raw_activations, row_sparse (the outputs are then [C,1] / [C,1,3] / [C,3], every row written), outputs_zeroed,
 * stage_events ([0] [1] [2] around the two passes, [3] [4] around the zero fill, which runs on `stream` in front of them) and
 * blend_pairs as for fr_backward; dense outputs are written in full, zero rows included. num_ranges is ignored: the per-Gaussian
 * pass runs in one piece and range_done, when given, is called exactly once as range_done(range_user, 0, 0, P) behind its launch
 * (not with row_sparse, not with P == 0). The per-Gaussian sums the call reads are cleared again, so any mix of fr_backward and
 * fr_backward_appearance calls over one forward state gives each call's gradients as a single call would. Never synchronises.
 * radii, means3D, scales, rotations, cov3D_precomp, opacities and the matrices are not read. */
int fr_backward_appearance(const fr_backward_args *args);

/* ---- Appearance backward pass of the FOVEATED renderer (extension; FR_VARIANT_FOV_PCHECK_OBB) ----
 * The reference's foveated extension is inference-only (…_fov_pcheck_obb/diff_gaussian_rasterization_fov_pcheck_obb/
 * __init__.py:128-187 returns None for every input). Here the per-level APPEARANCE parameters of the composed model -- opacities
 * [P,L] and shs_dcs [P,L,3], what the mask-learning loop learns and all that masking=True differentiates
 * (gaussian_renderer/__init__.py:71-82) -- get a gradient through the renderer that consumes them. The arithmetic is the
 * reference's RS / R0 backward (cuda_rasterizer/backward.cu:399-557, restricted as fr_backward_appearance restricts it) applied to
 * the forward pass of …_fov_pcheck_obb/cuda_rasterizer/forward.cu:262-609:
 *   single-level tile, level l = int(tile_min): pixel = C_l + T_l bg; Gaussian g takes part with opacities[g][l] and
 *     colour[g][l] = max(0, SH_C0 shs_dcs[g][l] + rest SH + 0.5);
 *   two-level tile (l1, l2 = l1 + 1): pixel = w1 (C_1 + T_1 bg) + (1 - w1)(C_2 + T_2 bg) (forward.cu:455-470); w1 depends on the
 *     tile's geometry and the settings only, so state 1 receives w1 dL/dpixel and state 2 (1 - w1) dL/dpixel; state 1 of a pixel
 *     with est > l2 starts finished (T = 1, no contributor); state 2 skips every Gaussian with highest_level + 1 < tile_min + 1
 *     (forward.cu:399);
 *   per blended (pixel, state, Gaussian) pair: dL/dcolour[g][l] += alpha T dL/dpix, dL/dalpha from the colour behind the entry and
 *     the background term, dL/dopacities[g][l] += G dL/dalpha; the saturation alpha = min(0.99, o G) is not differentiated
 *     (backward.cu:497-541).
 *
 * fr_forward_begin_fov_keep / fr_forward_fov_keep_call: fr_forward_begin_fov / fr_forward_fov_call that also KEEP what the backward
 * pass needs. Image and radii are those of the plain call bit for bit (the same blend; a second instantiation of the blend kernel
 * that also stores, per pixel and level state, the transmittance the state ended with and the list position of its last
 * contributor -- final_T / n_contrib of forward.cu:267-384 per state). The resize callbacks are asked for LARGER geometry and image
 * workspaces, fr_geometry_bytes_fov_keep / fr_image_bytes_fov_keep: the plain call's layout with, behind it, one 64-byte row of
 * gradient sums per Gaussian resp. two planes of each of the two per-state arrays; fr_geometry_bytes_fov / fr_image_bytes and every
 * introspection pointer answer what they answered. `state` (size = sizeof(fr_fov_state) as the caller was compiled) is filled by
 * fr_forward_finish (by the call itself with fr_forward_fov_keep_call) and must stay where it is until then; it is valid for as
 * long as the three workspaces are left alone.
 * Refused with FR_ERR_INVALID before anything is enqueued, the message names the field: a variant other than
 * FR_VARIANT_FOV_PCHECK_OBB; fr_foveation.levels > 4 (levels 5 .. 8 would need a second row of sums per Gaussian); a packed model
 * (packed_geom / packed_colour / packed_cull: training renders from the ordinary tensors); state NULL or its size too small. */
typedef struct fr_fov_state {
	uint32_t size;                  /* in: sizeof(fr_fov_state) */
	int32_t variant;                /* out, all below: FR_VARIANT_FOV_PCHECK_OBB */
	int32_t P, W, H;
	int32_t levels;                 /* fr_foveation.levels (4 without settings) */
	int32_t num_rendered;           /* fr_forward_args.num_rendered */
	int32_t num_items;              /* blend work items of the frame (tile << 3 | band | level state << 1 | two-level << 2) */
	float start_blend, blend_width; /* fr_foveation */
	char *geometry, *binning, *image; /* the workspaces the resize callbacks returned */
} fr_fov_state;
int fr_forward_begin_fov_keep(fr_forward_args *args, const fr_forward_ext *ext, const fr_foveation *fov, fr_fov_state *state, fr_frame **frame);
int fr_forward_fov_keep_call(fr_forward_args *args, const fr_forward_ext *ext, const fr_foveation *fov, fr_fov_state *state);
size_t fr_geometry_bytes_fov_keep(int32_t P, int32_t levels);
size_t fr_image_bytes_fov_keep(int32_t W, int32_t H);
/* introspection (tests): the kept per-state planes, [2][W*H] each: plane 0 = the state of a single-level tile / state 1 of a
 * two-level tile, plane 1 = state 2 (written in two-level tiles only) */
const float *fr_image_fov_state_T(int32_t W, int32_t H, const char *image);
const uint32_t *fr_image_fov_state_n(int32_t W, int32_t H, const char *image);
/* fr_backward_fov_appearance: the gradients over a kept forward state. size = sizeof(fr_backward_fov_args).
 *   state               the forward call's, unchanged
 *   background [3], dL_dpix [3,H,W]   required (background: what the forward call blended with)
 *   dL_dopacities       [P,L], required
 *   dL_dshs_dcs         [P,L,3], required: SH_C0 dL/dcolour[g][l], zero for a channel the forward pass clamped at that level
 *                       (backward.cu:20-139; a pre-clamp value of exactly 0 counts as clamped)
 *   dL_dlevel_colours   [P,L,3] or NULL: dL/dcolour[g][l]
 *   stage_events        optional [3]: recorded on `stream` in front of the tile pass, between the two passes and behind them
 *   blend_pairs         optional [T] diagnostic as fr_backward_args.blend_pairs
 * L = state->levels: the outputs have the model's own width. Every output is written in full: rows of Gaussians outside the
 * frame's visible list, of Gaussians that landed in no tile, and levels no tile used are exact zeros. A tile pass over the forward's
 * work items (longest list first; a few lanes' float atomics into one or two 64-byte rows per entry pair, as fr_backward_appearance's)
 * and a per-Gaussian pass that clears the sums it read: a second call over the same state gives the same gradients. Never
 * synchronises. FR_ERR_INVALID before anything is enqueued, naming the field: state NULL / of another variant / with levels > 4, a
 * required pointer NULL. */
typedef struct fr_backward_fov_args {
	uint32_t size;
	int32_t debug;
	const fr_fov_state *state;
	const float *background;
	const float *dL_dpix;
	float *dL_dopacities;
	float *dL_dshs_dcs;
	float *dL_dlevel_colours;
	void *stream;
	void **stage_events;
	uint32_t *blend_pairs;
} fr_backward_fov_args;
int fr_backward_fov_appearance(const fr_backward_fov_args *args);

/* The FULL backward pass of the foveated renderer (extension): beside the per-level appearance parameters, the shared geometry
 * (means3D, scales, rotations) and the rest SH coefficients of a composed model get their gradients through the renderer that ships
 * it. The derivative is the one fr_backward_fov_appearance takes (above: w1 a constant, state 1 starting finished where est > l2,
 * the upper state's existence skip, the power < -4.5 cutoff, the undifferentiated min(0.99, o G), T recovered by division, the
 * background term); per blended (pixel, level state, Gaussian) pair it forms the nine values of backward.cu:503-554. The three
 * colour sums and M00 are the state's LEVEL's (the level's quarter of the item's row, as above); the five moments M10 M01 M20 M11
 * M02 are the GAUSSIAN's: they are summed over every level state that blends it, with dL/dG = o_l dL/dalpha_l, into a second row.
 *
 * fr_forward_begin_fov_keep_full / fr_forward_fov_keep_full_call: the state-keeping forward with a LARGER geometry workspace,
 * fr_geometry_bytes_fov_keep_full: the keep layout with, behind it, one 32-byte row of moments per Gaussian (the image workspace is
 * fr_image_bytes_fov_keep's). Image and radii are those of the plain call bit for bit (the same kernels as the keep call). Nothing
 * else is kept: the chain rule RECOMPUTES the 3D covariance from the scales and rotations it is handed (the inference frame's
 * geometry rows have no room for it), so fr_backward_fov must be given the model the forward call rendered. The state's variant reads
 * FR_VARIANT_FOV_PCHECK_OBB | FR_FOV_STATE_FULL; fr_backward_fov_appearance REFUSES such a state (its variant test), and
 * fr_backward_fov refuses a plain keep state: each pass clears only the rows it owns. Refusals as fr_forward_begin_fov_keep's. */
#define FR_FOV_STATE_FULL 0x100
int fr_forward_begin_fov_keep_full(fr_forward_args *args, const fr_forward_ext *ext, const fr_foveation *fov, fr_fov_state *state, fr_frame **frame);
int fr_forward_fov_keep_full_call(fr_forward_args *args, const fr_forward_ext *ext, const fr_foveation *fov, fr_fov_state *state);
size_t fr_geometry_bytes_fov_keep_full(int32_t P, int32_t levels);
/* fr_backward_fov: size = sizeof(fr_backward_fov_full_args).
 *   state                 the _full forward call's, unchanged
 *   P, M, sh_degree       Gaussians (= state->P), SH coefficients per Gaussian INCLUDING the DC one (16: shs_rest is [P,M-1,3]), active degree
 *   means3D [P,3], scales [P,3], rotations [P,4]   required: the activated inputs of the forward call
 *   shs_rest [P,M-1,3]    required when M > 1
 *   viewmatrix, projmatrix [16], campos [3], background [3], dL_dpix [3,H,W]   required; tanfovx / tanfovy / scale_modifier as forward
 *   dL_dopacities [P,L], dL_dshs_dcs [P,L,3]       required, as fr_backward_fov_appearance's; dL_dlevel_colours [P,L,3] or NULL
 *   dL_dshs_rest [P,M-1,3] required when M > 1: the SH backward (backward.cu:20-139) applied to the sum over the item's level range
 *                         of [colour_l > 0] dL/dcolour_l; coefficients above sh_degree are exact zeros
 *   dL_dmeans3D [P,3]     required: view-direction term of the SH backward (fed with the same masked sum) + projection term
 *                         (backward.cu:346-396) + covariance term (backward.cu:144-274: clamped tangents and the 1e-7 guard as there)
 *   dL_dscales [P,3], dL_drotations [P,4]          required: w.r.t. the activated inputs, scale_modifier honoured (backward.cu:278-341;
 *                         dL_dscales is the reference's dL/d(scale_modifier scale), as fr_backward's: backward.cu:295-325)
 *   dL_dmeans2D [P,3]     required: as fr_backward returns it (x, y in NDC units, third component 0); dL_dconic [P,4] or NULL
 *   stage_events          optional [3]: in front of the tile pass, between the passes, behind them; blend_pairs optional [T]
 * Every output is dense and written in full, zero rows included: ONE fill over all of them in front of the tile pass, then plain
 * stores of the visible rows (the whole-line scheme of fr_backward is tied to k_preprocess_bwd's staging; chosen for simplicity, as
 * fr_backward_appearance). The per-Gaussian pass clears the sums it read: a second call over one state repeats the first. Never
 * synchronises. FR_ERR_INVALID before anything is enqueued, naming the field: state NULL / of another variant / not made by the
 * _full forward / with levels > 4; P != state->P; a required pointer NULL. (A packed model cannot get here: the _full forward
 * refuses packed_geom / packed_colour / packed_cull.) */
typedef struct fr_backward_fov_full_args {
	uint32_t size;
	int32_t debug;
	const fr_fov_state *state;
	int32_t P, M, sh_degree;
	float tanfovx, tanfovy, scale_modifier;
	const float *means3D, *scales, *rotations, *shs_rest;
	const float *viewmatrix, *projmatrix, *campos;
	const float *background;
	const float *dL_dpix;
	float *dL_dopacities, *dL_dshs_dcs, *dL_dlevel_colours;
	float *dL_dshs_rest, *dL_dmeans3D, *dL_dscales, *dL_drotations, *dL_dmeans2D, *dL_dconic;
	void *stream;
	void **stage_events;
	uint32_t *blend_pairs;
} fr_backward_fov_full_args;
int fr_backward_fov(const fr_backward_fov_full_args *args);

int fr_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, const float *projmatrix,
	uint8_t *present /* [P] bool */, void *stream);

/* The parameter activations in front of the rasterizer in a training iteration, one pass each way (SURVEY.md 8f rank 3;
 * replaces GaussianModel.get_scaling / get_rotation / get_opacity, fov3dgs/scene/gaussian_model.py:200-240, i.e.
 * exp [P,3], x / max(|x|, 1e-12) [P,4], sigmoid [P,1], and their autograd). Backward: dL_d* are the gradients w.r.t. the
 * activated values (NULL = zero), dL_draw_* the results, written in full. */
int fr_activate_forward(int32_t P, const float *raw_scaling, const float *raw_rotation, const float *raw_opacity, float *scaling, float *rotation,
	float *opacity, void *stream);
int fr_activate_backward(int32_t P, const float *raw_scaling, const float *raw_rotation, const float *raw_opacity, const float *dL_dscaling,
	const float *dL_drotation, const float *dL_dopacity, float *dL_draw_scaling, float *dL_draw_rotation, float *dL_draw_opacity, void *stream);

/* Image loss of a training iteration, fused (replaces fov3dgs/utils/loss_utils.py:17-18 l1_loss and
 * :37-76 ssim as eff_finetune.py:124-125 combines them). img / target: [C,H,W] fp32 device tensors.
 *   forward:  partials[b] = (sum |img - target|, sum ssim_map) over tile b (16 x 32 pixels) of one channel,
 *             b < fr_l1_ssim_blocks(C,H,W); the caller adds them up (l1 = sum0 / (C H W), ssim = sum1 / (C H W)).
 *             dmaps [3,C,H,W] (optional, NULL = value only) keeps what the backward needs.
 *   finish:   out[0..2] = (loss, l1, ssim) from the partials on the device (sums in double, in block order: the same
 *             numbers on every run): l1 = sum0 / (C H W), ssim = sum1 / (C H W), loss = (1-lambda) l1 + lambda (1 - ssim).
 *   backward: dL_dimg = s (w_l1 * sign(img - target) + w_ssim * d(sum ssim_map)/d img), written in full; s = *grad_scale
 *             (a DEVICE scalar: the upstream gradient of the loss, read by the kernel -- no host round trip, no extra
 *             pass over the image) or 1 when grad_scale is NULL.
 *             For loss = (1-l) L1 + l (1 - SSIM): w_l1 = (1-l) / (C H W), w_ssim = -l / (C H W). */
int64_t fr_l1_ssim_blocks(int32_t C, int32_t H, int32_t W);
int fr_l1_ssim_forward(int32_t C, int32_t H, int32_t W, const float *img, const float *target, float *dmaps, float *partials, void *stream);
int fr_l1_ssim_finish(int32_t C, int32_t H, int32_t W, const float *partials, float lambda_dssim, float *out3, void *stream);
int fr_l1_ssim_backward(int32_t C, int32_t H, int32_t W, const float *img, const float *target, const float *dmaps, float w_l1, float w_ssim,
	const float *grad_scale, float *dL_dimg, void *stream);

/* The uniform metameric (HVS) loss, fused (csrc/hvs.hip): MetamericLossUniform with bilinear_downsampling=True and the cropped
 * 5x5 filters, the loss of metric_mask_learn.py:227 and eff_finetune.py:122. Restated from
 *   metamer/odak_perception/metameric_loss_uniform.py:8-12 (uniform_blur: area-down by 1/p, bilinear-up), :57-69 (mean, var =
 *     E[x^2] - mean^2 floored at 1e-7, std), :71-88 (the statistics: h, every band with p halved per level, the last lowpass),
 *     :90-100 (mean over the statistics of their L1 / MSE mean), :135-156 (the call: the target is detached),
 *   metamer/odak_perception/spatial_steerable_pyramid.py:6-31 (sizes must be multiples of 2^levels), :132-180 (the pyramid),
 *   metamer/odak_perception/color_conversion.py:382-404 (RGB -> YCrCb).
 * img / target: [3,H,W] fp32 device tensors (rgb != 0: converted to YCrCb first). n_levels 2..6, n_orientations 1..8, H and W
 * multiples of 2^n_levels (else FR_ERR_INVALID), pooling_size > 0, mse != 0: MSE instead of L1.
 * filters: DEVICE buffer of (2 + n_orientations) * 25 floats = l0, h0, b_0 .. (row-major 5x5, as get_steerable_pyramid_filters(5,
 *   n, "cropped") returns them). The library holds no coefficients of its own.
 * fr_hvs_workspace_floats(.., which): floats of 0 = one picture's forward state, 1 = the backward workspace, 2 = the partial
 *   sums; -1 for bad arguments (fr_last_error says which).
 * forward:  builds img's state (bands, pooled mean / mean-square per band, lowpasses) in state_img and, unless target is NULL,
 *   the target's in state_target (NULL: state_target holds that target's state from an earlier call with the same settings);
 *   compares them and writes the loss to out[0]. The per-workgroup sums in `partials` are added in double in a fixed order.
 * backward: dL_dimg [3,H,W] = s * d loss / d img, written in full, from the two states of the forward; s = *grad_scale (a
 *   DEVICE scalar, the upstream gradient) or 1 when grad_scale is NULL. Every sum is a gather: the same bits on every run.
 * All launches go to `stream`; their number depends on n_levels only. */
int64_t fr_hvs_workspace_floats(int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations, int32_t which);
int fr_hvs_forward(int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations, int32_t mse, int32_t rgb,
	const float *filters, const float *img, const float *target, float *state_img, float *state_target, float *partials, float *out, void *stream);
int fr_hvs_backward(int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations, int32_t mse, int32_t rgb,
	const float *filters, const float *state_img, const float *state_target, float *workspace, const float *grad_scale, float *dL_dimg, void *stream);

/* The same loss of pictures that are first resized to the pyramid's size, the resize inside the kernels: what
 * F.interpolate(x, size=(H, W), mode='bilinear', align_corners=False) followed by the calls above computes
 * (metric_mask_learn.py:221-227, eff_finetune.py:116-122, prune.py:128-134), with no resized picture in memory and no atomics.
 * img / target: [3,Hs,Ws] fp32 device tensors. H, W: the size the loss runs at, multiples of 2^n_levels; Hs <= H and Ws <= W
 *   (a smaller H or W -- shrinking -- is FR_ERR_INVALID; an axis of equal size is the identity exactly; Hs == H and Ws == W is
 *   the plain call). Every other argument is fr_hvs_forward's / fr_hvs_backward's.
 * forward_resized:  the level-0 load samples the pictures bilinearly (src = (Hs / H) (y + .5) - .5, negative -> 0, the second tap
 *   clamped at the last row / column; R, G and B are interpolated, in double and kept in fp32, then the colour is converted).
 *   state_img / state_target / partials have the layout and sizes of the H x W call (fr_hvs_workspace_floats(H, W, ..)).
 * backward_resized: dL_dimg [3,Hs,Ws] = s * d loss / d img, written in full: the H x W gradient goes to the workspace and a
 *   gather per SOURCE pixel applies the transposed resize (weights added in ascending row, then column order: the same bits on
 *   every run). workspace: fr_hvs_resized_backward_floats(..) floats = the plain backward workspace + 3 H W (+ 0 when nothing
 *   is resized); -1 for bad arguments (fr_last_error says which). One launch more than fr_hvs_backward. */
int fr_hvs_forward_resized(int32_t Hs, int32_t Ws, int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations,
	int32_t mse, int32_t rgb, const float *filters, const float *img, const float *target, float *state_img, float *state_target, float *partials,
	float *out, void *stream);
int fr_hvs_backward_resized(int32_t Hs, int32_t Ws, int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations,
	int32_t mse, int32_t rgb, const float *filters, const float *state_img, const float *state_target, float *workspace, const float *grad_scale,
	float *dL_dimg, void *stream);
int64_t fr_hvs_resized_backward_floats(int32_t Hs, int32_t Ws, int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations);

/* The foveated (gaze-dependent) metameric loss, fused (csrc/hvs_fov.hip): MetamericLoss with use_bilinear_downup=True,
 * use_l2_foveal_loss=False, use_radial_weight=False, use_fullres_l0=False, equi=False and the cropped 5x5 filters, the "HVS FOV"
 * figure of hvs_loss_calc.py:21-75. The uniform loss above with another blur: every pixel of a band level has its own level of
 * detail lod = max(0, log2(1e-6 + pooling size in pixels)) from the gaze, the level's own size and alpha, real_image_width,
 * real_viewing_distance and mode (1 = "quadratic", 0 = "linear"), and the blur blends levels floor(lod) and floor(lod) + 1 of
 * the band's mip chain (successively area-halved copies, each bilinearly sampled at the pixel; the last level, always 1x1, is
 * a constant and also serves every lod beyond it). Restated from
 *   metamer/odak_perception/foveation.py:6-179, radially_varying_blur.py:23-140, metameric_loss.py:86-191, :204-271.
 * gaze_x, gaze_y: normalised image coordinates, x first; they may lie outside [0, 1].
 * Hs, Ws: 0, 0 = img / target are [3,H,W]; else they are [3,Hs,Ws] and are resized to H x W in the level-0 load, as in
 *   fr_hvs_forward_resized (Hs <= H, Ws <= W). H and W are multiples of 2^n_levels, and every band level's chain must end at
 *   1x1 or 1x2: any other size is FR_ERR_INVALID (fr_last_error names the level and its size; the reference itself fails there).
 * fr_hvs_fov_workspace_floats(.., which): floats of 0 = one picture's forward state (bands, both mip chains, lowpasses),
 *   1 = the backward workspace, 2 = the partial sums, 3 = the LOD maps (doubles: two floats each; 8-byte aligned; behind the
 *   maps, every level's largest value, from which the backward pass knows the chain levels that no pixel blends);
 *   -1 for bad arguments.
 * forward:  as fr_hvs_forward. lod: the LOD maps of every band level; lod_valid != 0 = it holds the maps of exactly these H, W,
 *   n_levels, alpha, real_image_width, real_viewing_distance, mode and gaze from an earlier call and is not rebuilt, else the
 *   call fills it (kernels on `stream`; a gaze change costs no host synchronisation).
 * backward: as fr_hvs_backward / fr_hvs_backward_resized, from the two states and the LOD maps of the forward. Every sum is a
 *   gather in a fixed order, with no atomics and no zero fill: the same bits on every run.
 * The number of launches depends on H, W and n_levels only.
 * fr_hvs_fov_backward_plan(.., level, k, out): host only, no GPU call. What the backward pass does at chain level k (1 .. K) of
 *   pyramid level `level` (0 .. n_levels - 2) of an H x W call, as ten numbers: out[0] = K, the chain's last level; out[1], out[2] =
 *   h_k, w_k; out[3], out[4] = rows, cols, the bound of a texel's footprint in pixels that the next three were sized for;
 *   out[5] = G, the lanes that share a texel (1, 8 or 64); out[6] = S, the row slices a footprint is cut into, and out[7] = R, the
 *   rows of a slice (the last slice runs to the footprint's end); out[8] = the offset in floats of g[k], [2,nmc,h_k,w_k] (the
 *   gradient of the mean chain, then of the chain of the square; nmc = 3 n_orientations, + 3 at level 0), in the backward
 *   workspace, out[9] = that of the slices' partial sums, [S,2,nmc,h_k,w_k]. Both are valid after fr_hvs_fov_backward (the
 *   offsets do not depend on Hs, Ws). FR_ERR_INVALID for a size fr_hvs_fov_workspace_floats refuses, a level or k out of range
 *   or a null out. For tests and tools. */
int64_t fr_hvs_fov_workspace_floats(int32_t Hs, int32_t Ws, int32_t H, int32_t W, int32_t n_levels, int32_t n_orientations, int32_t which);
int fr_hvs_fov_backward_plan(int32_t H, int32_t W, int32_t n_levels, int32_t n_orientations, int32_t level, int32_t k, int64_t *out);
int fr_hvs_fov_forward(int32_t Hs, int32_t Ws, int32_t H, int32_t W, double alpha, double real_image_width, double real_viewing_distance,
	int32_t mode, double gaze_x, double gaze_y, int32_t n_levels, int32_t n_orientations, int32_t mse, int32_t rgb, const float *filters,
	const float *img, const float *target, float *state_img, float *state_target, float *lod, int32_t lod_valid, float *partials, float *out,
	void *stream);
int fr_hvs_fov_backward(int32_t Hs, int32_t Ws, int32_t H, int32_t W, double alpha, double real_image_width, double real_viewing_distance,
	int32_t mode, double gaze_x, double gaze_y, int32_t n_levels, int32_t n_orientations, int32_t mse, int32_t rgb, const float *filters,
	const float *state_img, const float *state_target, const float *lod, float *workspace, const float *grad_scale, float *dL_dimg, void *stream);

/* The metamer of a target at a gaze, fused (csrc/metamer.hip): MetamerMSELoss with avg_pooling_downup=True (the bilinear
 * pyramid of the two losses above), equi=False and the cropped 5x5 filters -- the steerable pyramid's SYNTHESIS, which the two
 * losses above never need. filters, mode, gaze, alpha and the display geometry are fr_hvs_fov_forward's; the sizes it refuses are
 * refused here (H, W multiples of 2^n_levels, n_levels 2..6, n_orientations 1..8, every level's mip chain ending at 1x1 or 1x2).
 * fr_hvs_metamer replaces MetamerMSELoss.gen_metamer (metamer/odak_perception/metamer_mse_loss.py:63-123) and what it calls:
 *   MetamericLoss.calc_statsmaps (metameric_loss.py:86-167), construct_pyramid (spatial_steerable_pyramid.py:132-180) of target
 *   and noise, match_level (metamer_mse_loss.py:97-107), reconstruct_from_pyramid (spatial_steerable_pyramid.py:182-223) and
 *   ycrcb_2_rgb (color_conversion.py:424-427).
 *   target [3,H,W]: rgb = 1 RGB (converted as rgb_2_ycrcb does), 0 = already YCrCb. noise [3,H,W]: the picture whose pyramid is
 *   matched, used as it is (the reference draws rand_like of the YCrCb target). out [3,H,W]: the metamer in RGB, not clamped.
 *   h and every oriented band of the noise's pyramid become (band - mean) / max(rms, 1e-6) * std(y, x) + mean(y, x): ONE mean and
 *   ONE root mean square of the centred values per band, over its three channels, summed in double in a fixed order (partials
 *   per workgroup, one finishing workgroup); std and mean the target's blended statistics at the pixel, as the foveated loss
 *   forms them (variance floored at 1e-7), evaluated in the matching kernel. The last lowpass is the target's.
 *   Everything is enqueued on `stream`: no host synchronisation, no allocation, no float atomics, the same bits on every run.
 * fr_hvs_metamer_roundtrip replaces reconstruct_from_pyramid(construct_pyramid(x)) (spatial_steerable_pyramid.py:132-223): the
 *   synthesis from the picture's own pyramid, no noise and no matching. rgb = 1: x is RGB, converted on the way in and back on
 *   the way out; 0: the three channels as they are.
 * fr_hvs_metamer_workspace_floats(.., roundtrip): floats of the caller-owned workspace (8-byte aligned: it starts with doubles)
 *   of fr_hvs_metamer (roundtrip = 0) or fr_hvs_metamer_roundtrip (1); -1 for bad arguments.
 * The loss, MetamerMSELoss.__call__'s torch.nn.L1Loss / MSELoss (metamer_mse_loss.py:146-152; mse = 0 / 1) over n = 3 H W elements:
 *   forward:  one launch. out[0] = mean |image - metamer| or mean (image - metamer)^2, summed in double in a fixed order.
 *             workspace: fr_hvs_metamer_loss_workspace_doubles(n) doubles, ZERO before the first use; every call leaves the one
 *             word it needs zero (the last one) zero again, so the buffer serves call after call on one stream.
 *   backward: one elementwise launch. dL_dimage = grad_scale[0] (a device scalar; NULL = 1) times sign(d) / n or 2 d / n.
 * Every malformed argument is FR_ERR_INVALID before anything is enqueued; fr_last_error names the argument. */
int64_t fr_hvs_metamer_workspace_floats(int32_t H, int32_t W, int32_t n_levels, int32_t n_orientations, int32_t roundtrip);
int fr_hvs_metamer(int32_t H, int32_t W, double alpha, double real_image_width, double real_viewing_distance, int32_t mode,
	double gaze_x, double gaze_y, int32_t n_levels, int32_t n_orientations, int32_t rgb, const float *filters, const float *target,
	const float *noise, float *workspace, float *out, void *stream);
int fr_hvs_metamer_roundtrip(int32_t H, int32_t W, int32_t n_levels, int32_t n_orientations, int32_t rgb, const float *filters,
	const float *image, float *workspace, float *out, void *stream);
int64_t fr_hvs_metamer_loss_workspace_doubles(int64_t n);
int fr_hvs_metamer_loss_forward(int64_t n, int32_t mse, const float *image, const float *metamer, double *workspace, float *out, void *stream);
int fr_hvs_metamer_loss_backward(int64_t n, int32_t mse, const float *image, const float *metamer, const float *grad_scale,
	float *dL_dimage, void *stream);

/* Mean squared distance of every point to its three nearest neighbours: simple-knn's distCUDA2, the initial scale of
 * GaussianModel.create_from_pcd (replaces SimpleKNN::knn, fov3dgs/submodules/simple-knn/simple_knn.cu:185-220, as called by
 * distCUDA2, spatial.cu:15-25). points: [P,3] fp32 device array; mean_dist2: [P] fp32, written in full:
 *   mean_dist2[i] = ((b0 + b1) + b2) / 3.0f, b0 <= b1 <= b2 the three smallest d(i,j) = (dx*dx + dy*dy) + dz*dz over j != i
 *   (dx = p_j.x - p_i.x, no fma), a missing neighbour counting as FLT_MAX (P = 3: about FLT_MAX / 3, P <= 2: +inf);
 *   exact duplicates count at distance 0. The search is exact, so the result is one bit pattern, run after run.
 *   A point with a non-finite coordinate gets NaN and is nobody's neighbour.
 * workspace: fr_knn_workspace_bytes(P) bytes of device memory, 16-byte aligned (the library allocates nothing). Everything
 * runs on `stream`, with no host synchronisation. P = 0 launches nothing. */
size_t fr_knn_workspace_bytes(int32_t P);
int fr_knn_mean_dist2(int32_t P, const float *points, float *mean_dist2, void *workspace, void *stream);

/* The optimizer step of a training iteration: Adam over every parameter tensor of the model in one kernel launch (replaces
 * torch.optim.Adam(l, lr=0.0, eps=1e-15), fov3dgs/scene/gaussian_model.py:289, as stepped by eff_finetune.py:147). No
 * weight decay, amsgrad or maximize: the reference uses none. Per element, in torch's order of operations, every operation
 * rounded once:
 *   m = fma(one_minus_beta1, g - m, m);  v = fma(one_minus_beta2, g * g, v * beta2);   (the fusions of torch's GPU kernels)
 *   p += neg_step_size * (m / (sqrt(v) / bias_correction2_sqrt + eps))
 * with neg_step_size = -lr / (1 - beta1^t) and bias_correction2_sqrt = sqrt(1 - beta2^t) computed by the caller in double.
 * Everything runs on `stream` with no host synchronisation and no allocation; the table travels in the kernel arguments. */
#define FR_ADAM_MAX_TENSORS 16
enum {
	FR_ADAM_DENSE = 0, /* grad: [numel] */
	FR_ADAM_EXACT = 1, /* row-sparse grad, a row without an entry has gradient zero: every row decays and moves (= dense Adam on to_dense()) */
	FR_ADAM_LAZY = 2   /* row-sparse grad, only the listed rows of param / exp_avg / exp_avg_sq are read or written */
};

/* One parameter tensor of the step (replaces one entry of the param_groups of gaussian_model.py:289). All pointers are
 * device pointers to contiguous data; param, exp_avg, exp_avg_sq: fp32 [numel], updated in place. Row-sparse modes: the
 * tensor is [numel / width, width], grad holds the n_rows compact rows [n_rows, width] and rows [n_rows] their row numbers,
 * strictly increasing (a coalesced torch.sparse_coo gradient with one sparse dimension). A row number outside
 * [0, numel / width) is skipped, never dereferenced. */
typedef struct fr_adam_tensor {
	float *param, *exp_avg, *exp_avg_sq;
	const float *grad;
	const int64_t *rows; /* NULL in dense mode */
	int32_t *row_map;    /* exact mode, optional: scratch int32 [numel / width] for the row -> compact position lookup (filled
	                      * by the call, needs no initialisation; every tensor of a call that names it has the same rows, n_rows
	                      * and row count). NULL = binary search in rows */
	int64_t numel;
	int64_t n_rows;      /* 0 in dense mode */
	int32_t width;       /* elements per row (1 in dense mode) */
	int32_t mode;        /* FR_ADAM_* */
	float one_minus_beta1, beta2, one_minus_beta2;
	float bias_correction2_sqrt, eps, neg_step_size;
} fr_adam_tensor;

/* The whole step (replaces optimizer.step() over the six groups of gaussian_model.py:289). */
typedef struct fr_adam_args {
	int32_t num_tensors; /* 0 .. FR_ADAM_MAX_TENSORS */
	int32_t reserved;
	fr_adam_tensor tensors[FR_ADAM_MAX_TENSORS];
} fr_adam_args;

int fr_adam_step(const fr_adam_args *args, void *stream);

/* The pruning step of the Fov-3DGS loop (replaces metric_pruning, fov3dgs/prune.py:71-110 -- the same loop in
 * metric_mask_learn.py:72-111 -- and GaussianModel._prune_optimizer / prune_points, fov3dgs/scene/gaussian_model.py:624-664).
 * Everything runs on `stream` with no host synchronisation and no allocation, and every output is one bit pattern, run after
 * run. workspace: fr_prune_workspace_bytes(P) bytes of device memory, 16-byte aligned, shared by the select and the
 * compaction (a plan stays valid until the next plan or select on the same workspace). P = 0 launches nothing. */
#define FR_COMPACT_MAX_TENSORS 32
enum {
	FR_PRUNE_MAX_COMP_EFFICIENCY = 0, /* cur = counts < 1 ? 0 : contribs / ((float)counts + 1e-7f)          (prune.py:79-86) */
	FR_PRUNE_CONTRIB = 1              /* cur = contribs: the reference's "surface" and "max_contrib"; counts unused (prune.py:87-98) */
};
size_t fr_prune_workspace_bytes(int32_t P);

/* One view's update of the metric, in place (replaces prune.py:82-86 / :90-92 / :95-98):
 *   metrics[i] = metrics[i] < cur ? cur : metrics[i]        (a NaN cur leaves the old value)
 * contribs: [P] fp32 and counts: [P] int32 as the rasterizer returns them; every operation is rounded once in fp32, the
 * division correctly: the result equals the torch expression bit for bit. */
int fr_prune_metric_max(int32_t P, int32_t kind, const float *contribs, const int32_t *counts, float *metrics, void *stream);

/* The rows to prune (replaces the torch.sort, the index slice and the mask scatter of prune.py:101-107): mask [P] bytes,
 * written in full, with exactly k ones: the k smallest rows under the total order (key(m), index), where for the bit
 * pattern b of m  key = 0xFFFFFFFF (NaN), 0x80000000 (+0 or -0), ~b (sign bit set), b | 0x80000000 (otherwise) -- the
 * order of torch.sort(descending=False, stable=True). Inside a run of equal metrics the lowest indices go first. */
int fr_prune_select_lowest(int32_t P, const float *metrics, int64_t k, uint8_t *mask, void *workspace, void *stream);

/* Row compaction (replaces the 21 tensor[valid_points_mask] gathers of gaussian_model.py:629-664), in two calls so that the
 * caller can allocate between them. A row is kept when its mask byte is non-zero (invert = 0) or zero (invert != 0).
 *   plan: each workgroup's first destination row, into the workspace, and *count_out (a DEVICE int32) = the kept rows
 *         (P = 0 launches nothing and leaves *count_out unwritten).
 *   rows: out[j] = src[i_j] bitwise for the kept rows i_0 < i_1 < ..., for every tensor of the table in ONE launch; mask and
 *         invert are those of the plan. A row is row_words 4-byte words (0: the tensor is skipped); a destination row
 *         >= dst_rows is never written. */
typedef struct fr_compact_tensor {
	const void *src;   /* [P, row_words] words, contiguous */
	void *dst;         /* [dst_rows, row_words] words, contiguous; may be NULL when dst_rows or row_words is 0 */
	int32_t row_words;
	int32_t dst_rows;
} fr_compact_tensor;

typedef struct fr_compact_args {
	int32_t P;
	int32_t num_tensors; /* 0 .. FR_COMPACT_MAX_TENSORS */
	int32_t invert;
	int32_t reserved;
	const uint8_t *mask; /* [P] */
	void *workspace;     /* as given to fr_compact_plan */
	fr_compact_tensor tensors[FR_COMPACT_MAX_TENSORS];
} fr_compact_args;

int fr_compact_plan(int32_t P, const uint8_t *mask, int32_t invert, int32_t *count_out, void *workspace, void *stream);
int fr_compact_rows(const fr_compact_args *args, void *stream);

/* LightGaussian's global-significance pruning (csrc/significance.hip, csrc/prune.hip; replaces LightGaussian/prune.py:112-128
 * calculate_v_imp_score and scene/gaussian_model.py:776-782 prune_gaussians: two full torch.sorts for one element each, five
 * elementwise passes and a comparison). The per-view counts and scores come from the counting render (fr_forward_args.
 * gaussians_count). As above: caller's stream, no host synchronisation, no allocation, workspace = fr_prune_workspace_bytes(P),
 * P = 0 launches nothing, every output is one bit pattern.
 *   select_kth    *kth_out (a DEVICE word) = the element of rank k (0-based, ascending) under the total order of
 *                 fr_prune_select_lowest: what torch.sort(values, stable=True)[0][k] holds (a tie at zero gives +0.0, the NaN
 *                 class a quiet NaN). dtype: 0 = fp32, 1 = int32 (compared as integers: summed counts exceed 2^24). k outside
 *                 0 .. P-1 is FR_ERR_INVALID.
 *   mask_le       mask[i] = values[i] <= *threshold_dev: the IEEE comparison for fp32, so a NaN row is never marked
 *                 (gaussian_model.py:781). All rows tied with the threshold are marked: the number of ones is known on the
 *                 device only (fr_compact_plan counts them).
 *   volume        volume[i] = (s0 * s1) * s2 of scaling [P,3], each product rounded once (torch.prod(get_scaling, dim=1));
 *                 raw != 0: s = exp(raw scaling) first, the device expression of fr_activate_forward.
 *   v_importance  out[i] = powf(volume[i] / *kth_volume_dev, v_pow) * imp[i] (prune.py:126-127), the division correctly
 *                 rounded, nothing contracted. out may be volume. */
int fr_select_kth(int32_t P, const void *values, int32_t dtype, int64_t k, void *kth_out, void *workspace, void *stream);
int fr_mask_le(int32_t P, const void *values, int32_t dtype, const void *threshold_dev, uint8_t *mask, void *stream);
int fr_volume(int32_t P, const float *scaling, int32_t raw, float *volume, void *stream);
int fr_v_importance(int32_t P, const float *volume, const float *kth_volume_dev, float v_pow, const float *imp, float *out, void *stream);

/* LightGaussian's VecTree SH vector quantisation (csrc/vq.hip; replaces LightGaussian/vectree/vq.py:262-299 EuclideanCodebook.forward
 * in the configuration of vectree.py:44-51 -- one head, no projection, decay EMA, no dead-code threshold, temperature 0 -- the loop
 * of vectree.py:196-204 and the bit matrix of vectree.py:120-126). As above: caller's stream, no host synchronisation, no
 * allocation, no float atomics, every output one bit pattern, run after run.
 *   Input rows: row i of a call is feats[rows[i]] (feats: [N, D] fp32, row stride D; rows: n int32 (rows64 = 0) or int64 indices,
 *   or NULL: feats[i], N >= n). An index outside 0 .. N-1 is clamped into that range, never followed. weights, where given, are
 *   indexed like feats (weights[rows[i]]). 1 <= K <= 65536, 1 <= D <= 64, n < 2^31. workspace: fr_vq_workspace_bytes(n, K, D,
 *   training) bytes, 16-byte aligned; training = 0 suffices for nearest / gather, update and replace need training = 1.
 *   nearest   ind[i] = argmin_c ||x_i - e_c|| (vq.py:276-277: -cdist, argmax), ranked by ||e_c||^2 - 2 x_i . e_c with the dot product
 *             accumulated on the exact f32 matrix instruction (a fmaf chain over ascending d). An exact tie of two scores goes to
 *             the lower code. The n x K matrix is never formed.
 *   gather    quantize[i] = embed[ind[i]] (vq.py:280; to_half: rounded through fp16, vectree.py:95), dist2[i] = sum_d (x - e)^2
 *             from the differences, *loss = float(loss_weight * sum dist2 / (n D)) summed in double in a fixed order (vq.py:405-407).
 *             Each of quantize, dist2, loss may be NULL; feats may be NULL when only quantize is asked for.
 *   update    the training step on the codebook AS ASSIGNED (ind from nearest, before this call): w' = w n / sum w (vq.py:264; 1
 *             without weights), cluster_size = cluster_size decay + (1 - decay) sum_{ind = c} w' (:285-289), embed_sum = sum w' x
 *             (:292-294) in ascending row position, smoothed = (cluster_size + eps) / (sum cluster_size + K eps) sum cluster_size
 *             (:296), embed = embed decay + (1 - decay) embed_sum / smoothed (:298). A code with no member decays by `decay`.
 *   replace   the k <= 64 codes of smallest cluster_size are overwritten by the k input rows of largest weight, smallest with
 *             largest and so on (vectree.py:202-204, two torch.topk). Ties go to the lowest index in both selections.
 *   pack_bits / unpack_bits   `bits` (1 .. 16) per value, MSB first, values back to back: np.packbits of the reference's dec2bin
 *             matrix. out holds (count bits + 7) / 8 bytes, the last one zero-padded. */
size_t fr_vq_workspace_bytes(int64_t n, int32_t K, int32_t D, int32_t training);
int fr_vq_nearest(int64_t n, int32_t K, int32_t D, const float *feats, int64_t N, const void *rows, int32_t rows64, const float *embed,
	int32_t *ind, void *workspace, void *stream);
int fr_vq_gather(int64_t n, int32_t K, int32_t D, const float *feats, int64_t N, const void *rows, int32_t rows64, const float *embed,
	const int32_t *ind, int32_t to_half, float *quantize, float *dist2, float *loss, float loss_weight, void *workspace, void *stream);
int fr_vq_update(int64_t n, int32_t K, int32_t D, const float *feats, int64_t N, const void *rows, int32_t rows64, const float *weights,
	const int32_t *ind, float decay, float eps, float *embed, float *cluster_size, void *workspace, void *stream);
int fr_vq_replace(int64_t n, int32_t K, int32_t D, int32_t k, const float *feats, int64_t N, const void *rows, int32_t rows64,
	const float *weights, float *embed, const float *cluster_size, void *workspace, void *stream);
int fr_pack_bits(int64_t count, int32_t bits, const int32_t *values, uint8_t *out, void *stream);
int fr_unpack_bits(int64_t count, int32_t bits, const uint8_t *in, int32_t *values, void *stream);

/* The quality gate of the pruning loop (csrc/quality.hip; replaces test_ssim_loss / test_psnr_loss, fov3dgs/prune.py:137-174 --
 * two renders, the torch ssim and psnr and a host synchronisation per view -- and utils/image_utils.py:14-19 mse / psnr).
 * img / target: [C,H,W] fp32 device tensors. Everything runs on `stream` with no host synchronisation, no allocation and no
 * float atomics: every output is one bit pattern, run after run.
 *   forward: partials[3 b .. 3 b + 2] = (sum ssim_map, sum (img - target)^2, sum |img - target|) over tile b (16 x 32 pixels of
 *            one channel, channel-major), b < fr_quality_blocks(C,H,W) (0 for sizes the kernels do not take: C > 65535, ...).
 *            The SSIM map is the one of fr_l1_ssim_forward (loss_utils.py:37-76: 11x11 window, sigma 1.5, zero padding);
 *            with_ssim = 0 skips it and leaves the first sum 0. |img - target| and its tile sum are fp32, as in
 *            fr_l1_ssim_forward; the squared error is evaluated and added in double from the fp32 inputs.
 *   finish:  one workgroup. The C channels are `rows` consecutive groups of C / rows (rows = 1: the whole picture, what
 *            prune.py measures; rows = C: one value per channel, what image_utils.psnr returns for a [3,H,W] input). For group
 *            r, with n = (C / rows) H W and the sums added in double in tile order:
 *              per_view[4 (slot + r) .. + 3] = (ssim = sum0 / n, psnr = 20 log10(1 / sqrt(mse)), l1 = sum2 / n, mse = sum1 / n)
 *            psnr is evaluated in double and is +inf for mse = 0, as in the reference. per_view: float [capacity][4] owned by
 *            the caller; slot + rows <= capacity. accum (optional, NULL = none): double[4] owned by the caller,
 *            += (ssim, psnr, l1, 1) per group with the fp32 values above: the running sums over the views and the view count
 *            (zero it to reset). partials and accum must be 8-byte aligned. */
int64_t fr_quality_blocks(int32_t C, int32_t H, int32_t W);
int fr_quality_forward(int32_t C, int32_t H, int32_t W, int32_t with_ssim, const float *img, const float *target, double *partials, void *stream);
int fr_quality_finish(int32_t C, int32_t H, int32_t W, int32_t rows, const double *partials, float *per_view, int32_t slot, int32_t capacity,
	double *accum, void *stream);

/* The scale-decay loss of the pruning loop's training step (csrc/prune_step.hip; replaces prune.py:257-261 and its autograd):
 *   loss = mean_p( max_j s[p][j] * max(counts[p] - threshold, 0) ),  s = scaling (raw = 0: activated, as get_scaling returns it)
 *   or exp(scaling) (raw != 0: the log-scales, the exp is taken in the kernel). scaling: [P,3] fp32, counts: [P] int32 as the
 *   rasterizer's gs_count. A row with counts <= threshold adds exactly 0 to the value and gets a gradient of exactly 0.
 *   forward:  one launch that leaves a double per workgroup in partials[fr_scale_decay_blocks(P)] (8-byte aligned, owned by the
 *             caller) and a one-workgroup finish: *out (a DEVICE float) = the sum in double, in workgroup order, divided by P.
 *   backward: dL_dscaling [P,3], written in full: g (counts[p] - threshold)+ / P in the column of the row's maximum -- the
 *             lowest column among equals, torch.max's index -- times exp(scaling) there when raw != 0; 0 elsewhere.
 *             g = *grad_scale (a DEVICE scalar, the upstream gradient) or 1 when grad_scale is NULL.
 * No host synchronisation, no allocation, no float atomics. P must be positive. */
int64_t fr_scale_decay_blocks(int32_t P);
int fr_scale_decay_forward(int32_t P, const float *scaling, const int32_t *counts, int32_t threshold, int32_t raw, double *partials, float *out,
	void *stream);
int fr_scale_decay_backward(int32_t P, const float *scaling, const int32_t *counts, int32_t threshold, int32_t raw, const float *grad_scale,
	float *dL_dscaling, void *stream);

/* The opacity cap after a pruning round (csrc/prune_step.hip; replaces the device work of reset_opacity / reset_opacity_max /
 * reset_opacity_upper_bound, fov3dgs/scene/gaussian_model.py:421-431, :447-452, and the two zeros_like of
 * replace_tensor_to_optimizer, :609-622), one launch:
 *   out[i] = 1 / (1 + expf(-raw[i])) > max_opacity ? cap_logit : raw[i]      (the input's bits where it is not capped: a NaN
 *   stays; the reference passes those rows through logit(sigmoid()), which moves them by rounding noise)
 *   exp_avg[i] = exp_avg_sq[i] = 0                                            (either may be NULL: a group without state)
 * cap_logit: the caller's log(max / (1 - max)). max_opacity must lie inside (0, 1). P = 0 launches nothing. */
int fr_opacity_cap(int32_t P, const float *raw_opacity, float max_opacity, float cap_logit, float *out, float *exp_avg, float *exp_avg_sq,
	void *stream);

/* Densification: the steps of GaussianModel that add rows (fov3dgs/scene/gaussian_model.py:666-851, :865-867). Every decision
 * is taken per SOURCE row, so a whole densify_and_prune -- two torch.cat and two prune_points over the full training state in
 * the reference -- is one plan and one pass over the state. Everything runs on `stream` with no host synchronisation and no
 * allocation, and every output is one bit pattern, run after run. workspace: fr_densify_workspace_bytes(P) bytes of device
 * memory, 16-byte aligned; a plan stays valid until the next plan on the same workspace. P = 0 launches nothing.
 *
 * Layout of every output tensor (what the reference's cat / [mask] sequence produces):
 *   kept originals in index order | surviving clones in index order | surviving children of copy 0 in index order | ... of
 *   copy N - 1.
 * Child c of the r-th split row (r counted in index order over ALL split rows, surviving or not) reads noise[c * n_split + r]:
 * the reference's repeat(N, 1) order.
 *
 * FR_DENSIFY_AND_PRUNE keeps two quirks of the reference's densify_and_prune (:820-834):
 *   - densification_postfix zeroes max_radii2D before the final cut (:706), so `max_radii2D > max_screen_size` (:829) is false
 *     for every non-negative max_screen_size: that argument only switches the world-size test (:830) on (use_world_size);
 *   - clones carry padded_grad 0 (:734-735) and are small (:807), so they are never split. */
enum {
	FR_DENSIFY_CLONE_MASK = 0, /* keep every row; clone where mask is set (position_grad_densify :836-851, any clone)           */
	FR_DENSIFY_SPLIT_MASK = 1, /* split where mask is set: the parent goes, N children come (:709-729, :757-801)                 */
	FR_DENSIFY_CLONE_GRAD = 2, /* clone = |g| >= max_grad && smax <= t_dense                      (densify_and_clone, :803-818)  */
	FR_DENSIFY_SPLIT_GRAD = 3, /* split = g >= max_grad && smax > t_dense                         (densify_and_split, :731-755)  */
	FR_DENSIFY_AND_PRUNE = 4   /* both, then the opacity / world-size cut                          (densify_and_prune, :820-834)  */
};
enum {
	FR_DENSIFY_COPY = 0,     /* clones and children take the parent's row bitwise                                                */
	FR_DENSIFY_ZERO_NEW = 1, /* kept originals are copied, every clone or child row is zero (exp_avg, exp_avg_sq: :674-675)       */
	FR_DENSIFY_XYZ = 2,      /* as COPY, but child c of split row r = (R[0] s0 + R[1] s1) + R[2] s2 + xyz per component, with
	                            s_k = expf(scaling_k) * noise[c * n_split + r][k] and R = build_rotation(rotation / |rotation|)
	                            (utils/general_utils.py:78-99); fp32, no contraction                        (:740-744)          */
	FR_DENSIFY_SCALING = 3   /* as COPY, but children get logf(expf(scaling_k) / (0.8f * N))                       (:745)         */
};
size_t fr_densify_workspace_bytes(int32_t P);

/* add_densification_stats (:865-867): for the rows with update_filter != 0
 *   accum[i] += sqrtf(gx * gx + gy * gy) (the first two columns of grad [P,3], no contraction), denom[i] += 1.   One launch. */
int fr_densify_stats(int32_t P, const float *grad, const uint8_t *update_filter, float *accum, float *denom, void *stream);

/* The plan (replaces the mask arithmetic of :734-738, :805-807, :821-831 and every .sum() / nonzero of the sequence): one class
 * byte per source row into the workspace (bit 0 the original is kept, 1 its clone survives, 2 it is split, 3 its children
 * survive), each tile's first destination row in each of the four segments, and counts_out (a DEVICE int32[4]) = {kept
 * originals, surviving clones, split rows, surviving children per copy}. With
 *   g = accum / denom (correctly rounded, NaN -> 0; denom NULL: g = accum; rows >= n_grad: g = 0, the reference's padded_grad),
 *   smax = max_k expf(scaling_k), o = 1 / (1 + expf(-opacity)), cs_k = logf(expf(scaling_k) / (0.8f * N)):
 *   clone = |g| >= max_grad && smax <= t_dense           split = g >= max_grad && smax > t_dense
 *   dead  = o < min_opacity || (use_world_size && smax > t_world)                                   (FR_DENSIFY_AND_PRUNE only)
 *   kept = !split && !dead, clone survives = clone && !dead,
 *   children survive = split && !(o < min_opacity || (use_world_size && max_k expf(cs_k) > t_world)) */
typedef struct fr_densify_plan_args {
	int32_t P;
	int32_t mode;           /* FR_DENSIFY_CLONE_MASK .. FR_DENSIFY_AND_PRUNE */
	int32_t N;              /* children per split row, 1 .. 4 */
	int32_t use_world_size; /* FR_DENSIFY_AND_PRUNE: max_screen_size was given */
	int32_t n_grad;         /* the *_GRAD modes: rows of accum (<= P); FR_DENSIFY_AND_PRUNE: P */
	int32_t reserved;
	float max_grad, min_opacity;
	float t_dense;          /* percent_dense * extent */
	float t_world;          /* 0.1 * extent */
	const float *accum;     /* [n_grad] xyz_gradient_accum, or the caller's grads with denom = NULL */
	const float *denom;     /* [n_grad] or NULL */
	const float *scaling;   /* [P,3] raw _scaling (not read by the *_MASK modes) */
	const float *opacity;   /* [P] raw _opacity (FR_DENSIFY_AND_PRUNE only) */
	const uint8_t *mask;    /* [P] the *_MASK modes */
	int32_t *counts_out;    /* DEVICE int32[4] */
	void *workspace;
} fr_densify_plan_args;

typedef struct fr_densify_tensor {
	const void *src;   /* [P, row_words] words, contiguous */
	void *dst;         /* [n_keep + n_clone + N * n_child, row_words] words, contiguous */
	int32_t row_words; /* 4-byte words per row (0: the tensor is skipped); 3 for FR_DENSIFY_XYZ and FR_DENSIFY_SCALING */
	int32_t role;      /* FR_DENSIFY_COPY .. FR_DENSIFY_SCALING */
} fr_densify_tensor;

/* The gather (replaces cat_tensors_to_optimizer :666-686, the child arithmetic :740-749 and the _prune_optimizer gathers that
 * follow): every tensor of the table in ONE launch. n_keep .. n_child are what the plan left in counts_out; a row that would
 * land beyond its segment is never written. */
typedef struct fr_densify_rows_args {
	int32_t P;
	int32_t N;              /* as given to the plan */
	int32_t num_tensors;    /* 0 .. FR_COMPACT_MAX_TENSORS */
	int32_t reserved;
	int32_t n_keep, n_clone, n_split, n_child;
	const float *scaling;   /* [P,3] raw _scaling, [P,4] raw _rotation and [N * n_split, 3] standard normal noise: read for the */
	const float *rotation;  /* children of FR_DENSIFY_XYZ / FR_DENSIFY_SCALING tensors, may be NULL otherwise                    */
	const float *noise;
	void *workspace;        /* as given to fr_densify_plan */
	fr_densify_tensor tensors[FR_COMPACT_MAX_TENSORS];
} fr_densify_rows_args;

int fr_densify_plan(const fr_densify_plan_args *args, void *stream);
int fr_densify_rows(const fr_densify_rows_args *args, void *stream);

/* Bytes fr_forward will request for the geometry / image workspaces (P, W, H dependent) and for the
 * binning workspace given a number of instances; lets a caller pre-size persistent buffers. */
size_t fr_geometry_bytes(int32_t variant, int32_t P);
size_t fr_image_bytes(int32_t variant, int32_t W, int32_t H);
size_t fr_binning_bytes(int32_t variant, int64_t num_instances);
/* fr_geometry_bytes of a call with fr_foveation.levels = `levels` (2 .. 8; 4: the same number; 0 for a bad argument): the rows of
 * the levels 4 .. 7 and the four-wide copies of the level columns lie BEHIND everything fr_geometry_bytes counts, so every
 * fr_geometry_* pointer below is where it is without settings. */
size_t fr_geometry_bytes_fov(int32_t variant, int32_t P, int32_t levels);

/* Introspection for tests: device pointers to internal per-tile / per-instance state inside the workspaces.
 * ranges: uint32 [T,2]. point_list: uint32 [num_rendered], the per-tile depth-sorted lists -- of ITEMS: an item is a
 * position in the library's list of the Gaussians that survive its cull pass, which is in increasing Gaussian index
 * (fr_geometry_vis_list), so vis_list[point_list[i]] is the reference's point_list entry and the order is the
 * reference's. Everything the library keeps per candidate Gaussian (records, level colours, level ranges, walk records)
 * is indexed by item: dense rows instead of rows scattered over all P Gaussians. */
const uint32_t *fr_image_ranges(int32_t variant, int32_t W, int32_t H, const char *image);
const uint32_t *fr_binning_point_list(int32_t variant, int64_t num_instances, const char *binning);
const float *fr_image_final_T(int32_t variant, int32_t W, int32_t H, const char *image);
const uint32_t *fr_image_n_contrib(int32_t variant, int32_t W, int32_t H, const char *image);
/* per-item records float[.][12] = (x, y, conic a, conic b | conic c, opacity, r, g | b, depth, clamp bits, Gaussian index);
 * valid for items whose Gaussian has radii > 0 (RF: the second third holds (conic c, highest level, -, -)) */
const float *fr_geometry_records(int32_t variant, int32_t P, const char *geometry);
/* RF: device pointer to float[5][T] = levels, tile_min, grad_x, grad_y, blending(0/1 as float) */
const float *fr_image_tile_levels(int32_t W, int32_t H, const char *image);
/* the Gaussians that survived the cull pass, in increasing index: uint32 [count], with count = *fr_geometry_vis_count
 * (a device word); "item" i everywhere else means position i of this list */
const uint32_t *fr_geometry_vis_list(int32_t variant, int32_t P, const char *geometry);
const uint32_t *fr_geometry_vis_count(int32_t variant, int32_t P, const char *geometry);
/* walk record of item i: float[16] = (centre x, y, OBB axis 1 x, y | axis 2 x, y, half length 1, 2 |
 * id + flags << 30, depth bits, clipped rectangle x0 + y0 << 16, its width | tiles, highest level, -, -)
 * -- what the reference keeps as eigen_vecs / eigen_lengths (RS forward.cu:244-265) */
const float *fr_geometry_walk_records(int32_t variant, int32_t P, const char *geometry);
/* RF: per-item per-level (r, g, b, opacity) float[.][4][4] (compute_fov_colors, RF rasterizer_impl.cu:490-530; only
 * the levels of the Gaussian's level range are written) and the packed level ranges uint32 [.] = lo | hi << 8 */
const float *fr_geometry_level_colours(int32_t P, const char *geometry);
const uint32_t *fr_geometry_level_ranges(int32_t P, const char *geometry);
/* RF with fr_foveation.levels > 4: the rows of the levels 4 .. 7, float[.][4][4] like fr_geometry_level_colours (which keeps the
 * levels 0 .. 3); NULL for levels <= 4 */
const float *fr_geometry_level_colours_hi(int32_t P, int32_t levels, const char *geometry);

/* LPIPS, VGG16, version 0.1 (csrc/lpips.hip; replaces fov3dgs/lpipsPyTorch/__init__.py:6-21, modules/lpips.py:30-36,
 * modules/networks.py:41-64 and :89-96, modules/utils.py:6-8 -- a torchvision VGG16 and two weight downloads per picture pair).
 * The library holds no weights: the caller hands in the 13 convolutions of vgg16().features and the five `lin` vectors.
 *   fr_lpips_packed_bytes     the size of the packed weights.
 *   fr_lpips_pack_weights     a HOST routine, once per set of weights: conv_weights[13] ([Cout,Cin,3,3] each, the convolutions of
 *                             vgg16().features in order: 3-64, 64-64, 64-128, 128-128, 128-256, 256-256 x2, 256-512, 512-512 x5),
 *                             conv_biases[13] ([Cout]) and lin_weights[5] ([C], C = 64, 128, 256, 512, 512), all host float32, into
 *                             `packed` (host, fr_lpips_packed_bytes). The caller copies `packed` to the device. A NULL pointer is
 *                             FR_ERR_INVALID, the message names it.
 *   fr_lpips_workspace_bytes  the workspace of one call over N picture pairs of H x W: two ping-pong activation buffers of
 *                             2 N x 64 x H x W floats (relu1_1 and relu1_2 of both pictures, the largest maps) and the head's
 *                             partial sums; -1 for sizes fr_lpips_forward refuses (fr_last_error says which).
 *   fr_lpips_forward          size = sizeof(fr_lpips_args). x, y: [N,3,H,W] fp32 device planes, scaled as the caller has them
 *                             ((x - mean) / std is applied on load; [0, 1] pictures are NOT rescaled to [-1, 1], as in the
 *                             reference). packed: the packed weights on the device, 16-byte aligned. workspace: 256-byte aligned.
 *                             out[1] (device) = sum over the five taps AND over the batch of mean_HW( sum_c w_c (n(fx)_c -
 *                             n(fy)_c)^2 ), n(a) = a / (sqrt(sum_c a_c^2) + 1e-10): torch.sum(torch.cat(res, 0), 0, True) of the
 *                             reference. out_taps (optional, device [5]): the five addends, each summed over the batch.
 *                             out_features[k] (optional, device [N,C_k,H_k,W_k], NCHW): x's tap maps before the normalisation
 *                             (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3; H_k = H >> k), for tests and diagnosis.
 *                             Exact f32 on the matrix cores, one k-ordered chain per output, sums in double in a fixed order, no
 *                             float atomics: every output is one bit pattern, run after run; equal pictures give exactly 0.
 *                             stage_events (optional [19], fr_event_create handles, NULL entries skipped): recorded on `stream` in
 *                             front of the first layer ([0]) and behind each of the 18 stages in their order -- the 13
 *                             convolutions, the head of a tap directly behind the tap's convolution.
 *                             Everything runs on `stream`; nothing is allocated and nothing synchronises (debug != 0 does, after
 *                             every stage). FR_ERR_INVALID before anything is enqueued, the message names the field: size too
 *                             small, N outside 1 .. 512, H or W outside 16 .. 16384 (below 16 the fourth pool has no output: the
 *                             reference raises there too), x / y / packed / workspace / out NULL, a misaligned buffer. */
typedef struct fr_lpips_args {
	uint32_t size;
	int32_t N, H, W;
	int32_t debug;
	const float *x;
	const float *y;
	const void *packed;
	void *workspace;
	float *out;
	float *out_taps;
	float *out_features[5];
	void *stream;
	void **stage_events;
} fr_lpips_args;
size_t fr_lpips_packed_bytes(void);
int fr_lpips_pack_weights(const float *const *conv_weights, const float *const *conv_biases, const float *const *lin_weights, void *packed);
int64_t fr_lpips_workspace_bytes(int32_t N, int32_t H, int32_t W);
int fr_lpips_forward(const fr_lpips_args *args);

/* LPIPS as a training loss: the forward that keeps what the backward needs, and the backward pass (csrc/lpips.hip; replaces
 * lpipsPyTorch/modules/lpips.py, modules/networks.py and modules/utils.py run under torch.autograd -- lpips(render, gt).backward()).
 * The gradient is that of fr_lpips_forward's value with respect to x, times an upstream scalar read on the device.
 *   fr_lpips_backward_packed_bytes    the size of the backward weights, a blob of their own beside the packed weights.
 *   fr_lpips_pack_backward_weights    a HOST routine, once per set of weights: conv_weights[13] as for fr_lpips_pack_weights into
 *                                     `packed_backward` (host). Per layer 1 .. 12 the slabs of W'[ci,co,ky,kx] = W[co,ci,2-ky,2-kx]
 *                                     (Cin' = Cout, Cout' = Cin) in the layout of the forward's slabs, [Cout'/64][Cin'/8] slabs of
 *                                     [tap][group of 4][64][4]; in front of them the first layer's [chunk of 8][tap][8][3]. No bias.
 *   fr_lpips_keep_workspace_bytes     the kept state of one differentiable forward over N pairs of H x W: x's 13 post-ReLU maps and
 *                                     the five tap gradients (the gradient of the value with respect to x's tap maps, computed by
 *                                     the forward's head pass, where both pictures' taps are in hand: y's maps are not kept).
 *                                     3.25 GB for one 1080 x 1920 pair. -1 for sizes fr_lpips_forward refuses (fr_last_error).
 *   fr_lpips_keep_activation_offset   the byte offset of layer 0 .. 12's map in the kept state, [N][C/8][H_l][W_l][8] floats
 *                                     (channel c of a pixel at [c / 8] ... [c % 8]); -1 for a bad size or layer.
 *   fr_lpips_forward_keep             fr_lpips_forward with x's maps written to `keep` (256-byte aligned, caller-owned, one per
 *                                     call that is to be differentiated) instead of ping-ponging; `workspace` is that of
 *                                     fr_lpips_workspace_bytes and holds nothing once the call has run. out[1] has the bits
 *                                     fr_lpips_forward gives: the same kernels. stage_events: as fr_lpips_forward, [19].
 *   fr_lpips_backward                 grad_x[N,3,H,W] (device, written whole) = grad_out[0] * d value / d x from `keep`.
 *                                     grad_out: one device float, never read by the host. workspace: fr_lpips_workspace_bytes,
 *                                     scratch. Rules: a ReLU passes the gradient where the kept output is > 0; a 2 x 2 pool sends
 *                                     it to the window's first maximum in row-major order (torch's rules); at a pixel whose tap
 *                                     vector is all zero the gradient is finite (the normalisation's second term is taken as 0,
 *                                     its limit) where the reference's sqrt backward gives NaN. Exact f32 on the matrix cores, no
 *                                     atomics: one bit pattern per element, run after run; equal pictures give exactly 0
 *                                     everywhere. stage_events (optional [14]): in front of the pass and behind each of the 13
 *                                     stages, the convolutions of the layers 12 .. 1 and the first layer's.
 * Both calls run on `stream`, allocate nothing and never synchronise (debug != 0 does). FR_ERR_INVALID before anything is
 * enqueued, the message names the field: size too small, N / H / W out of range as for fr_lpips_forward, a NULL pointer, a
 * misaligned buffer. */
typedef struct fr_lpips_keep_args {
	uint32_t size;
	int32_t N, H, W;
	int32_t debug;
	const float *x;
	const float *y;
	const void *packed;
	void *workspace;
	void *keep;
	float *out;
	float *out_taps;
	void *stream;
	void **stage_events;
} fr_lpips_keep_args;
typedef struct fr_lpips_backward_args {
	uint32_t size;
	int32_t N, H, W;
	int32_t debug;
	const void *packed_backward;
	const void *keep;
	void *workspace;
	const float *grad_out;
	float *grad_x;
	void *stream;
	void **stage_events;
} fr_lpips_backward_args;
size_t fr_lpips_backward_packed_bytes(void);
int fr_lpips_pack_backward_weights(const float *const *conv_weights, void *packed_backward);
int64_t fr_lpips_keep_workspace_bytes(int32_t N, int32_t H, int32_t W);
int64_t fr_lpips_keep_activation_offset(int32_t N, int32_t H, int32_t W, int32_t layer);
int fr_lpips_forward_keep(const fr_lpips_keep_args *args);
int fr_lpips_backward(const fr_lpips_backward_args *args);

#ifdef __cplusplus
}
#endif
#endif /* FOVRASTER_H */
