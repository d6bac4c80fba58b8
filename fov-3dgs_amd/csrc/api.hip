// extern "C" entry points of libfovraster_hip.so (see include/fovraster.h for the contract and
// for the reference interfaces each one replaces).
#include "common.h"
#include <atomic>
#include <mutex>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <new>

namespace fr {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
}

int check_launch(const char *what, hipStream_t stream, bool debug)
{
	hipError_t e = hipGetLastError();
	static const bool trace = getenv("FR_TRACE") != nullptr;
	if (trace) { fprintf(stderr, "[fovraster] launched %s\n", what); fflush(stderr); }
	if (e == hipSuccess && debug) e = hipStreamSynchronize(stream);
	if (trace && debug) { fprintf(stderr, "[fovraster] %s done (%d)\n", what, (int)e); fflush(stderr); }
	if (e != hipSuccess)
	{
		set_error("%s: %s", what, hipGetErrorString(e));
		return FR_ERR_HIP;
	}
	return FR_OK;
}

#define FR_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { set_error("%s: %s", #call, hipGetErrorString(e_)); return FR_ERR_HIP; } } while (0)

static int validate_forward(const fr_forward_args *a)
{
	if (!a) { set_error("null args"); return FR_ERR_INVALID; }
	if (a->variant < FR_VARIANT_ORIGINAL || a->variant > FR_VARIANT_MMFR_PCHECK_OBB) { set_error("unknown variant %d", a->variant); return FR_ERR_INVALID; }
	if (a->P < 0 || a->W <= 0 || a->H <= 0) { set_error("bad sizes P=%d W=%d H=%d", a->P, a->W, a->H); return FR_ERR_INVALID; }
	if (a->P > (1 << 30) || a->W > 16 * 65535 || a->H > 16 * 65535) { set_error("too large: P=%d (max 2^30) W=%d H=%d (max 65535 tiles per axis)", a->P, a->W, a->H); return FR_ERR_INVALID; }
	if ((int64_t)((a->W + FR_TILE - 1) / FR_TILE) * ((a->H + FR_TILE - 1) / FR_TILE) >= (1 << 29)) { set_error("too many tiles (W=%d H=%d)", a->W, a->H); return FR_ERR_INVALID; }
	if (!a->out_color) { set_error("out_color is null"); return FR_ERR_INVALID; }
	// ORIGINAL with both statistics pointers is the counting render; one of them alone is a caller's mistake, not a request
	if (a->variant == FR_VARIANT_ORIGINAL && (a->gaussians_count != nullptr) != (a->contributions != nullptr))
	{ set_error("variant original: gaussians_count and contributions go together (both = the counting render, neither = the plain one); only %s is set",
		a->gaussians_count ? "gaussians_count" : "contributions"); return FR_ERR_INVALID; }
	if (a->P == 0) return FR_OK;
	if (!a->means3D || !a->opacities || !a->viewmatrix || !a->projmatrix || !a->campos || !a->background || !a->radii)
	{ set_error("a required pointer is null"); return FR_ERR_INVALID; }
	if (!a->geometry_resize || !a->binning_resize || !a->image_resize) { set_error("resize callbacks are required"); return FR_ERR_INVALID; }
	const bool fov = a->variant == FR_VARIANT_FOV_PCHECK_OBB;
	if (fov)
	{
		if (a->shs_rest) { set_error("shs_rest is not used by the foveated variant (its shs already is the rest part)"); return FR_ERR_INVALID; }
		if (!a->shs || !a->shs_dcs || !a->highest_levels) { set_error("foveated variant needs shs (rest), shs_dcs and highest_levels"); return FR_ERR_INVALID; }
		if (a->M != 15) { set_error("foveated variant expects M=15 rest coefficients, got %d", a->M); return FR_ERR_INVALID; }
	}
	else if (a->variant == FR_VARIANT_NAIVE_FOV_PCHECK_OBB || a->variant == FR_VARIANT_MMFR_PCHECK_OBB)
	{
		if (!a->shs || a->colors_precomp || a->shs_rest || !a->highest_levels) { set_error("the shared-model foveated variant needs shs [P,M,3] and highest_levels (no colors_precomp / shs_rest)"); return FR_ERR_INVALID; }
		if (a->M < (a->D + 1) * (a->D + 1)) { set_error("M=%d too small for SH degree %d", a->M, a->D); return FR_ERR_INVALID; }
		if (a->packed_geom || a->packed_colour || a->packed_cull) { set_error("the shared-model foveated variant has no packed layout"); return FR_ERR_INVALID; }
	}
	else
	{
		if ((a->shs == nullptr) == (a->colors_precomp == nullptr)) { set_error("provide exactly one of shs / colors_precomp"); return FR_ERR_INVALID; }
		if (a->shs && a->M < (a->D + 1) * (a->D + 1)) { set_error("M=%d too small for SH degree %d", a->M, a->D); return FR_ERR_INVALID; }
		if (a->shs_rest && (!a->shs || a->M < 2)) { set_error("shs_rest needs shs (the DC part) and M >= 2"); return FR_ERR_INVALID; }
	}
	if (a->D < 0 || a->D > 3) { set_error("SH degree %d not in 0..3", a->D); return FR_ERR_INVALID; }
	const bool has_sr = a->scales && a->rotations;
	if (has_sr == (a->cov3D_precomp != nullptr)) { set_error("provide exactly one of scales+rotations / cov3D_precomp"); return FR_ERR_INVALID; }
	if ((a->packed_geom != nullptr) != (a->packed_colour != nullptr) || (a->packed_geom != nullptr) != (a->packed_cull != nullptr))
	{ set_error("packed_geom, packed_colour and packed_cull go together"); return FR_ERR_INVALID; }
	if (a->packed_geom && (!has_sr || !a->shs || a->colors_precomp || a->M != (fov ? 15 : 16)))
	{ set_error("the packed model needs scales + rotations and shs with all 16 coefficients (M=%d)", a->M); return FR_ERR_INVALID; }
	if (a->raw_activations && (is_fov(a->variant) || !has_sr || a->packed_geom))
	{ set_error("raw_activations: plain variants with scales + rotations, without the packed layout"); return FR_ERR_INVALID; }
	if (a->no_stats && a->variant != FR_VARIANT_PCHECK_OBB_SUM) { set_error("no_stats: pcheck_obb_sum only"); return FR_ERR_INVALID; }
	if (has_stats(a->variant) && !a->no_stats && (!a->gaussians_count || !a->contributions)) { set_error("this variant needs gaussians_count and contributions"); return FR_ERR_INVALID; }
	if (a->variant == FR_VARIANT_PCHECK_OBB_LWMC && !a->loss_map) { set_error("pcheck_obb_loss_weighted_max_count needs loss_map"); return FR_ERR_INVALID; }
	return FR_OK;
}

// fr_foveation -> what the kernels take. The level step and the cap are formed HERE, once, in the reference's order of operations
// (RF rasterizer_impl.cu:99-177 with the constants of auxiliary.h:26-32 replaced), so that every kernel and a CPU derivation
// that does the same arithmetic use the same floats. f == NULL: the reference's constants.
static FovParams fov_params(const fr_foveation *f)
{
	FovParams p;
	p.levels = f ? f->levels : FR_FOV_LEVELS;
	const float sqrt_max_ps = (float)sqrt((double)(f ? f->max_pooling_size : 12.0f)); // 12: the reference's literal 3.4641016151377544f
	p.riw = f ? f->real_image_width : 2.0f;
	p.rvd = f ? f->real_viewing_distance : 1.0f;
	p.step = (float)(((double)sqrt_max_ps - 1.) / (double)(float)(p.levels - 1));
	p.cap = (float)((double)(float)p.levels - 0.1);
	p.start_blend = f ? f->start_blend : 0.5f;
	p.blend_width = f ? f->blend_width : 0.5f;
	p.box_top = (float)(p.levels > FR_FOV_LEVELS ? p.levels : FR_FOV_LEVELS);
	return p;
}

// refuses a bad fr_foveation before anything is enqueued; the message names the field
static int validate_foveation(const fr_forward_args *a, const fr_foveation *f)
{
	if (!f) return FR_OK;
	if (f->size < sizeof(fr_foveation)) { set_error("fr_foveation.size is %u, expected at least %u", f->size, (unsigned)sizeof(fr_foveation)); return FR_ERR_INVALID; }
	if (a->variant != FR_VARIANT_FOV_PCHECK_OBB)
	{ set_error("fr_foveation: settings are for variant %d (fov_pcheck_obb) only, not variant %d (the SMFR / MMFR baselines keep the reference's constants)", FR_VARIANT_FOV_PCHECK_OBB, a->variant); return FR_ERR_INVALID; }
	if (f->levels < 2 || f->levels > FR_FOV_MAX_LEVELS) { set_error("fr_foveation.levels is %d, not in 2..%d", f->levels, FR_FOV_MAX_LEVELS); return FR_ERR_INVALID; }
	if (!std::isfinite(f->max_pooling_size) || !(f->max_pooling_size > 1.0f)) { set_error("fr_foveation.max_pooling_size is %g, must be finite and > 1", (double)f->max_pooling_size); return FR_ERR_INVALID; }
	if (!std::isfinite(f->real_image_width) || !(f->real_image_width > 0.0f)) { set_error("fr_foveation.real_image_width is %g, must be finite and > 0", (double)f->real_image_width); return FR_ERR_INVALID; }
	if (!std::isfinite(f->real_viewing_distance) || !(f->real_viewing_distance > 0.0f)) { set_error("fr_foveation.real_viewing_distance is %g, must be finite and > 0", (double)f->real_viewing_distance); return FR_ERR_INVALID; }
	if (!std::isfinite(f->start_blend) || !(f->start_blend > 0.0f && f->start_blend < 1.0f)) { set_error("fr_foveation.start_blend is %g, must lie in (0, 1)", (double)f->start_blend); return FR_ERR_INVALID; }
	if (!std::isfinite(f->blend_width) || !(f->blend_width > 0.0f)) { set_error("fr_foveation.blend_width is %g, must be finite and > 0", (double)f->blend_width); return FR_ERR_INVALID; }
	if (f->levels > FR_FOV_LEVELS && (a->packed_geom || a->packed_colour || a->packed_cull))
	{ set_error("fr_foveation.levels is %d: the packed model layout holds at most %d levels", f->levels, FR_FOV_LEVELS); return FR_ERR_INVALID; }
	return FR_OK;
}

} // namespace fr

using namespace fr;

extern "C" {

int fr_abi_version(void) { return FR_ABI_VERSION; }

void *fr_event_create(void)
{
	hipEvent_t e;
	if (hipEventCreate(&e) != hipSuccess) { set_error("hipEventCreate failed"); return nullptr; }
	return (void *)e;
}
void fr_event_destroy(void *event) { if (event) (void)hipEventDestroy((hipEvent_t)event); }
int fr_event_elapsed_ms(void *start, void *stop, float *ms)
{
	if (!start || !stop || !ms) { set_error("null event"); return FR_ERR_INVALID; }
	// (an event that was never recorded is the caller's mistake, not a device fault: the error is reported here and not left
	// behind as the runtime's sticky "last error" for whoever calls into HIP next)
	hipError_t e = hipEventSynchronize((hipEvent_t)stop);
	if (e == hipSuccess) e = hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
	if (e != hipSuccess) { (void)hipGetLastError(); set_error("event timing: %s (was the event recorded?)", hipGetErrorString(e)); return FR_ERR_HIP; }
	return FR_OK;
}
const char *fr_last_error(void) { return g_err; }

size_t fr_geometry_bytes(int32_t variant, int32_t P) { return carve_geom(variant, (size_t)P, nullptr).bytes; }
size_t fr_geometry_bytes_fov(int32_t variant, int32_t P, int32_t levels)
{
	if (P < 0 || levels < 2 || levels > FR_FOV_MAX_LEVELS) { set_error("bad geometry_bytes_fov arguments"); return 0; }
	return carve_geom(variant, (size_t)P, nullptr, levels).bytes;
}
size_t fr_image_bytes(int32_t variant, int32_t W, int32_t H) { return carve_image(variant, W, H, nullptr).bytes; }
size_t fr_binning_bytes(int32_t variant, int64_t n) { (void)variant; return carve_bin(n, nullptr).bytes; }

const uint32_t *fr_image_ranges(int32_t variant, int32_t W, int32_t H, const char *image) { return (const uint32_t *)carve_image(variant, W, H, (char *)image).ranges; }
const uint32_t *fr_binning_point_list(int32_t variant, int64_t n, const char *binning) { (void)variant; return carve_bin(n, (char *)binning).point_list; }
const float *fr_image_final_T(int32_t variant, int32_t W, int32_t H, const char *image) { return carve_image(variant, W, H, (char *)image).final_T; }
const uint32_t *fr_image_n_contrib(int32_t variant, int32_t W, int32_t H, const char *image) { return carve_image(variant, W, H, (char *)image).n_contrib; }
const float *fr_geometry_records(int32_t variant, int32_t P, const char *geometry) { return (const float *)carve_geom(variant, (size_t)P, (char *)geometry).rec; }
const uint32_t *fr_geometry_vis_list(int32_t variant, int32_t P, const char *geometry) { return carve_geom(variant, (size_t)P, (char *)geometry).vis_list; }
const uint32_t *fr_geometry_vis_count(int32_t variant, int32_t P, const char *geometry) { return carve_geom(variant, (size_t)P, (char *)geometry).slab_ctr + 1; }
const float *fr_geometry_walk_records(int32_t variant, int32_t P, const char *geometry) { return (const float *)carve_geom(variant, (size_t)P, (char *)geometry).wrec; }
const float *fr_geometry_level_colours(int32_t P, const char *geometry) { return (const float *)carve_geom(FR_VARIANT_FOV_PCHECK_OBB, (size_t)P, (char *)geometry).lvl; }
const float *fr_geometry_level_colours_hi(int32_t P, int32_t levels, const char *geometry) { return (const float *)carve_geom(FR_VARIANT_FOV_PCHECK_OBB, (size_t)P, (char *)geometry, levels).lvl_hi; }
const uint32_t *fr_geometry_level_ranges(int32_t P, const char *geometry) { return carve_geom(FR_VARIANT_FOV_PCHECK_OBB, (size_t)P, (char *)geometry).lrange; }
const float *fr_image_tile_levels(int32_t W, int32_t H, const char *image) { return carve_image(FR_VARIANT_FOV_PCHECK_OBB, W, H, (char *)image).tile_lv; }

// ---- the forward call ---------------------------------------------------------------------------
// A frame is enqueued in two halves around its ONE host synchronisation (the instance count, which sizes the binning
// workspace -- the reference synchronises twice for it, rasterizer_impl.cu:281 and RS :401,422):
//   fr_forward_begin    workspaces (geometry, image), fills, tile levels, cull pass, projection, tile counts, tile scan
//   fr_forward_finish   waits for the count, binning workspace, emission, per-tile sort, colours, blend
// fr_forward is begin + finish. A host that keeps TWO frames in flight (two streams, two workspace sets) calls
// begin(n + 1) before finish(n): the latency-bound head of one frame then runs beside the sort and the blend of the other.
} // extern "C"

namespace fr {

// 64 bytes of pinned, device-mapped host memory per frame in flight: the tile scan writes the frame's totals and its sequence
// number there, the host polls (a copy command after the kernel costs ~10 us more of an idle GPU). One pool per PROCESS behind a
// mutex (a frame handle may be dropped by another thread than the one that made it -- a garbage collector's finalizer -- or after
// its thread has gone); the device address of mapped host memory belongs to the device that was current when it was asked for.
struct PinnedBlock
{
	uint32_t *host = nullptr, *dev = nullptr; int device = -1; bool busy = false;
	hipEvent_t quarantine = nullptr; bool quarantined = false; // a DROPPED frame's tile scan may still be on its way to the block
};
static std::mutex g_pinned_mu;
static PinnedBlock g_pinned_pool[64];
static PinnedBlock *take_pinned(int device)
{
	std::lock_guard<std::mutex> lock(g_pinned_mu);
	PinnedBlock *spare = nullptr;
	for (PinnedBlock &b : g_pinned_pool)
	{
		if (b.busy) continue;
		if (b.quarantined)
		{
			if (hipEventQuery(b.quarantine) != hipSuccess) { (void)hipGetLastError(); continue; }
			b.quarantined = false;
		}
		// (an idle block still holds its last frame's sequence word; no write to it is in flight: not busy, not quarantined)
		if (b.host && b.device == device) { __atomic_store_n(&b.host[4], 0u, __ATOMIC_RELEASE); b.busy = true; return &b; }
		if (!spare) spare = &b;
	}
	if (!spare) return nullptr; // every block of the pool in flight: the frame falls back to a copy + stream wait
	if (spare->host) (void)hipHostFree(spare->host);
	spare->host = spare->dev = nullptr; spare->device = device;
	void *h = nullptr, *d = nullptr;
	if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocPortable) == hipSuccess && hipHostGetDevicePointer(&d, h, 0) == hipSuccess)
	{ spare->host = (uint32_t *)h; spare->dev = (uint32_t *)d; for (int i = 0; i < 16; i++) spare->host[i] = 0; }
	else if (h) (void)hipHostFree(h);
	(void)hipGetLastError();
	if (!spare->host) return nullptr;
	spare->busy = true;
	return spare;
}
// A frame gives its block back. unread: its tile scan was enqueued and the host never read the totals (an error return between the
// scan and the count, fr_forward_abandon, a handle dropped by a finalizer): the write may still be on its way, so the block is not
// handed to another frame before an event on the frame's stream has passed.
static void release_pinned(PinnedBlock *b, bool unread, hipStream_t stream)
{
	if (!b) return;
	bool drained = !unread;
	if (unread)
	{
		std::lock_guard<std::mutex> lock(g_pinned_mu);
		if (!b->quarantine && hipEventCreateWithFlags(&b->quarantine, hipEventDisableTiming) != hipSuccess) b->quarantine = nullptr;
		if (b->quarantine && hipEventRecord(b->quarantine, stream) == hipSuccess) { b->quarantined = true; b->busy = false; return; }
		(void)hipGetLastError();
	}
	if (!drained) (void)hipStreamSynchronize(stream); // (no event to be had: wait the write out)
	std::lock_guard<std::mutex> lock(g_pinned_mu);
	b->busy = false;
}

// what the next frame of a kind (variant, P, W, H) asks its binning workspace for before its count is in
struct Guess { int32_t variant = -1, P = 0, W = 0, H = 0; int64_t capacity = 0; };
static Guess &guess_for(int variant) { static thread_local Guess guesses[8]; return guesses[variant & 7]; }

} // namespace fr

struct fr_frame
{
	fr_forward_args *a = nullptr;
	FwdCtx c;
	AuxStream *ax = nullptr;       // the frame's helper streams (null: everything on the launch stream)
	bool aux_pending = false;      // work on ax->s2 that the launch stream has not waited for yet
	PinnedBlock *pin = nullptr;
	bool scan_enqueued = false;    // the kernel that writes the pinned totals block is on the stream ...
	bool totals_read = false;      // ... and the host has read what it wrote
	bool empty = false;            // P == 0: nothing left to do
	fr_fov_state *keep_state = nullptr; // the state-keeping foveated forward: filled by fr_forward_finish
	// every exit that abandons the frame joins the helper stream first: the caller may free or reuse out_color / the
	// statistics arrays / the workspaces as soon as the call has returned
	void join_aux() { if (aux_pending && ax) (void)hipStreamWaitEvent(c.stream, ax->join2, 0); aux_pending = false; }
	~fr_frame() { join_aux(); release_pinned(pin, scan_enqueued && !totals_read, c.stream); }
};

namespace fr {

// what the state-keeping foveated forward refuses, before anything is enqueued (the message names the field)
static int validate_fov_keep(const fr_forward_args *a, const fr_foveation *fov, const fr_fov_state *state)
{
	if (!state) { set_error("fr_fov_state: state is null"); return FR_ERR_INVALID; }
	if (state->size < sizeof(fr_fov_state)) { set_error("fr_fov_state.size is %u, expected at least %u", state->size, (unsigned)sizeof(fr_fov_state)); return FR_ERR_INVALID; }
	if (a->variant != FR_VARIANT_FOV_PCHECK_OBB)
	{ set_error("fr_forward_args.variant is %d: the state-keeping forward is for variant %d (fov_pcheck_obb) only", a->variant, FR_VARIANT_FOV_PCHECK_OBB); return FR_ERR_INVALID; }
	if (fov && fov->levels > FR_FOV_LEVELS)
	{ set_error("fr_foveation.levels is %d: the appearance backward pass keeps one row of sums per Gaussian, i.e. at most %d levels", fov->levels, FR_FOV_LEVELS); return FR_ERR_INVALID; }
	if (a->packed_geom || a->packed_colour || a->packed_cull)
	{ set_error("packed_geom / packed_colour / packed_cull: the state-keeping forward renders from the ordinary tensors (a packed model is inference-only)"); return FR_ERR_INVALID; }
	return FR_OK;
}

// The kept state a foveated backward pass is handed (`who`: the entry point, for the messages). full: fr_backward_fov, which wants the
// state of a _full forward and has nothing to do without Gaussians; fr_backward_fov_appearance wants a plain keep state and answers
// FR_OK for P == 0 (the caller's: the workspaces of such a state are not looked at). Each pass refuses the other's state.
static int validate_fov_state(const fr_fov_state *st, const char *who, bool full)
{
	if (!st) { set_error("%s: state is null", who); return FR_ERR_INVALID; }
	if (st->size < sizeof(fr_fov_state)) { set_error("fr_fov_state.size is %u, expected at least %u", st->size, (unsigned)sizeof(fr_fov_state)); return FR_ERR_INVALID; }
	if ((st->variant & ~FR_FOV_STATE_FULL) != FR_VARIANT_FOV_PCHECK_OBB)
	{ set_error("%s: state.variant is %d, not %d (fov_pcheck_obb): not the state of a state-keeping foveated forward", who, st->variant & ~FR_FOV_STATE_FULL, FR_VARIANT_FOV_PCHECK_OBB); return FR_ERR_INVALID; }
	if (full && !(st->variant & FR_FOV_STATE_FULL))
	{ set_error("%s: state.variant lacks FR_FOV_STATE_FULL: the state was not made by fr_forward_begin_fov_keep_full (its geometry workspace has no rows of moments)", who); return FR_ERR_INVALID; }
	if (!full && (st->variant & FR_FOV_STATE_FULL))
	{ set_error("%s: state.variant carries FR_FOV_STATE_FULL: the state was made by fr_forward_begin_fov_keep_full, whose rows of moments this pass would leave uncleared", who); return FR_ERR_INVALID; }
	if (st->levels < 2 || st->levels > FR_FOV_LEVELS)
	{ set_error("%s: state.levels is %d, not in 2..%d (levels 5 .. 8 would need a second row of sums)", who, st->levels, FR_FOV_LEVELS); return FR_ERR_INVALID; }
	if (st->P < 0 || (full && st->P == 0) || st->W <= 0 || st->H <= 0 || st->num_rendered < 0 || st->num_items < 0
		|| (int64_t)st->num_items > 4 * (int64_t)((st->W + FR_TILE - 1) / FR_TILE) * ((st->H + FR_TILE - 1) / FR_TILE))
	{ set_error("%s: state holds bad sizes (P=%d W=%d H=%d num_rendered=%d num_items=%d)", who, st->P, st->W, st->H, st->num_rendered, st->num_items); return FR_ERR_INVALID; }
	if (st->P > 0 && (!st->geometry || !st->image || (st->num_rendered > 0 && !st->binning))) { set_error("%s: state.geometry / image / binning is null", who); return FR_ERR_INVALID; }
	return FR_OK;
}

// what a call with fr_forward_aux refuses, before anything is enqueued (the message names the cause); a struct with neither pointer
// asks for nothing
static int validate_aux(const fr_forward_args *a, const fr_forward_aux *aux, int keep)
{
	if (!aux) return FR_OK;
	if (aux->size < sizeof(fr_forward_aux)) { set_error("fr_forward_aux.size is %u, expected at least %u", aux->size, (unsigned)sizeof(fr_forward_aux)); return FR_ERR_INVALID; }
	if ((aux->depth != nullptr) != (aux->coverage != nullptr))
	{ set_error("fr_forward_aux: depth and coverage go together (both planes or neither); only %s is set", aux->depth ? "depth" : "coverage"); return FR_ERR_INVALID; }
	if (!aux->depth) return FR_OK;
	if (a->variant != FR_VARIANT_FOV_PCHECK_OBB && a->variant != FR_VARIANT_PCHECK_OBB)
	{ set_error("fr_forward_aux: depth / coverage are outputs of variant %d (fov_pcheck_obb) and variant %d (pcheck_obb) only, not of variant %d",
		FR_VARIANT_FOV_PCHECK_OBB, FR_VARIANT_PCHECK_OBB, a->variant); return FR_ERR_INVALID; }
	if (keep) { set_error("fr_forward_aux: depth / coverage are outputs of the inference frame, not of the state-keeping forwards (_keep, _keep_full)"); return FR_ERR_INVALID; }
	return FR_OK;
}

// keep: 0 = the inference frame, 1 = the state-keeping forward, 2 = the same for the full backward pass (fr_forward_begin_fov_keep_full)
static int forward_begin(fr_forward_args *a, const fr_forward_ext *ext, const fr_foveation *fov, fr_fov_state *keep_state, int keep, fr_frame **out,
	const fr_forward_aux *aux = nullptr)
{
	if (!out) { set_error("null frame handle"); return FR_ERR_INVALID; }
	*out = nullptr;
	int rc = validate_forward(a);
	if (rc) return rc;
	rc = validate_aux(a, aux, keep);
	if (rc) return rc;
	if (keep) { rc = validate_fov_keep(a, fov, keep_state); if (rc) return rc; }
	if (ext && ext->size < sizeof(fr_forward_ext)) { set_error("fr_forward_ext.size is %u, expected at least %u", ext->size, (unsigned)sizeof(fr_forward_ext)); return FR_ERR_INVALID; }
	rc = validate_foveation(a, fov);
	if (rc) return rc;
	hipStream_t stream = (hipStream_t)a->stream;
	a->num_rendered = 0;
	a->max_tile_instances = 0;
	a->num_candidates = 0;
	fr_frame *f = new (std::nothrow) fr_frame;
	if (!f) { set_error("out of host memory"); return FR_ERR_ALLOC; }
	struct Guard { fr_frame *f; ~Guard() { delete f; } } guard = { f }; // (released at the end: an early return drops the frame)
	f->a = a;
	FwdCtx &c = f->c;
	c.a = a; c.stream = stream;
	c.visibility = ext ? ext->visibility : nullptr; // (read here: ext need not outlive this call)
	c.fov = fov_params(fov);                        // (likewise: the settings travel in the kernels' arguments)
	c.keep = keep ? 1 : 0;
	if (aux) { c.aux_depth = aux->depth; c.aux_cov = aux->coverage; } // (likewise read here)
	f->keep_state = keep ? keep_state : nullptr;
	if (keep)
	{
		const uint32_t sz = keep_state->size;
		memset(keep_state, 0, sizeof(fr_fov_state));
		keep_state->size = sz; keep_state->variant = a->variant | (keep == 2 ? FR_FOV_STATE_FULL : 0); keep_state->P = a->P; keep_state->W = a->W; keep_state->H = a->H;
		keep_state->levels = c.fov.levels; keep_state->start_blend = c.fov.start_blend; keep_state->blend_width = c.fov.blend_width;
	}
	if (a->P == 0)
	{
		// reference: RasterizeGaussiansCUDA returns the zero-initialised image when P == 0
		FR_HIP(hipMemsetAsync(a->out_color, 0, sizeof(float) * 3 * (size_t)a->W * a->H, stream));
		if (c.aux_depth)
		{
			FR_HIP(hipMemsetAsync(c.aux_depth, 0, sizeof(float) * (size_t)a->W * a->H, stream));
			FR_HIP(hipMemsetAsync(c.aux_cov, 0, sizeof(float) * (size_t)a->W * a->H, stream));
		}
		f->empty = true;
		*out = f; guard.f = nullptr;
		return FR_OK;
	}
	// optional per-stage timing: record the caller's events on the launch stream (no sync here)
	auto mark = [&](int i) { if (a->stage_events && a->stage_events[i]) (void)hipEventRecord((hipEvent_t)a->stage_events[i], stream); };
	c.gx = (a->W + FR_TILE - 1) / FR_TILE; c.gy = (a->H + FR_TILE - 1) / FR_TILE; c.T = c.gx * c.gy;
	c.focal_y = a->H / (2.0f * a->tanfovy);
	c.focal_x = a->W / (2.0f * a->tanfovx);

	char *gptr = a->geometry_resize(a->resize_user[0], keep == 2 ? carve_fov_full_geom((size_t)a->P, nullptr, c.fov.levels).bytes
		: keep ? carve_fov_keep_geom((size_t)a->P, nullptr, c.fov.levels).bytes : carve_geom(a->variant, (size_t)a->P, nullptr, c.fov.levels).bytes);
	char *iptr = a->image_resize(a->resize_user[2], keep ? carve_fov_keep_image(a->W, a->H, nullptr).bytes : carve_image(a->variant, a->W, a->H, nullptr).bytes);
	if (!gptr || !iptr) { set_error("geometry/image resize callback returned null"); return FR_ERR_ALLOC; }
	c.geom = carve_geom(a->variant, (size_t)a->P, gptr, c.fov.levels);
	c.img = carve_image(a->variant, a->W, a->H, iptr);
	if (keep)
	{
		// (behind the plain call's arrays: fr_geometry_bytes_fov_keep / fr_image_bytes_fov_keep)
		const FovKeepImage ki = carve_fov_keep_image(a->W, a->H, iptr);
		c.keep_T = ki.final_T; c.keep_n = ki.n_contrib;
		c.keep_acc = carve_fov_keep_geom((size_t)a->P, gptr, c.fov.levels).acc;
		if (keep == 2) c.keep_mom = carve_fov_full_geom((size_t)a->P, gptr, c.fov.levels).mom; // (behind the keep layout: fr_geometry_bytes_fov_keep_full)
		keep_state->geometry = gptr; keep_state->image = iptr;
	}

	// RF: the two level states of a two-level tile are blended by different waves, which ADD their halves to the image: those
	// tiles' pixels are cleared by k_project's waves beside their stream over the cloud (preprocess.hip). Before that: a fill
	// command over the whole image on the helper stream, 6 us and a queue slot of its own; clearing only those tiles inside
	// k_tile_levels tripled that kernel (11 -> 32 us: 45 workgroups cannot write this much).
	c.fov_split = a->variant == FR_VARIANT_FOV_PCHECK_OBB ? 1 : 0;
	// The frame's helper stream (s2 of the pair that belongs to this thread and launch stream) carries the large fills -- the
	// training variants' two statistics arrays -- beside the cull / binning kernels; only the blend kernel at the END of the
	// frame needs them and waits (fr_forward_finish).
	f->ax = (!a->debug && !a->no_helper_streams) ? aux_stream(stream) : nullptr;
	hipStream_t fill_stream = stream;
	const bool stats = (has_stats(a->variant) && !a->no_stats) || is_counting(a);
	if (f->ax && stats)
	{
		if (hipEventRecord(f->ax->fork, stream) != hipSuccess || hipStreamWaitEvent(f->ax->s2, f->ax->fork, 0) != hipSuccess) { (void)hipGetLastError(); f->ax = nullptr; }
		else fill_stream = f->ax->s2;
	}
	auto fills_done = [&]() { if (fill_stream != stream && hipEventRecord(f->ax->join2, f->ax->s2) == hipSuccess) f->aux_pending = true; };
	if (stats)
	{
		const hipError_t e1 = hipMemsetAsync(a->gaussians_count, 0, sizeof(int32_t) * (size_t)a->P, fill_stream);
		const hipError_t e2 = hipMemsetAsync(a->contributions, 0, sizeof(float) * (size_t)a->P, fill_stream);
		fills_done();
		if (e1 != hipSuccess || e2 != hipSuccess) { set_error("hipMemsetAsync(statistics): %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2)); return FR_ERR_HIP; }
	}
	// small clears in front of the first kernel: the per-tile instance counters (k_bin's workgroups add their shares to them;
	// the global-atomics path of huge tile grids counts in them directly) and, next to them, the level boxes (RF:
	// k_tile_levels raises them with atomicMax; it clears the slab counters itself)
	FR_HIP(hipMemsetAsync(c.img.tile_count, 0, (size_t)((char *)(c.img.lv_bbox + 5 * FR_LV_BBOX_STRIDE) - (char *)c.img.tile_count), stream)); // + lv_bbox
	if (!is_fov(a->variant)) // RF: k_tile_levels clears them
		FR_HIP(hipMemsetAsync(c.geom.slab_ctr, 0, FR_SLAB_CTR_WORDS * sizeof(uint32_t), stream));
	if (a->list_consumed) FR_HIP(hipMemsetAsync(a->list_consumed, 0, sizeof(uint32_t) * (size_t)c.T, stream));
	if (a->blend_pairs) FR_HIP(hipMemsetAsync(a->blend_pairs, 0, sizeof(uint32_t) * (size_t)c.T, stream));
	// this frame's tag, the totals block's sequence word: one counter per PROCESS, as the pool of blocks is -- no two frames in flight,
	// whatever threads they belong to, share a tag, and a block never holds the tag of the frame that takes it (0 is never a tag)
	static std::atomic<uint32_t> frame_seq{0};
	uint32_t seq = frame_seq.fetch_add(1, std::memory_order_relaxed) + 1;
	while (seq == 0) seq = frame_seq.fetch_add(1, std::memory_order_relaxed) + 1;
	c.totals_seq = seq;
	mark(FR_STAGE_TILE_LEVELS);
	if (is_fov(a->variant)) { rc = launch_tile_levels(c); if (rc) return rc; }
	// fr_forward_aux: the two level states of a two-level tile ADD their halves to the depth / coverage planes as they do to the image;
	// those tiles of the two planes are cleared by a kernel of their own, launched in such calls only (k_project's code stays what it is)
	if (c.fov_split && c.aux_depth) { rc = launch_aux_clear(c); if (rc) return rc; }
	if (c.geom.pad_op) { rc = launch_pad_levels(c); if (rc) return rc; } // (fr_foveation.levels other than 4 and 8)
	mark(FR_STAGE_PROJECT);
	rc = launch_project(c); if (rc) return rc;
	int cur_dev = 0;
	(void)hipGetDevice(&cur_dev);
	f->pin = a->debug ? nullptr : take_pinned(cur_dev);
	c.totals_host_dev = f->pin ? f->pin->dev : nullptr;
	c.scan_fused = 0;
	mark(FR_STAGE_BIN);
	f->scan_enqueued = true; // (from here on a dropped frame quarantines its block: ~fr_frame)
	rc = launch_bin(c); if (rc) return rc;
	mark(FR_STAGE_TILE_SCAN);
	if (!c.scan_fused) { rc = launch_tile_scan(c); if (rc) return rc; } // (else: k_bin's last workgroup did it)
	*out = f; guard.f = nullptr;
	return FR_OK;
}

} // namespace fr

extern "C" {

int fr_forward_begin_fov(fr_forward_args *a, const fr_forward_ext *ext, const fr_foveation *fov, fr_frame **out)
{
	return forward_begin(a, ext, fov, nullptr, 0, out);
}

int fr_forward_begin_fov_keep(fr_forward_args *a, const fr_forward_ext *ext, const fr_foveation *fov, fr_fov_state *state, fr_frame **out)
{
	return forward_begin(a, ext, fov, state, 1, out);
}

int fr_forward_begin_fov_keep_full(fr_forward_args *a, const fr_forward_ext *ext, const fr_foveation *fov, fr_fov_state *state, fr_frame **out)
{
	return forward_begin(a, ext, fov, state, 2, out);
}

int fr_forward_finish(fr_frame *f)
{
	if (!f) { set_error("null frame"); return FR_ERR_INVALID; }
	struct Guard { fr_frame *f; ~Guard() { delete f; } } guard = { f }; // the handle is released whatever happens
	if (f->empty) return FR_OK;
	fr_forward_args *a = f->a;
	FwdCtx &c = f->c;
	hipStream_t stream = c.stream;
	auto mark = [&](int i) { if (a->stage_events && a->stage_events[i]) (void)hipEventRecord((hipEvent_t)a->stage_events[i], stream); };
	// Everything behind the tile scan needs the frame's counts: the number of instances D (size of the binning workspace)
	// and the sort / blend class counts. They are on their way to the frame's pinned block, which the host polls: the
	// numbers land a few microseconds before k_tile_scan retires, so the launches that follow reach the queue while it still
	// runs and the GPU does not wait for the host.
	// The binning workspace is asked for BEFORE the count is in -- sized like the largest frame of this kind so far plus a
	// quarter -- while the GPU is still binning: the callback (the caller's allocator, a Python function behind ctypes in the
	// reference-shaped host code) is then off the critical path between the tile scan and k_emit. A frame that does not fit
	// asks again with its real size (the callback may therefore be called twice per frame; the last answer is the one in use).
	Guess &gs = guess_for(a->variant);
	const bool same_kind = gs.variant == a->variant && gs.P == a->P && gs.W == a->W && gs.H == a->H;
	char *early_bin = nullptr;
	const int64_t early_cap = (same_kind && !a->debug) ? gs.capacity : 0;
	if (early_cap > 0) early_bin = a->binning_resize(a->resize_user[1], carve_bin(early_cap, nullptr, c.T).bytes);

	uint32_t totals[10] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 }, candidates = 0;
	uint32_t *const pinned = f->pin ? f->pin->host : nullptr;
	if (!pinned)
	{
		FR_HIP(hipMemcpyAsync(totals, c.img.totals, sizeof(totals), hipMemcpyDeviceToHost, stream));
		FR_HIP(hipMemcpyAsync(&candidates, c.geom.slab_ctr + 1, sizeof(candidates), hipMemcpyDeviceToHost, stream));
		FR_HIP(hipStreamSynchronize(stream));
	}
	else
	{
		// poll the sequence word instead of sleeping on the stream: the numbers arrive a few microseconds before
		// the kernel retires, and the wake-up latency of a stream wait is saved. The stream is queried now and then
		// so that a failed launch cannot hang the caller.
		const volatile uint32_t *v = pinned;
		for (uint32_t spins = 1; __atomic_load_n(&pinned[4], __ATOMIC_ACQUIRE) != c.totals_seq; spins++)
			if ((spins & 0xffff) == 0)
			{
				const hipError_t q = hipStreamQuery(stream);
				if (q == hipErrorNotReady) continue;
				if (q != hipSuccess) { set_error("hip: %s", hipGetErrorString(q)); return FR_ERR_HIP; }
				if (__atomic_load_n(&pinned[4], __ATOMIC_ACQUIRE) != c.totals_seq) { set_error("tile scan did not publish its totals"); return FR_ERR_HIP; }
			}
		for (int i = 0; i < 4; i++) totals[i] = v[i];
		totals[5] = v[5]; totals[6] = v[6]; totals[7] = v[7]; candidates = v[8];
		totals[8] = v[10]; totals[9] = v[11]; // (the device's totals[8], [9]: word 8 of the block was taken, word 9 is unused)
	}
	f->totals_read = true;
	// reference auxiliary.h:156-160: a point behind the near plane although the caller said the cloud was prefiltered
	// (there: printf + __trap, which kills the context; here an error code)
	if (a->prefiltered && totals[7] != 0)
	{ set_error("Point is filtered although prefiltered is set. This shouldn't happen!"); return FR_ERR_PREFILTERED; }
	if (totals[0] > 0x7fffffffu) { set_error("too many instances (%u)", totals[0]); return FR_ERR_INVALID; }
	a->num_rendered = (int32_t)totals[0];
	a->max_tile_instances = (int32_t)totals[1];
	a->num_candidates = (int32_t)candidates;
	c.heavy4 = (int)totals[2]; c.heavy2 = (int)totals[3];
	c.n_items = (int)totals[5]; c.heavy8 = (int)totals[6];
	c.heavy16 = (int)totals[8]; c.heavy32 = (int)totals[9];
	// what the next frame of this kind will ask for: a quarter of headroom over the largest frame seen
	const int64_t want = (int64_t)totals[0] + (int64_t)totals[0] / 4 + 65536;
	if (!same_kind) { gs.variant = a->variant; gs.P = a->P; gs.W = a->W; gs.H = a->H; gs.capacity = 0; }
	if (want > gs.capacity) gs.capacity = want;

	const bool fits_early = early_bin && (int64_t)totals[0] <= early_cap;
	const int64_t capacity = fits_early ? early_cap : (int64_t)totals[0];
	char *bptr = fits_early ? early_bin : a->binning_resize(a->resize_user[1], carve_bin(capacity, nullptr, c.T).bytes);
	if (!bptr) { set_error("binning resize callback returned null"); return FR_ERR_ALLOC; }
	c.bin = carve_bin(capacity, bptr, c.T);
	c.capacity = capacity;
	c.items_cap = (int64_t)(c.fov_split ? 4 : 2) * c.T; // two bands per tile, twice that for an RF two-level tile
	int rc = FR_OK;
	mark(FR_STAGE_EMIT);
	if (a->num_rendered > 0) { rc = launch_emit(c); if (rc) return rc; }
	mark(FR_STAGE_TILE_SORT);
	if (a->num_rendered > 0) { rc = launch_tile_sort(c); if (rc) return rc; }
	mark(FR_STAGE_RENDER);
	f->join_aux(); // the fills of the frame's head
	if (c.keep)
	{
		// the backward pass adds into the rows of sums of the frame's items: they start as zeros
		rc = launch_fov_keep_clear(c); if (rc) return rc;
		f->keep_state->binning = bptr; f->keep_state->num_rendered = a->num_rendered; f->keep_state->num_items = c.n_items;
	}
	rc = launch_render(c);
	mark(FR_NUM_STAGES);
	return rc;
}

int fr_forward_abandon(fr_frame *f)
{
	if (!f) { set_error("null frame"); return FR_ERR_INVALID; }
	delete f; // ~fr_frame joins the helper stream and quarantines the pinned block (the frame's tile scan may not have written its totals yet)
	return FR_OK;
}

int fr_forward_begin_ext(fr_forward_args *a, const fr_forward_ext *ext, fr_frame **out) { return fr_forward_begin_fov(a, ext, nullptr, out); }
int fr_forward_begin(fr_forward_args *a, fr_frame **out) { return fr_forward_begin_fov(a, nullptr, nullptr, out); }

int fr_forward_fov_call(fr_forward_args *a, const fr_forward_ext *ext, const fr_foveation *fov)
{
	fr_frame *f = nullptr;
	const int rc = fr_forward_begin_fov(a, ext, fov, &f);
	if (rc) return rc;
	return fr_forward_finish(f);
}

int fr_forward_begin_aux(fr_forward_args *a, const fr_forward_ext *ext, const fr_foveation *fov, const fr_forward_aux *aux, fr_frame **out)
{
	return forward_begin(a, ext, fov, nullptr, 0, out, aux);
}

int fr_forward_aux_call(fr_forward_args *a, const fr_forward_ext *ext, const fr_foveation *fov, const fr_forward_aux *aux)
{
	fr_frame *f = nullptr;
	const int rc = fr_forward_begin_aux(a, ext, fov, aux, &f);
	if (rc) return rc;
	return fr_forward_finish(f);
}

int fr_forward_fov_keep_call(fr_forward_args *a, const fr_forward_ext *ext, const fr_foveation *fov, fr_fov_state *state)
{
	fr_frame *f = nullptr;
	const int rc = fr_forward_begin_fov_keep(a, ext, fov, state, &f);
	if (rc) return rc;
	return fr_forward_finish(f);
}

int fr_forward_fov_keep_full_call(fr_forward_args *a, const fr_forward_ext *ext, const fr_foveation *fov, fr_fov_state *state)
{
	fr_frame *f = nullptr;
	const int rc = fr_forward_begin_fov_keep_full(a, ext, fov, state, &f);
	if (rc) return rc;
	return fr_forward_finish(f);
}

size_t fr_geometry_bytes_fov_keep_full(int32_t P, int32_t levels)
{
	if (P < 0 || levels < 2 || levels > FR_FOV_LEVELS) { set_error("bad geometry_bytes_fov_keep_full arguments (levels 2 .. %d)", FR_FOV_LEVELS); return 0; }
	return carve_fov_full_geom((size_t)P, nullptr, levels).bytes;
}

size_t fr_geometry_bytes_fov_keep(int32_t P, int32_t levels)
{
	if (P < 0 || levels < 2 || levels > FR_FOV_LEVELS) { set_error("bad geometry_bytes_fov_keep arguments (levels 2 .. %d)", FR_FOV_LEVELS); return 0; }
	return carve_fov_keep_geom((size_t)P, nullptr, levels).bytes;
}
size_t fr_image_bytes_fov_keep(int32_t W, int32_t H) { return carve_fov_keep_image(W, H, nullptr).bytes; }
const float *fr_image_fov_state_T(int32_t W, int32_t H, const char *image) { return carve_fov_keep_image(W, H, (char *)image).final_T; }
const uint32_t *fr_image_fov_state_n(int32_t W, int32_t H, const char *image) { return carve_fov_keep_image(W, H, (char *)image).n_contrib; }

int fr_forward_ext_call(fr_forward_args *a, const fr_forward_ext *ext) { return fr_forward_fov_call(a, ext, nullptr); }

int fr_forward(fr_forward_args *a) { return fr_forward_ext_call(a, nullptr); }

int fr_pack_geom(int32_t P, const float *means3D, const float *scales, const float *rotations, const float *opacities,
	int32_t levels, const float *highest_levels, float *packed_geom, void *stream)
{
	if (P < 0 || levels < 1 || levels > 4 || (P > 0 && (!means3D || !scales || !rotations || !opacities || !packed_geom)))
	{ set_error("bad pack_geom arguments"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	return launch_pack_geom(P, means3D, scales, rotations, opacities, levels, highest_levels, packed_geom, (hipStream_t)stream);
}

int fr_pack_cull(int32_t P, const float *means3D, const float *scales, const float *rotations, float *packed_cull, void *stream)
{
	if (P < 0 || (P > 0 && (!means3D || !scales || !rotations || !packed_cull))) { set_error("bad pack_cull arguments"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	return launch_pack_cull(P, means3D, scales, rotations, packed_cull, (hipStream_t)stream);
}

int fr_pack_colour(int32_t P, const float *shs, const float *shs_rest, const float *shs_dcs, float *packed_colour, void *stream)
{
	if (P < 0 || (P > 0 && (!shs || !packed_colour)) || (shs_rest && shs_dcs)) { set_error("bad pack_colour arguments"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	return launch_pack_colour(P, shs, shs_rest, shs_dcs, packed_colour, (hipStream_t)stream);
}

int fr_pack_colour_fov(int32_t P, const float *shs, const float *shs_dcs, int32_t levels, float *packed_colour, void *stream)
{
	if (P < 0 || levels < 1 || levels > FR_FOV_LEVELS || (P > 0 && (!shs || !shs_dcs || !packed_colour))) { set_error("bad pack_colour_fov arguments"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	return launch_pack_colour(P, shs, nullptr, shs_dcs, packed_colour, (hipStream_t)stream, levels);
}

int fr_activate_forward(int32_t P, const float *raw_scaling, const float *raw_rotation, const float *raw_opacity, float *scaling, float *rotation,
	float *opacity, void *stream)
{
	if (P < 0 || (P > 0 && (!raw_scaling || !raw_rotation || !raw_opacity || !scaling || !rotation || !opacity))) { set_error("bad activate_forward arguments"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	return launch_activate_forward(P, raw_scaling, raw_rotation, raw_opacity, scaling, rotation, opacity, (hipStream_t)stream);
}

int fr_activate_backward(int32_t P, const float *raw_scaling, const float *raw_rotation, const float *raw_opacity, const float *dL_dscaling,
	const float *dL_drotation, const float *dL_dopacity, float *dL_draw_scaling, float *dL_draw_rotation, float *dL_draw_opacity, void *stream)
{
	if (P < 0 || (P > 0 && (!raw_scaling || !raw_rotation || !raw_opacity || !dL_draw_scaling || !dL_draw_rotation || !dL_draw_opacity)))
	{ set_error("bad activate_backward arguments"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	return launch_activate_backward(P, raw_scaling, raw_rotation, raw_opacity, dL_dscaling, dL_drotation, dL_dopacity, dL_draw_scaling, dL_draw_rotation,
		dL_draw_opacity, (hipStream_t)stream);
}

int64_t fr_l1_ssim_blocks(int32_t C, int32_t H, int32_t W)
{
	if (C <= 0 || H <= 0 || W <= 0) return 0;
	return (int64_t)C * ((H + 31) / 32) * ((W + 15) / 16); // one (sum |x - y|, sum ssim) pair per 16 x 32 tile, see loss.hip
}

int fr_l1_ssim_forward(int32_t C, int32_t H, int32_t W, const float *img, const float *target, float *dmaps, float *partials, void *stream)
{
	if (C <= 0 || H <= 0 || W <= 0 || C > 65535 || !img || !target || !partials) { set_error("bad l1_ssim_forward arguments"); return FR_ERR_INVALID; }
	return launch_l1_ssim_forward(C, H, W, img, target, dmaps, partials, (hipStream_t)stream);
}

int fr_l1_ssim_finish(int32_t C, int32_t H, int32_t W, const float *partials, float lambda_dssim, float *out3, void *stream)
{
	if (C <= 0 || H <= 0 || W <= 0 || C > 65535 || !partials || !out3) { set_error("bad l1_ssim_finish arguments"); return FR_ERR_INVALID; }
	return launch_l1_ssim_finish((int)fr_l1_ssim_blocks(C, H, W), (double)C * H * W, partials, lambda_dssim, out3, (hipStream_t)stream);
}

int fr_l1_ssim_backward(int32_t C, int32_t H, int32_t W, const float *img, const float *target, const float *dmaps, float w_l1, float w_ssim,
	const float *grad_scale, float *dL_dimg, void *stream)
{
	if (C <= 0 || H <= 0 || W <= 0 || C > 65535 || !img || !target || !dmaps || !dL_dimg) { set_error("bad l1_ssim_backward arguments"); return FR_ERR_INVALID; }
	return launch_l1_ssim_backward(C, H, W, img, target, dmaps, w_l1, w_ssim, grad_scale, dL_dimg, (hipStream_t)stream);
}

size_t fr_knn_workspace_bytes(int32_t P) { return knn_workspace_bytes(P); }

int fr_knn_mean_dist2(int32_t P, const float *points, float *mean_dist2, void *workspace, void *stream)
{
	if (P < 0 || (P > 0 && (!points || !mean_dist2 || !workspace))) { set_error("bad knn_mean_dist2 arguments (P=%d)", P); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	if ((uintptr_t)workspace % 16) { set_error("knn workspace must be 16-byte aligned"); return FR_ERR_INVALID; }
	return launch_knn(P, points, mean_dist2, workspace, (hipStream_t)stream);
}

int fr_adam_step(const fr_adam_args *a, void *stream)
{
	if (!a) { set_error("null args"); return FR_ERR_INVALID; }
	if (a->num_tensors < 0 || a->num_tensors > FR_ADAM_MAX_TENSORS) { set_error("adam_step: %d tensors (at most %d)", a->num_tensors, FR_ADAM_MAX_TENSORS); return FR_ERR_INVALID; }
	for (int k = 0; k < a->num_tensors; k++)
	{
		const fr_adam_tensor &t = a->tensors[k];
		if (t.numel < 0 || t.n_rows < 0 || t.width <= 0 || t.mode < FR_ADAM_DENSE || t.mode > FR_ADAM_LAZY)
		{ set_error("adam_step: tensor %d: bad sizes (numel=%lld n_rows=%lld width=%d mode=%d)", k, (long long)t.numel, (long long)t.n_rows, t.width, t.mode); return FR_ERR_INVALID; }
		if (t.numel == 0) continue;
		if (!t.param || !t.exp_avg || !t.exp_avg_sq) { set_error("adam_step: tensor %d: a state pointer is null", k); return FR_ERR_INVALID; }
		if (t.mode == FR_ADAM_DENSE ? !t.grad : (t.n_rows > 0 && (!t.grad || !t.rows))) { set_error("adam_step: tensor %d: gradient pointer is null", k); return FR_ERR_INVALID; }
		if (t.mode != FR_ADAM_DENSE && (t.numel % t.width || t.n_rows > t.numel / t.width))
		{ set_error("adam_step: tensor %d: %lld rows of width %d do not fit %lld elements", k, (long long)t.n_rows, t.width, (long long)t.numel); return FR_ERR_INVALID; }
	}
	const fr_adam_tensor *first = nullptr; // the tensors that share the row map share what it is built from
	for (int k = 0; k < a->num_tensors; k++)
	{
		const fr_adam_tensor &t = a->tensors[k];
		if (t.mode != FR_ADAM_EXACT || !t.row_map || t.n_rows == 0 || t.numel == 0) continue;
		if (t.n_rows > 0x7fffffff) { set_error("adam_step: tensor %d: too many rows for a row map", k); return FR_ERR_INVALID; }
		if (!first) first = &t;
		else if (t.row_map != first->row_map || t.rows != first->rows || t.n_rows != first->n_rows || t.numel / t.width != first->numel / first->width)
		{ set_error("adam_step: tensor %d: one row map per call, shared only by tensors with the same rows", k); return FR_ERR_INVALID; }
	}
	return launch_adam(a, (hipStream_t)stream);
}

size_t fr_prune_workspace_bytes(int32_t P) { return prune_workspace_bytes(P); }

int fr_prune_metric_max(int32_t P, int32_t kind, const float *contribs, const int32_t *counts, float *metrics, void *stream)
{
	if (P < 0) { set_error("prune_metric_max: bad size P=%d", P); return FR_ERR_INVALID; }
	if (kind != FR_PRUNE_MAX_COMP_EFFICIENCY && kind != FR_PRUNE_CONTRIB) { set_error("prune_metric_max: unknown kind %d", kind); return FR_ERR_INVALID; }
	if (P > 0 && (!contribs || !metrics || (kind == FR_PRUNE_MAX_COMP_EFFICIENCY && !counts))) { set_error("prune_metric_max: a required pointer is null"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	return launch_prune_metric(P, kind, contribs, counts, metrics, (hipStream_t)stream);
}

int fr_prune_select_lowest(int32_t P, const float *metrics, int64_t k, uint8_t *mask, void *workspace, void *stream)
{
	if (P < 0) { set_error("prune_select_lowest: bad size P=%d", P); return FR_ERR_INVALID; }
	if (k < 0 || k > P) { set_error("prune_select_lowest: k=%lld is not in 0..P=%d", (long long)k, P); return FR_ERR_INVALID; }
	if (P > 0 && (!metrics || !mask || !workspace)) { set_error("prune_select_lowest: a required pointer is null"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	if ((uintptr_t)workspace % 16) { set_error("prune workspace must be 16-byte aligned"); return FR_ERR_INVALID; }
	return launch_prune_select(P, metrics, k, mask, workspace, (hipStream_t)stream);
}

int fr_compact_plan(int32_t P, const uint8_t *mask, int32_t invert, int32_t *count_out, void *workspace, void *stream)
{
	if (P < 0) { set_error("compact_plan: bad size P=%d", P); return FR_ERR_INVALID; }
	if (P > 0 && (!mask || !count_out || !workspace)) { set_error("compact_plan: a required pointer is null"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK; // (nothing launched: *count_out is not written)
	if ((uintptr_t)workspace % 16) { set_error("prune workspace must be 16-byte aligned"); return FR_ERR_INVALID; }
	return launch_compact_plan(P, mask, invert, count_out, workspace, (hipStream_t)stream);
}

int fr_compact_rows(const fr_compact_args *a, void *stream)
{
	if (!a) { set_error("null args"); return FR_ERR_INVALID; }
	if (a->P < 0) { set_error("compact_rows: bad size P=%d", a->P); return FR_ERR_INVALID; }
	if (a->num_tensors < 0 || a->num_tensors > FR_COMPACT_MAX_TENSORS) { set_error("compact_rows: %d tensors (at most %d)", a->num_tensors, FR_COMPACT_MAX_TENSORS); return FR_ERR_INVALID; }
	if (a->P > 0 && (!a->mask || !a->workspace)) { set_error("compact_rows: mask or workspace is null"); return FR_ERR_INVALID; }
	for (int k = 0; k < a->num_tensors; k++)
	{
		const fr_compact_tensor &t = a->tensors[k];
		if (t.row_words < 0 || t.dst_rows < 0 || t.dst_rows > a->P) { set_error("compact_rows: tensor %d: bad sizes (row_words=%d dst_rows=%d P=%d)", k, t.row_words, t.dst_rows, a->P); return FR_ERR_INVALID; }
		if (a->P > 0 && t.row_words > 0 && t.dst_rows > 0 && (!t.src || !t.dst)) { set_error("compact_rows: tensor %d: a data pointer is null", k); return FR_ERR_INVALID; }
	}
	if (a->P == 0 || a->num_tensors == 0) return FR_OK;
	if ((uintptr_t)a->workspace % 16) { set_error("prune workspace must be 16-byte aligned"); return FR_ERR_INVALID; }
	return launch_compact_rows(a, (hipStream_t)stream);
}

int fr_select_kth(int32_t P, const void *values, int32_t dtype, int64_t k, void *kth_out, void *workspace, void *stream)
{
	if (P < 0) { set_error("select_kth: bad size P=%d", P); return FR_ERR_INVALID; }
	if (dtype != 0 && dtype != 1) { set_error("select_kth: unknown dtype %d (0 = fp32, 1 = int32)", dtype); return FR_ERR_INVALID; }
	// (P = 0 has no element of any rank)
	if (k < 0 || k >= P) { set_error("select_kth: k=%lld is not in 0..P-1=%d", (long long)k, P - 1); return FR_ERR_INVALID; }
	if (!values || !kth_out || !workspace) { set_error("select_kth: a required pointer is null"); return FR_ERR_INVALID; }
	if ((uintptr_t)workspace % 16) { set_error("prune workspace must be 16-byte aligned"); return FR_ERR_INVALID; }
	return launch_select_kth(P, values, dtype, k, kth_out, workspace, (hipStream_t)stream);
}

int fr_mask_le(int32_t P, const void *values, int32_t dtype, const void *threshold_dev, uint8_t *mask, void *stream)
{
	if (P < 0) { set_error("mask_le: bad size P=%d", P); return FR_ERR_INVALID; }
	if (dtype != 0 && dtype != 1) { set_error("mask_le: unknown dtype %d (0 = fp32, 1 = int32)", dtype); return FR_ERR_INVALID; }
	if (P > 0 && (!values || !threshold_dev || !mask)) { set_error("mask_le: a required pointer is null"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	return launch_mask_le(P, values, dtype, threshold_dev, mask, (hipStream_t)stream);
}

int fr_volume(int32_t P, const float *scaling, int32_t raw, float *volume, void *stream)
{
	if (P < 0) { set_error("volume: bad size P=%d", P); return FR_ERR_INVALID; }
	if (P > 0 && (!scaling || !volume)) { set_error("volume: a required pointer is null"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	return launch_volume(P, scaling, raw, volume, (hipStream_t)stream);
}

int fr_v_importance(int32_t P, const float *volume, const float *kth_volume_dev, float v_pow, const float *imp, float *out, void *stream)
{
	if (P < 0) { set_error("v_importance: bad size P=%d", P); return FR_ERR_INVALID; }
	if (P > 0 && (!volume || !kth_volume_dev || !imp || !out)) { set_error("v_importance: a required pointer is null"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	return launch_v_importance(P, volume, kth_volume_dev, v_pow, imp, out, (hipStream_t)stream);
}

size_t fr_densify_workspace_bytes(int32_t P) { return densify_workspace_bytes(P); }

int fr_densify_stats(int32_t P, const float *grad, const uint8_t *update_filter, float *accum, float *denom, void *stream)
{
	if (P < 0) { set_error("densify_stats: bad size P=%d", P); return FR_ERR_INVALID; }
	if (P > 0 && (!grad || !update_filter || !accum || !denom)) { set_error("densify_stats: a required pointer is null"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	return launch_densify_stats(P, grad, update_filter, accum, denom, (hipStream_t)stream);
}

int fr_densify_plan(const fr_densify_plan_args *a, void *stream)
{
	if (!a) { set_error("null args"); return FR_ERR_INVALID; }
	if (a->P < 0) { set_error("densify_plan: bad size P=%d", a->P); return FR_ERR_INVALID; }
	if (a->mode < FR_DENSIFY_CLONE_MASK || a->mode > FR_DENSIFY_AND_PRUNE) { set_error("densify_plan: unknown mode %d", a->mode); return FR_ERR_INVALID; }
	if (a->N < 1 || a->N > 4) { set_error("densify_plan: N=%d is not in 1..4", a->N); return FR_ERR_INVALID; }
	if (a->P == 0) return FR_OK; // (nothing launched: counts_out is not written)
	if (!a->counts_out || !a->workspace) { set_error("densify_plan: counts_out or workspace is null"); return FR_ERR_INVALID; }
	if ((uintptr_t)a->workspace % 16) { set_error("densify workspace must be 16-byte aligned"); return FR_ERR_INVALID; }
	const bool by_mask = a->mode == FR_DENSIFY_CLONE_MASK || a->mode == FR_DENSIFY_SPLIT_MASK;
	if (by_mask && !a->mask) { set_error("densify_plan: mode %d needs a mask", a->mode); return FR_ERR_INVALID; }
	if (!by_mask)
	{
		if (a->n_grad < 0 || a->n_grad > a->P) { set_error("densify_plan: n_grad=%d is not in 0..P=%d", a->n_grad, a->P); return FR_ERR_INVALID; }
		if (!a->scaling || (a->n_grad > 0 && !a->accum)) { set_error("densify_plan: scaling or accum is null"); return FR_ERR_INVALID; }
		if (a->mode == FR_DENSIFY_AND_PRUNE && (!a->opacity || !a->denom || a->n_grad != a->P))
		{ set_error("densify_plan: densify_and_prune needs opacity, denom and n_grad = P"); return FR_ERR_INVALID; }
	}
	return launch_densify_plan(a, (hipStream_t)stream);
}

int fr_densify_rows(const fr_densify_rows_args *a, void *stream)
{
	if (!a) { set_error("null args"); return FR_ERR_INVALID; }
	if (a->P < 0) { set_error("densify_rows: bad size P=%d", a->P); return FR_ERR_INVALID; }
	if (a->N < 1 || a->N > 4) { set_error("densify_rows: N=%d is not in 1..4", a->N); return FR_ERR_INVALID; }
	if (a->num_tensors < 0 || a->num_tensors > FR_COMPACT_MAX_TENSORS) { set_error("densify_rows: %d tensors (at most %d)", a->num_tensors, FR_COMPACT_MAX_TENSORS); return FR_ERR_INVALID; }
	if (a->n_keep < 0 || a->n_keep > a->P || a->n_clone < 0 || a->n_clone > a->P || a->n_split < 0 || a->n_split > a->P || a->n_child < 0 || a->n_child > a->n_split)
	{ set_error("densify_rows: bad counts (keep=%d clone=%d split=%d child=%d P=%d)", a->n_keep, a->n_clone, a->n_split, a->n_child, a->P); return FR_ERR_INVALID; }
	const int64_t rows = (int64_t)a->n_keep + a->n_clone + (int64_t)a->N * a->n_child;
	if (rows > 0x7fffffff) { set_error("densify_rows: %lld output rows do not fit an int32", (long long)rows); return FR_ERR_INVALID; }
	if (a->P == 0 || a->num_tensors == 0 || rows == 0) return FR_OK;
	if (!a->workspace) { set_error("densify_rows: workspace is null"); return FR_ERR_INVALID; }
	if ((uintptr_t)a->workspace % 16) { set_error("densify workspace must be 16-byte aligned"); return FR_ERR_INVALID; }
	for (int k = 0; k < a->num_tensors; k++)
	{
		const fr_densify_tensor &t = a->tensors[k];
		if (t.row_words < 0 || t.role < FR_DENSIFY_COPY || t.role > FR_DENSIFY_SCALING) { set_error("densify_rows: tensor %d: bad row_words=%d or role=%d", k, t.row_words, t.role); return FR_ERR_INVALID; }
		if (t.row_words > 0 && (!t.src || !t.dst)) { set_error("densify_rows: tensor %d: a data pointer is null", k); return FR_ERR_INVALID; }
		if (t.role >= FR_DENSIFY_XYZ)
		{
			if (t.row_words != 3) { set_error("densify_rows: tensor %d: role %d needs rows of 3 words, not %d", k, t.role, t.row_words); return FR_ERR_INVALID; }
			if (a->n_child > 0 && (!a->scaling || (t.role == FR_DENSIFY_XYZ && (!a->rotation || !a->noise))))
			{ set_error("densify_rows: tensor %d: role %d needs scaling (xyz: rotation and noise too)", k, t.role); return FR_ERR_INVALID; }
		}
	}
	return launch_densify_rows(a, (hipStream_t)stream);
}

int fr_backward(const fr_backward_args *a)
{
	if (!a) { set_error("null args"); return FR_ERR_INVALID; }
	if (!has_backward(a->variant))
	{ set_error("backward exists only for the original and pcheck_obb_sum/_max/_loss_weighted_max_count variants (the reference's inference variants have none)"); return FR_ERR_INVALID; }
	if (a->P == 0) return FR_OK;
	if (!a->geometry || !a->image || (a->R > 0 && !a->binning) || !a->dL_dpix || !a->radii) { set_error("missing workspace / gradient pointer"); return FR_ERR_INVALID; }
	if (!a->dL_dmean2D || !a->dL_dopacity || !a->dL_dmean3D || (!a->dL_dcov3D && a->cov3D_precomp) || (!a->dL_dcolor && a->colors_precomp) || !a->dL_dscale || !a->dL_drot)
	{ set_error("missing gradient output pointer"); return FR_ERR_INVALID; }
	if (a->shs && !a->dL_dsh) { set_error("dL_dsh is null"); return FR_ERR_INVALID; }
	if (a->shs_rest && (!a->shs || !a->dL_dsh_rest)) { set_error("shs_rest needs shs and dL_dsh_rest"); return FR_ERR_INVALID; }
	if (a->raw_activations && a->cov3D_precomp) { set_error("raw_activations needs scales + rotations"); return FR_ERR_INVALID; }
	// (row_sparse promises that every compact row is written: with cov3D_precomp nobody writes dL_dscale / dL_drot)
	if (a->row_sparse && a->cov3D_precomp) { set_error("row_sparse needs scales + rotations (with cov3D_precomp the dL_dscale / dL_drot rows would stay unwritten)"); return FR_ERR_INVALID; }
	return launch_backward(a);
}

int fr_backward_appearance(const fr_backward_args *a)
{
	if (!a) { set_error("null args"); return FR_ERR_INVALID; }
	if (!has_backward(a->variant))
	{ set_error("backward exists only for the original and pcheck_obb_sum/_max/_loss_weighted_max_count variants (the reference's inference variants have none)"); return FR_ERR_INVALID; }
	// only the opacity and the colour are differentiated: a pointer for anything else would stay unwritten, so it is refused
	const struct { const void *p; const char *name; } forbidden[] = {
		{ a->dL_dmean2D, "dL_dmean2D" }, { a->dL_dconic, "dL_dconic" }, { a->dL_dmean3D, "dL_dmean3D" }, { a->dL_dcov3D, "dL_dcov3D" },
		{ a->dL_dscale, "dL_dscale" }, { a->dL_drot, "dL_drot" }, { a->dL_dsh_rest, "dL_dsh_rest" } };
	for (const auto &f : forbidden)
		if (f.p) { set_error("backward_appearance: %s must be NULL (only dL_dopacity, dL_dsh = the DC part and dL_dcolor are written)", f.name); return FR_ERR_INVALID; }
	if (a->P == 0) return FR_OK;
	if (!a->geometry || !a->image || (a->R > 0 && !a->binning) || !a->dL_dpix || !a->background) { set_error("missing workspace / gradient pointer"); return FR_ERR_INVALID; }
	if (!a->dL_dopacity) { set_error("backward_appearance: dL_dopacity is null"); return FR_ERR_INVALID; }
	if (a->dL_dsh && (!a->shs || a->colors_precomp)) { set_error("backward_appearance: dL_dsh needs shs (with colors_precomp ask for dL_dcolor)"); return FR_ERR_INVALID; }
	if (a->raw_activations && a->cov3D_precomp) { set_error("raw_activations needs scales + rotations"); return FR_ERR_INVALID; }
	return launch_backward_appearance(a);
}

int fr_backward_fov_appearance(const fr_backward_fov_args *a)
{
	if (!a) { set_error("null args"); return FR_ERR_INVALID; }
	if (a->size < sizeof(fr_backward_fov_args)) { set_error("fr_backward_fov_args.size is %u, expected at least %u", a->size, (unsigned)sizeof(fr_backward_fov_args)); return FR_ERR_INVALID; }
	const fr_fov_state *st = a->state;
	const int rc = validate_fov_state(st, "backward_fov_appearance", false);
	if (rc) return rc;
	if (st->P == 0) return FR_OK;
	if (!a->dL_dpix) { set_error("backward_fov_appearance: dL_dpix is null"); return FR_ERR_INVALID; }
	if (!a->background) { set_error("backward_fov_appearance: background is null"); return FR_ERR_INVALID; }
	if (!a->dL_dopacities) { set_error("backward_fov_appearance: dL_dopacities is null"); return FR_ERR_INVALID; }
	if (!a->dL_dshs_dcs) { set_error("backward_fov_appearance: dL_dshs_dcs is null"); return FR_ERR_INVALID; }
	return launch_backward_fov_appearance(a);
}

int fr_backward_fov(const fr_backward_fov_full_args *a)
{
	if (!a) { set_error("null arguments"); return FR_ERR_INVALID; }
	if (a->size < sizeof(fr_backward_fov_full_args)) { set_error("fr_backward_fov_full_args.size is %u, expected at least %u", a->size, (unsigned)sizeof(fr_backward_fov_full_args)); return FR_ERR_INVALID; }
	const fr_fov_state *st = a->state;
	const int rc = validate_fov_state(st, "backward_fov", true);
	if (rc) return rc;
	if (a->P != st->P) { set_error("backward_fov: P is %d, the state's %d", a->P, st->P); return FR_ERR_INVALID; }
	if (a->M < 1 || a->M > 16 || a->sh_degree < 0 || a->sh_degree > 3 || (a->sh_degree + 1) * (a->sh_degree + 1) > a->M)
	{ set_error("backward_fov: M is %d and sh_degree %d (1 <= (sh_degree + 1)^2 <= M <= 16)", a->M, a->sh_degree); return FR_ERR_INVALID; }
	const struct { const void *p; const char *name; } need[] = { { a->means3D, "means3D" }, { a->scales, "scales" }, { a->rotations, "rotations" },
		{ a->M > 1 ? (const void *)a->shs_rest : (const void *)a, "shs_rest" }, { a->viewmatrix, "viewmatrix" }, { a->projmatrix, "projmatrix" }, { a->campos, "campos" },
		{ a->background, "background" }, { a->dL_dpix, "dL_dpix" }, { a->dL_dopacities, "dL_dopacities" }, { a->dL_dshs_dcs, "dL_dshs_dcs" },
		{ a->M > 1 ? (const void *)a->dL_dshs_rest : (const void *)a, "dL_dshs_rest" }, { a->dL_dmeans3D, "dL_dmeans3D" }, { a->dL_dscales, "dL_dscales" },
		{ a->dL_drotations, "dL_drotations" }, { a->dL_dmeans2D, "dL_dmeans2D" } };
	for (const auto &n : need) if (!n.p) { set_error("backward_fov: %s is null", n.name); return FR_ERR_INVALID; }
	return launch_backward_fov_full(a);
}

int fr_backward_prefill(const fr_backward_args *a, void *fill_stream)
{
	if (!a) { set_error("null args"); return FR_ERR_INVALID; }
	if (a->P <= 0) return FR_OK;
	return launch_gradient_fill(a, (hipStream_t)fill_stream, false, true);
}

int fr_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, const float *projmatrix, uint8_t *present, void *stream)
{
	(void)projmatrix;
	if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) { set_error("bad mark_visible arguments"); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	return launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream);
}

} // extern "C"
