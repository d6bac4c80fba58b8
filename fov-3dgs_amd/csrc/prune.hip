// fovraster -- the pruning step of the Fov-3DGS loop: the per-view importance metric, the mask of the k least important
// Gaussians, and the cut of those rows out of every per-Gaussian tensor.
//
// Reference (fov3dgs/prune.py:71-110, the same loop in fov3dgs/metric_mask_learn.py:72-111;
// fov3dgs/scene/gaussian_model.py:624-664): ten elementwise torch passes per view for the metric, a full torch.sort of all
// P metrics to find the lowest prune_ratio of them plus a float mask scatter, and 21 tensor[mask] gathers, each with its own
// nonzero and host synchronisation. The unstable sort picks an arbitrary subset of a tied run, and most metrics tie at 0.
//
// Contract (include/fovraster.h): the metric is the torch expression bit for bit; the mask holds exactly k ones, the k
// smallest rows under the total order (key(m), index); out[j] = src[i_j] bitwise for the kept rows i_0 < i_1 < ...
//
// Kernels, all on the caller's stream, integer atomics only inside LDS, cross-workgroup totals as plain stores that a
// following kernel consumes, no host round trip, so every output is one bit pattern, run after run:
//   k_prune_metric    metrics[i] = metrics[i] < cur ? cur : metrics[i]
//   k_prune_hist / k_prune_pick
//                     radix select, 4 x 8 bits from the top: LDS digit histograms of the keys that match the digits
//                     found so far (one row of 256 counts per workgroup), then one workgroup that adds the rows, finds
//                     the digit that holds rank k and leaves (threshold so far, rank inside it) for the next pass
//   k_select_tail     fr_select_kth (LightGaussian's percentile thresholds, significance.hip): the same four passes over fp32
//                     or int32 values, then the threshold key turned back into the value of rank k
//   k_prune_tie_count / k_prune_scan / k_prune_write
//                     rows with key == threshold per tile, their exclusive running sum in index order, and the mask:
//                     key < T, or key == T and fewer than r equal keys before it
//   k_compact_count / k_prune_scan / k_compact_rows
//                     kept rows per tile, first destination row of every tile (+ the total), and the gather of every
//                     tensor of the table in one launch: grid (tiles, tensors)
#include "common.h"
#include "row_scan.h"

// the metric must round exactly as written: no contraction, a correctly rounded division
#pragma clang fp contract(off)

namespace fr {

#define PRUNE_HIST_WGS 256   // most workgroups (= rows of counts) of a histogram pass; the tiles are dealt round-robin
#define PRUNE_HIST_UNROLL 4  // tiles whose keys a histogram workgroup has in flight at a time

struct PruneLayout {
	size_t bytes;
	size_t hist, state, tie, first; // byte offsets
	int64_t tiles;
};

static PruneLayout prune_layout(int64_t P)
{
	PruneLayout L{};
	L.tiles = (P + PRUNE_TILE - 1) / PRUNE_TILE;
	size_t o = 0;
	L.hist = o;  o = align_up(o + (size_t)PRUNE_HIST_WGS * 256 * sizeof(uint32_t));
	L.state = o; o = align_up(o + 16 * sizeof(uint32_t));                  // {threshold key so far, rank inside it}
	L.tie = o;   o = align_up(o + (size_t)L.tiles * sizeof(uint32_t));     // select: rows with key == T per tile, then their running sum
	L.first = o; o = align_up(o + (size_t)L.tiles * sizeof(uint32_t));     // compaction: kept rows per tile, then the first destination row
	L.bytes = o;
	return L;
}

size_t prune_workspace_bytes(int P) { return P > 0 ? prune_layout(P).bytes : 0; }

// ---- helpers ---------------------------------------------------------------------------------------------------------
// total order of the select: ascending key = torch.sort(stable=True)'s ascending order of the floats (NaN last, -0 == +0)
__device__ __forceinline__ uint32_t prune_key(float m)
{
	const uint32_t b = __float_as_uint(m);
	if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
	if ((b & 0x7fffffffu) == 0u) return 0x80000000u;
	return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// ... and of int32 values (fr_select_kth with dtype 1: summed hit counts exceed 2^24, so no detour through float): the words
// travel through the same loads as the floats' bit patterns, and the key is the value with its sign bit flipped
template <int DT>
__device__ __forceinline__ uint32_t prune_key_of(float m) { return DT == 1 ? __float_as_uint(m) ^ 0x80000000u : prune_key(m); }

// the keys of rows i .. i + 3 (0 where i + j >= P) and, as the return value, how many of them exist
template <int DT = 0>
__device__ __forceinline__ int prune_load_keys(const float *__restrict__ metrics, size_t i, size_t P, bool aligned, uint32_t key[PRUNE_PER_THREAD])
{
	if (i + PRUNE_PER_THREAD <= P && aligned)
	{
		const float4 v = *(const float4 *)(metrics + i);
		key[0] = prune_key_of<DT>(v.x); key[1] = prune_key_of<DT>(v.y); key[2] = prune_key_of<DT>(v.z); key[3] = prune_key_of<DT>(v.w);
		return PRUNE_PER_THREAD;
	}
	int n = 0;
#pragma unroll
	for (int j = 0; j < PRUNE_PER_THREAD; j++)
	{
		const bool valid = i + j < P;
		key[j] = valid ? prune_key_of<DT>(metrics[i + j]) : 0u;
		n += valid;
	}
	return n;
}

// bit j: row i + j exists and is kept (mask byte != 0, the other way round with invert)
__device__ __forceinline__ uint32_t compact_kept_bits(const uint8_t *__restrict__ mask, size_t i, size_t P, bool aligned, int invert)
{
	uint32_t bits = 0;
	if (i + PRUNE_PER_THREAD <= P && aligned)
	{
		const uint32_t v = *(const uint32_t *)(mask + i);
#pragma unroll
		for (int j = 0; j < PRUNE_PER_THREAD; j++) bits |= (uint32_t)((((v >> (8 * j)) & 255u) != 0u) != (invert != 0)) << j;
		return bits;
	}
#pragma unroll
	for (int j = 0; j < PRUNE_PER_THREAD; j++)
		if (i + j < P) bits |= (uint32_t)((mask[i + j] != 0) != (invert != 0)) << j;
	return bits;
}

// ---- metric ----------------------------------------------------------------------------------------------------------
// prune.py:79-98. kind 0: cur = contribs / (float(count) + 1e-7f), 0 where count < 1; kind 1: cur = contribs. A NaN cur
// fails `metrics < cur` and leaves the old value, as the reference's masked assignment does.
template <int KIND>
__global__ void __launch_bounds__(256) k_prune_metric(int P, const float *__restrict__ contribs, const int32_t *__restrict__ counts, float *__restrict__ metrics)
{
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * 256)
	{
		float cur = contribs[i];
		if (KIND == FR_PRUNE_MAX_COMP_EFFICIENCY)
		{
			const int32_t c = counts[i];
			cur = c < 1 ? 0.0f : cur / ((float)c + 1e-7f);
		}
		if (metrics[i] < cur) metrics[i] = cur;
	}
}

// ---- radix select ----------------------------------------------------------------------------------------------------
// one key of every lane into the workgroup's histogram; a wave whose live keys all carry one digit (the giant tie at 0 of
// a real metric) adds it with one atomic. Called in uniform control flow.
__device__ __forceinline__ void prune_hist_add(uint32_t *s_hist, uint32_t key, bool valid, uint32_t prefix, uint32_t himask, int shift, int lane)
{
	const bool live = valid && ((key ^ prefix) & himask) == 0u;
	const uint32_t d = (key >> shift) & 255u;
	const uint64_t act = __ballot(live);
	if (act == 0) return; // (wave-uniform)
	const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, __builtin_ctzll(act));
	if (__ballot(live && d == d0) == act)
	{
		if (lane == __builtin_ctzll(act)) atomicAdd(&s_hist[d0], (uint32_t)__popcll(act));
	}
	else if (live) atomicAdd(&s_hist[d], 1u);
}

// counts[blockIdx.x][d] = keys of this workgroup's tiles whose digits above `shift` equal those of state[0] and whose
// digit at `shift` is d. Tiles that every thread reads as one 16-byte load go PRUNE_HIST_UNROLL at a time, all loads
// issued before the first key is counted; the last tile, and everything when metrics is not 16-byte aligned, one by one.
template <int DT>
__global__ void __launch_bounds__(256) k_prune_hist(int P, int64_t tiles, int shift, const float *__restrict__ metrics,
	const uint32_t *__restrict__ state, uint32_t *__restrict__ counts, int aligned)
{
	__shared__ uint32_t s_hist[256];
	const int t = threadIdx.x, lane = t & 63;
	s_hist[t] = 0;
	const uint32_t himask = shift < 24 ? ~0u << (shift + 8) : 0u;
	const uint32_t prefix = shift < 24 ? state[0] : 0u;
	const int64_t full_tiles = aligned ? (int64_t)P / PRUNE_TILE : 0;
	__syncthreads();
	for (int64_t tile0 = blockIdx.x; tile0 < tiles; tile0 += (int64_t)gridDim.x * PRUNE_HIST_UNROLL)
	{
		if (tile0 + (int64_t)(PRUNE_HIST_UNROLL - 1) * gridDim.x < full_tiles)
		{
			float4 v[PRUNE_HIST_UNROLL];
#pragma unroll
			for (int u = 0; u < PRUNE_HIST_UNROLL; u++)
				v[u] = *(const float4 *)(metrics + (size_t)(tile0 + (int64_t)u * gridDim.x) * PRUNE_TILE + (size_t)t * PRUNE_PER_THREAD);
#pragma unroll
			for (int u = 0; u < PRUNE_HIST_UNROLL; u++)
			{
				prune_hist_add(s_hist, prune_key_of<DT>(v[u].x), true, prefix, himask, shift, lane);
				prune_hist_add(s_hist, prune_key_of<DT>(v[u].y), true, prefix, himask, shift, lane);
				prune_hist_add(s_hist, prune_key_of<DT>(v[u].z), true, prefix, himask, shift, lane);
				prune_hist_add(s_hist, prune_key_of<DT>(v[u].w), true, prefix, himask, shift, lane);
			}
			continue;
		}
		for (int u = 0; u < PRUNE_HIST_UNROLL; u++)
		{
			const int64_t tile = tile0 + (int64_t)u * gridDim.x;
			if (tile >= tiles) break;
			uint32_t key[PRUNE_PER_THREAD];
			const int n = prune_load_keys<DT>(metrics, (size_t)tile * PRUNE_TILE + (size_t)t * PRUNE_PER_THREAD, (size_t)P, aligned != 0, key);
#pragma unroll
			for (int j = 0; j < PRUNE_PER_THREAD; j++) prune_hist_add(s_hist, key[j], j < n, prefix, himask, shift, lane);
		}
	}
	__syncthreads();
	counts[(size_t)blockIdx.x * 256 + t] = s_hist[t];
}

// One workgroup, thread d = digit d: adds the rows of counts, finds the digit whose run of keys holds rank r (1-based among
// the keys that matched so far; the first pass starts from k) and leaves state = {threshold so far, rank inside that digit}.
__global__ void __launch_bounds__(256) k_prune_pick(int rows, int shift, uint32_t k, const uint32_t *__restrict__ counts, uint32_t *state)
{
	__shared__ uint32_t s_w[4];
	const int t = threadIdx.x;
	const uint32_t prefix = shift < 24 ? state[0] : 0u, r = shift < 24 ? state[1] : k;
	uint32_t sum = 0;
#pragma unroll 32
	for (int w = 0; w < rows; w++) sum += counts[(size_t)w * 256 + t];
	uint32_t tot;
	const uint32_t ex = prune_block_scan(sum, s_w, &tot);
	if (ex < r && r - ex <= sum) { state[0] = prefix | ((uint32_t)t << shift); state[1] = r - ex; }
}

__global__ void __launch_bounds__(256) k_prune_tie_count(int P, const float *__restrict__ metrics, const uint32_t *__restrict__ state,
	uint32_t *__restrict__ tie, int aligned)
{
	__shared__ uint32_t s_w[4];
	const int t = threadIdx.x;
	const uint32_t T = state[0];
	uint32_t key[PRUNE_PER_THREAD];
	const int n = prune_load_keys(metrics, (size_t)blockIdx.x * PRUNE_TILE + (size_t)t * PRUNE_PER_THREAD, (size_t)P, aligned != 0, key);
	uint32_t c = 0;
#pragma unroll
	for (int j = 0; j < PRUNE_PER_THREAD; j++) c += j < n && key[j] == T;
	uint32_t tot;
	prune_block_scan(c, s_w, &tot);
	if (t == 0) tie[blockIdx.x] = tot;
}

// One workgroup: vals[i] -> sum of vals[0 .. i) in place, PRUNE_SCAN_CHUNK tiles per round; *total (optional) gets the sum.
__global__ void __launch_bounds__(256) k_prune_scan(int64_t n, uint32_t *__restrict__ vals, int32_t *__restrict__ total)
{
	__shared__ uint32_t s_w[4];
	uint32_t carry = 0;
	uint32_t next = threadIdx.x < n ? vals[threadIdx.x] : 0u;
	for (int64_t c = 0; c < n; c += PRUNE_SCAN_CHUNK)
	{
		const int64_t i = c + threadIdx.x;
		const uint32_t v = next;
		next = i + PRUNE_SCAN_CHUNK < n ? vals[i + PRUNE_SCAN_CHUNK] : 0u; // (in flight while this round is scanned)
		uint32_t tot;
		const uint32_t ex = prune_block_scan(v, s_w, &tot);
		if (i < n) vals[i] = carry + ex;
		carry += tot;
	}
	if (total && threadIdx.x == 0) *total = (int32_t)carry;
}

// mask[i] = key < T || (key == T && fewer than r rows with key == T come before i)
__global__ void __launch_bounds__(256) k_prune_write(int P, const float *__restrict__ metrics, const uint32_t *__restrict__ state,
	const uint32_t *__restrict__ tie, uint8_t *__restrict__ mask, int aligned, int mask_aligned)
{
	__shared__ uint32_t s_w[4];
	const int t = threadIdx.x;
	const uint32_t T = state[0], r = state[1];
	const size_t i = (size_t)blockIdx.x * PRUNE_TILE + (size_t)t * PRUNE_PER_THREAD;
	uint32_t key[PRUNE_PER_THREAD];
	const int n = prune_load_keys(metrics, i, (size_t)P, aligned != 0, key);
	uint32_t c = 0;
#pragma unroll
	for (int j = 0; j < PRUNE_PER_THREAD; j++) c += j < n && key[j] == T;
	uint32_t tot;
	uint32_t rank = tie[blockIdx.x] + prune_block_scan(c, s_w, &tot);
	uint32_t out = 0;
#pragma unroll
	for (int j = 0; j < PRUNE_PER_THREAD; j++)
	{
		bool take = key[j] < T;
		if (key[j] == T) { take = rank < r; rank++; }
		out |= (uint32_t)(j < n && take) << (8 * j);
	}
	if (n == PRUNE_PER_THREAD && mask_aligned) *(uint32_t *)(mask + i) = out;
	else
		for (int j = 0; j < n; j++) mask[i + j] = (uint8_t)((out >> (8 * j)) & 255u);
}

// ---- compaction ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_compact_count(int P, const uint8_t *__restrict__ mask, int invert, uint32_t *__restrict__ first, int aligned)
{
	__shared__ uint32_t s_w[4];
	const int t = threadIdx.x;
	const uint32_t bits = compact_kept_bits(mask, (size_t)blockIdx.x * PRUNE_TILE + (size_t)t * PRUNE_PER_THREAD, (size_t)P, aligned != 0, invert);
	uint32_t tot;
	prune_block_scan((uint32_t)__popc(bits), s_w, &tot);
	if (t == 0) first[blockIdx.x] = tot;
}

struct CompactTensor { const uint32_t *src; uint32_t *dst; uint32_t row_words, dst_rows; };
struct CompactTable {
	int P, invert, aligned;
	const uint8_t *mask;
	const uint32_t *first;
	CompactTensor t[FR_COMPACT_MAX_TENSORS];
};

// Workgroup (x, y): the kept rows of tile x of tensor y. The tile's kept rows go to LDS in index order; they are
// consecutive in the destination, from row first[x] on, so word e of the tile's output is word e % W of kept row e / W:
// consecutive lanes write consecutive words, and read runs of W consecutive words. A destination row >= dst_rows is not
// written.
__global__ void __launch_bounds__(256) k_compact_rows(const CompactTable p)
{
	__shared__ uint32_t s_w[4];
	__shared__ uint16_t s_rows[PRUNE_TILE];
	const CompactTensor ten = p.t[blockIdx.y];
	const uint32_t W = ten.row_words; // > 0: the launcher leaves zero-width tensors out
	const int t = threadIdx.x;
	const size_t row0 = (size_t)blockIdx.x * PRUNE_TILE;
	const uint32_t bits = compact_kept_bits(p.mask, row0 + (size_t)t * PRUNE_PER_THREAD, (size_t)p.P, p.aligned != 0, p.invert);
	uint32_t n_kept;
	uint32_t at = prune_block_scan((uint32_t)__popc(bits), s_w, &n_kept);
#pragma unroll
	for (int j = 0; j < PRUNE_PER_THREAD; j++)
		if (bits >> j & 1u) s_rows[at++] = (uint16_t)(t * PRUNE_PER_THREAD + j);
	__syncthreads();
	const uint32_t base = p.first[blockIdx.x];
	if (base >= ten.dst_rows) return;
	const uint32_t n_out = min(n_kept, ten.dst_rows - base);
	const uint64_t total = (uint64_t)n_out * W;
	const uint32_t *__restrict__ src = ten.src + row0 * W;
	uint32_t *__restrict__ dst = ten.dst + (size_t)base * W;
	const uint32_t dj = 256u / W, dc = 256u % W; // what 256 words further means in (row, word) terms
	uint32_t j = (uint32_t)t / W, c = (uint32_t)t % W;
	for (uint64_t e = t; e < total; e += 256)
	{
		dst[e] = src[(size_t)s_rows[j] * W + c];
		j += dj; c += dc;
		if (c >= W) { c -= W; j++; }
	}
}

// ---- launchers -------------------------------------------------------------------------------------------------------
static unsigned prune_grid(int P) { const int64_t b = ((int64_t)P + 255) / 256; return (unsigned)(b < 4096 ? b : 4096); }

int launch_prune_metric(int P, int kind, const float *contribs, const int32_t *counts, float *metrics, hipStream_t stream)
{
	if (kind == FR_PRUNE_MAX_COMP_EFFICIENCY)
		hipLaunchKernelGGL(k_prune_metric<FR_PRUNE_MAX_COMP_EFFICIENCY>, dim3(prune_grid(P)), dim3(256), 0, stream, P, contribs, counts, metrics);
	else
		hipLaunchKernelGGL(k_prune_metric<FR_PRUNE_CONTRIB>, dim3(prune_grid(P)), dim3(256), 0, stream, P, contribs, counts, metrics);
	return check_launch("prune_metric", stream, false);
}

// the four radix passes: state = {key of the element of 1-based rank `rank`, that rank inside the run of equal keys}
template <int DT>
static void prune_radix_passes(int P, const PruneLayout &L, const float *values, uint32_t rank, void *ws, hipStream_t stream)
{
	char *base = (char *)ws;
	uint32_t *counts = (uint32_t *)(base + L.hist), *state = (uint32_t *)(base + L.state);
	// a histogram workgroup takes PRUNE_HIST_UNROLL tiles at a time, so that many fewer workgroups than tiles, at most PRUNE_HIST_WGS
	const unsigned tiles = (unsigned)L.tiles, want = (tiles + PRUNE_HIST_UNROLL - 1) / PRUNE_HIST_UNROLL, wgs = want < PRUNE_HIST_WGS ? want : PRUNE_HIST_WGS;
	const int aligned = (uintptr_t)values % 16 == 0;
	for (int shift = 24; shift >= 0; shift -= 8)
	{
		hipLaunchKernelGGL(k_prune_hist<DT>, dim3(wgs), dim3(256), 0, stream, P, L.tiles, shift, values, state, counts, aligned);
		hipLaunchKernelGGL(k_prune_pick, dim3(1), dim3(256), 0, stream, (int)wgs, shift, rank, counts, state);
	}
}

int launch_prune_select(int P, const float *metrics, int64_t k, uint8_t *mask, void *ws, hipStream_t stream)
{
	if (k == 0 || k == P) // nothing or everything: no order needed
	{
		const hipError_t e = hipMemsetAsync(mask, k == 0 ? 0 : 1, (size_t)P, stream);
		if (e != hipSuccess) { set_error("prune_select: %s", hipGetErrorString(e)); return FR_ERR_HIP; }
		return FR_OK;
	}
	const PruneLayout L = prune_layout(P);
	char *base = (char *)ws;
	uint32_t *state = (uint32_t *)(base + L.state), *tie = (uint32_t *)(base + L.tie);
	const unsigned tiles = (unsigned)L.tiles;
	const int aligned = (uintptr_t)metrics % 16 == 0, mask_aligned = (uintptr_t)mask % 4 == 0;
	prune_radix_passes<0>(P, L, metrics, (uint32_t)k, ws, stream);
	int rc = check_launch("prune_select", stream, false);
	if (rc) return rc;
	hipLaunchKernelGGL(k_prune_tie_count, dim3(tiles), dim3(256), 0, stream, P, metrics, state, tie, aligned);
	hipLaunchKernelGGL(k_prune_scan, dim3(1), dim3(256), 0, stream, L.tiles, tie, (int32_t *)nullptr);
	hipLaunchKernelGGL(k_prune_write, dim3(tiles), dim3(256), 0, stream, P, metrics, state, tie, mask, aligned, mask_aligned);
	return check_launch("prune_write", stream, false);
}

// fr_select_kth: the threshold key the four passes leave in state[0], turned back into a value (one thread)
__global__ void k_select_tail(const uint32_t *__restrict__ state, int dtype, uint32_t *__restrict__ kth_out)
{
	const uint32_t key = state[0];
	uint32_t bits;
	if (dtype == 1) bits = key ^ 0x80000000u;
	else if (key == 0xffffffffu) bits = 0x7fc00000u;        // the NaN class: a quiet NaN
	else if (key == 0x80000000u) bits = 0u;                 // the zero class (-0 and +0): +0.0
	else bits = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
	*kth_out = bits;
}

int launch_select_kth(int P, const void *values, int dtype, int64_t k, void *kth_out, void *ws, hipStream_t stream)
{
	const PruneLayout L = prune_layout(P);
	if (dtype == 1) prune_radix_passes<1>(P, L, (const float *)values, (uint32_t)k + 1u, ws, stream);
	else prune_radix_passes<0>(P, L, (const float *)values, (uint32_t)k + 1u, ws, stream);
	hipLaunchKernelGGL(k_select_tail, dim3(1), dim3(1), 0, stream, (const uint32_t *)((const char *)ws + L.state), dtype, (uint32_t *)kth_out);
	return check_launch("select_kth", stream, false);
}

int launch_compact_plan(int P, const uint8_t *mask, int invert, int32_t *count_out, void *ws, hipStream_t stream)
{
	const PruneLayout L = prune_layout(P);
	uint32_t *first = (uint32_t *)((char *)ws + L.first);
	hipLaunchKernelGGL(k_compact_count, dim3((unsigned)L.tiles), dim3(256), 0, stream, P, mask, invert, first, (int)((uintptr_t)mask % 4 == 0));
	hipLaunchKernelGGL(k_prune_scan, dim3(1), dim3(256), 0, stream, L.tiles, first, count_out);
	return check_launch("compact_plan", stream, false);
}

int launch_compact_rows(const fr_compact_args *a, hipStream_t stream)
{
	const PruneLayout L = prune_layout(a->P);
	CompactTable p;
	p.P = a->P; p.invert = a->invert; p.aligned = (uintptr_t)a->mask % 4 == 0;
	p.mask = a->mask;
	p.first = (const uint32_t *)((const char *)a->workspace + L.first);
	int n = 0;
	for (int k = 0; k < a->num_tensors; k++)
	{
		const fr_compact_tensor &t = a->tensors[k];
		if (t.row_words == 0 || t.dst_rows == 0) continue; // zero-width rows and empty destinations: nothing to copy
		p.t[n].src = (const uint32_t *)t.src; p.t[n].dst = (uint32_t *)t.dst;
		p.t[n].row_words = (uint32_t)t.row_words; p.t[n].dst_rows = (uint32_t)t.dst_rows;
		n++;
	}
	if (n == 0) return FR_OK;
	for (int k = n; k < FR_COMPACT_MAX_TENSORS; k++) p.t[k] = CompactTensor{nullptr, nullptr, 0u, 0u};
	hipLaunchKernelGGL(k_compact_rows, dim3((unsigned)L.tiles, (unsigned)n), dim3(256), 0, stream, p);
	return check_launch("compact_rows", stream, false);
}

} // namespace fr
