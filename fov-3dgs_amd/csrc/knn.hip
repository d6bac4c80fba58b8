// fovraster -- simple-knn's distCUDA2: the mean squared distance of every point to its three nearest neighbours, the
// initial scale of GaussianModel.create_from_pcd (fov3dgs/scene/gaussian_model.py:245-267).
//
// Reference (fov3dgs/submodules/simple-knn/simple_knn.cu:185-220, spatial.cu:15-25): CUB reductions for the bounds with
// two blocking copies to the host, a CUB radix sort of 30-bit Morton codes, boxes of 1024 consecutive sorted points, and
// a search in which every point tests all P / 1024 boxes (quadratic in P), with cudaMalloc / thrust temporaries per call.
//
// Contract (include/fovraster.h): out[i] = ((b0 + b1) + b2) / 3 where b0 <= b1 <= b2 are the three smallest
// d(i, j) = (dx*dx + dy*dy) + dz*dz over j != i, missing neighbours counting as FLT_MAX. That value does not depend on any
// order, and the search below is exact, so the output is one bit pattern per input.
//
// Kernels, all on the caller's stream, no atomics outside LDS, no host round trip:
//   k_knn_bounds      partial min / max rows, one per workgroup (<= 256 rows)
//   k_knn_morton      folds the rows, writes 30-bit Morton keys (10 bits per axis, clamped: NaN or a zero extent -> 0)
//                     and the digit histogram of the first radix pass
//   k_knn_hist / k_knn_scan / k_knn_scatter
//                     LSD radix sort, 4 x 8 bits, stable: per-tile LDS histograms, a [digit][tile] scan, a scatter that
//                     ranks keys inside a wave with ballots; the last pass writes the sorted points as float4 (w = index)
//   k_knn_leaf_boxes / k_knn_node_boxes
//                     an implicit 64-ary tree over the sorted order: a leaf is 64 consecutive points, a node the box of 64
//                     children, up to the first level of <= 64 nodes
//   k_knn_search      one wave per leaf: the 64 lanes are 64 spatially coherent queries that walk the tree together
#include "common.h"
#include <cfloat>

// the pair distance and the box bound must round exactly as written: no contraction into fma, whatever the build flags
#pragma clang fp contract(off)

namespace fr {

#define KNN_TILE 4096      // keys per workgroup of the radix passes: 4 waves x 16 rounds x 64 lanes
#define KNN_ROUNDS 16
#define KNN_BND_ROWS 256   // most partial-bounds rows k_knn_bounds writes (k_knn_morton folds them with one thread each)
#define KNN_MAX_LEVELS 6   // ceil(2^31 / 64) = 2^25 leaves -> 2^19 -> 2^13 -> 128 -> 2: five levels for any int32 P

struct KnnLayout {
	size_t bytes;
	size_t bounds, counts, totals, x, b; // byte offsets; x: keys / values of passes 0-2, then the sorted float4 points
	size_t boxes;                        // float4 pairs (lo, hi) of every tree node, level by level
	int64_t tiles, rows;
	int levels;
	int64_t level_n[KNN_MAX_LEVELS], level_off[KNN_MAX_LEVELS]; // nodes per level and their first node in `boxes`
};

static size_t knn_align(size_t x) { return (x + 255) & ~(size_t)255; }

static KnnLayout knn_layout(int64_t P)
{
	KnnLayout L{};
	L.tiles = (P + KNN_TILE - 1) / KNN_TILE;
	L.rows = L.tiles < KNN_BND_ROWS ? L.tiles : KNN_BND_ROWS;
	int64_t n = (P + 63) / 64, nodes = 0;
	L.levels = 0;
	while (true)
	{
		L.level_n[L.levels] = n;
		L.level_off[L.levels] = nodes;
		nodes += n;
		L.levels++;
		if (n <= 64) break;
		n = (n + 63) / 64;
	}
	size_t o = 0;
	L.bounds = o; o = knn_align(o + (size_t)L.rows * 8 * sizeof(float));
	L.counts = o; o = knn_align(o + (size_t)256 * L.tiles * sizeof(uint32_t));
	L.totals = o; o = knn_align(o + 256 * sizeof(uint32_t));
	L.x = o;      o = knn_align(o + (size_t)P * 16);
	L.b = o;      o = knn_align(o + (size_t)P * 8);
	L.boxes = o;  o = knn_align(o + (size_t)nodes * 32);
	L.bytes = o;
	return L;
}

size_t knn_workspace_bytes(int P) { return P > 0 ? knn_layout(P).bytes : 0; }

// ---- wave / block helpers --------------------------------------------------------------------------------------------
__device__ __forceinline__ float knn_wave_min(float v)
{
#pragma unroll
	for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o));
	return v;
}
__device__ __forceinline__ float knn_wave_max(float v)
{
#pragma unroll
	for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
	return v;
}

// exclusive prefix sum over the 256 threads of a workgroup (s_w: 4 words of LDS); *total gets the sum
__device__ __forceinline__ uint32_t knn_block_scan(uint32_t v, uint32_t *s_w, uint32_t *total)
{
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint32_t inc = v;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1)
	{
		const uint32_t n = __shfl_up(inc, o);
		if (lane >= o) inc += n;
	}
	if (lane == 63) s_w[w] = inc;
	__syncthreads();
	uint32_t pre = 0;
	for (int k = 0; k < w; k++) pre += s_w[k];
	*total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
	__syncthreads();
	return pre + inc - v;
}

__device__ __forceinline__ uint32_t knn_spread10(uint32_t x)
{
	x = (x | (x << 16)) & 0x030000FFu;
	x = (x | (x << 8)) & 0x0300F00Fu;
	x = (x | (x << 4)) & 0x030C30C3u;
	x = (x | (x << 2)) & 0x09249249u;
	return x;
}

// 10-bit cell of one coordinate; a NaN (also 0 / 0 of an axis with zero extent) or anything outside the box is clamped
__device__ __forceinline__ uint32_t knn_cell(float v, float lo, float scale)
{
	return (uint32_t)fminf(fmaxf((v - lo) * scale, 0.0f), 1023.0f);
}

// the pair distance of the contract, in its order
__device__ __forceinline__ float knn_dist(float4 q, float4 p)
{
	const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
	return (dx * dx + dy * dy) + dz * dz;
}

// branch-free insertion into b0 <= b1 <= b2 of d when `take` and d < b2; otherwise +inf goes through the min / max chain,
// which leaves the three values as they are (no NaN ever reaches fminf / fmaxf: a NaN d fails d < b2)
__device__ __forceinline__ void knn_insert(float d, bool take, float &b0, float &b1, float &b2)
{
	d = take && d < b2 ? d : __builtin_inff();
	b2 = fminf(b2, fmaxf(b1, d));
	b1 = fminf(b1, fmaxf(b0, d));
	b0 = fminf(b0, d);
}

// ---- bounds ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_knn_bounds(int P, const float *__restrict__ pts, float *__restrict__ rows)
{
	__shared__ float s_r[4][6];
	float v[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * 256)
	{
#pragma unroll
		for (int k = 0; k < 3; k++)
		{
			const float c = pts[3 * i + k];
			v[k] = fminf(v[k], c);
			v[3 + k] = fmaxf(v[3 + k], c);
		}
	}
#pragma unroll
	for (int k = 0; k < 3; k++) { v[k] = knn_wave_min(v[k]); v[3 + k] = knn_wave_max(v[3 + k]); }
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	if (lane == 0)
	{
#pragma unroll
		for (int k = 0; k < 6; k++) s_r[w][k] = v[k];
	}
	__syncthreads();
	if (threadIdx.x < 6)
	{
		const int k = threadIdx.x;
		float r = s_r[0][k];
		for (int j = 1; j < 4; j++) r = k < 3 ? fminf(r, s_r[j][k]) : fmaxf(r, s_r[j][k]);
		rows[(size_t)blockIdx.x * 8 + k] = r;
	}
}

// ---- Morton keys + the first pass's histogram ------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_knn_morton(int P, int nrows, int64_t tiles, const float *__restrict__ pts,
	const float *__restrict__ rows, uint32_t *__restrict__ keys, uint32_t *__restrict__ counts)
{
	__shared__ float s_r[4][6];
	__shared__ float s_box[6];
	__shared__ uint32_t s_hist[256];
	const int t = threadIdx.x, lane = t & 63, w = t >> 6;
	s_hist[t] = 0;
	float v[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
	if (t < nrows)
	{
#pragma unroll
		for (int k = 0; k < 6; k++) v[k] = rows[(size_t)t * 8 + k];
	}
#pragma unroll
	for (int k = 0; k < 3; k++) { v[k] = knn_wave_min(v[k]); v[3 + k] = knn_wave_max(v[3 + k]); }
	if (lane == 0)
	{
#pragma unroll
		for (int k = 0; k < 6; k++) s_r[w][k] = v[k];
	}
	__syncthreads();
	if (t < 6)
	{
		float r = s_r[0][t];
		for (int j = 1; j < 4; j++) r = t < 3 ? fminf(r, s_r[j][t]) : fmaxf(r, s_r[j][t]);
		s_box[t] = r;
	}
	__syncthreads();
	float lo[3], scale[3];
#pragma unroll
	for (int k = 0; k < 3; k++) { lo[k] = s_box[k]; scale[k] = 1024.0f / (s_box[3 + k] - s_box[k]); }
	const size_t base = (size_t)blockIdx.x * KNN_TILE;
#pragma unroll 4
	for (int r = 0; r < KNN_ROUNDS; r++)
	{
		const size_t i = base + (size_t)r * 256 + t;
		if (i < (size_t)P)
		{
			const uint32_t key = knn_spread10(knn_cell(pts[3 * i], lo[0], scale[0])) | (knn_spread10(knn_cell(pts[3 * i + 1], lo[1], scale[1])) << 1)
				| (knn_spread10(knn_cell(pts[3 * i + 2], lo[2], scale[2])) << 2);
			keys[i] = key;
			atomicAdd(&s_hist[key & 255], 1u);
		}
	}
	__syncthreads();
	counts[(size_t)t * tiles + blockIdx.x] = s_hist[t];
}

// ---- radix sort ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_knn_hist(int P, int64_t tiles, int shift, const uint32_t *__restrict__ keys, uint32_t *__restrict__ counts)
{
	__shared__ uint32_t s_hist[256];
	const int t = threadIdx.x;
	s_hist[t] = 0;
	__syncthreads();
	const size_t base = (size_t)blockIdx.x * KNN_TILE;
#pragma unroll 4
	for (int r = 0; r < KNN_ROUNDS; r++)
	{
		const size_t i = base + (size_t)r * 256 + t;
		if (i < (size_t)P) atomicAdd(&s_hist[(keys[i] >> shift) & 255], 1u);
	}
	__syncthreads();
	counts[(size_t)t * tiles + blockIdx.x] = s_hist[t];
}

// one workgroup per digit: counts[d][tile] -> exclusive prefix over the tiles, totals[d] = the digit's count
__global__ void __launch_bounds__(256) k_knn_scan(int64_t tiles, uint32_t *__restrict__ counts, uint32_t *__restrict__ totals)
{
	__shared__ uint32_t s_w[4];
	uint32_t *row = counts + (size_t)blockIdx.x * tiles;
	uint32_t carry = 0;
	for (int64_t c = 0; c < tiles; c += 256)
	{
		const int64_t i = c + threadIdx.x;
		const uint32_t v = i < tiles ? row[i] : 0;
		uint32_t tot;
		const uint32_t ex = knn_block_scan(v, s_w, &tot);
		if (i < tiles) row[i] = carry + ex;
		carry += tot;
	}
	if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

enum { KNN_PASS_FIRST = 0, KNN_PASS_MID = 1, KNN_PASS_LAST = 2 };

// Stable scatter of one 8-bit digit. Wave w of the workgroup owns keys [w * 1024, (w + 1) * 1024) of the tile and ranks
// them in 16 rounds of 64: equal digits within a round are found with 8 ballots, the wave's running count per digit sits
// in LDS. FIRST: values are the key positions (no value array yet). LAST: writes sorted[pos] = (x, y, z, index bits).
template <int MODE>
__global__ void __launch_bounds__(256) k_knn_scatter(int P, int64_t tiles, int shift, const uint32_t *__restrict__ keys_in,
	const uint32_t *__restrict__ vals_in, uint32_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out,
	const float *__restrict__ pts, float4 *__restrict__ sorted, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ totals)
{
	__shared__ uint32_t s_cnt[4][256];
	__shared__ uint32_t s_w[4];
	const int t = threadIdx.x, lane = t & 63, w = t >> 6;
	uint32_t tot;
	const uint32_t digit_base = knn_block_scan(totals[t], s_w, &tot) + counts[(size_t)t * tiles + blockIdx.x];
#pragma unroll
	for (int k = 0; k < 4; k++) s_cnt[k][t] = 0;
	__syncthreads();

	const size_t i0 = (size_t)blockIdx.x * KNN_TILE + (size_t)w * (KNN_ROUNDS * 64) + lane;
	const uint64_t lt = (1ull << lane) - 1;
	uint32_t key[KNN_ROUNDS], val[KNN_ROUNDS], rank[KNN_ROUNDS];
#pragma unroll
	for (int r = 0; r < KNN_ROUNDS; r++)
	{
		const size_t i = i0 + (size_t)r * 64;
		const bool valid = i < (size_t)P;
		const uint32_t k = valid ? keys_in[i] : 0u;
		key[r] = k;
		val[r] = MODE == KNN_PASS_FIRST ? (uint32_t)i : (valid ? vals_in[i] : 0u);
		const uint32_t d = (k >> shift) & 255;
		uint64_t m = __ballot(valid);
#pragma unroll
		for (int b = 0; b < 8; b++)
		{
			const bool bit = (d >> b) & 1;
			const uint64_t bb = __ballot(bit);
			m &= bit ? bb : ~bb;
		}
		const uint32_t c = s_cnt[w][d];
		rank[r] = c + (uint32_t)__popcll(m & lt);
		FR_WAVE_LDS_SYNC();
		if (valid && lane == 63 - __clzll(m)) s_cnt[w][d] = c + (uint32_t)__popcll(m);
		FR_WAVE_LDS_SYNC();
	}
	__syncthreads();
	uint32_t run = digit_base;
#pragma unroll
	for (int k = 0; k < 4; k++) { const uint32_t c = s_cnt[k][t]; s_cnt[k][t] = run; run += c; }
	__syncthreads();
#pragma unroll
	for (int r = 0; r < KNN_ROUNDS; r++)
	{
		const size_t i = i0 + (size_t)r * 64;
		if (i >= (size_t)P) continue;
		const uint32_t pos = s_cnt[w][(key[r] >> shift) & 255] + rank[r];
		if (pos >= (uint32_t)P) continue; // cannot happen (the counts are the same keys'); keeps a bad workspace in bounds
		if (MODE == KNN_PASS_LAST)
		{
			const size_t j = val[r];
			sorted[pos] = make_float4(pts[3 * j], pts[3 * j + 1], pts[3 * j + 2], __uint_as_float(val[r]));
		}
		else
		{
			keys_out[pos] = key[r];
			vals_out[pos] = val[r];
		}
	}
}

// ---- the tree --------------------------------------------------------------------------------------------------------
// boxes[2 n] = (lo.xyz, 0), boxes[2 n + 1] = (hi.xyz, 0); a box without points is (+inf, -inf), which no bound passes
__global__ void __launch_bounds__(256) k_knn_leaf_boxes(int P, int64_t n_leaves, const float4 *__restrict__ sorted, float4 *__restrict__ boxes)
{
	const int lane = threadIdx.x & 63;
	const size_t leaf = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (leaf >= (size_t)n_leaves) return;
	const size_t i = leaf * 64 + lane;
	const float inf = __builtin_inff();
	float4 lo = make_float4(inf, inf, inf, 0.0f), hi = make_float4(-inf, -inf, -inf, 0.0f);
	if (i < (size_t)P) { const float4 p = sorted[i]; lo = make_float4(p.x, p.y, p.z, 0.0f); hi = lo; }
	lo.x = knn_wave_min(lo.x); lo.y = knn_wave_min(lo.y); lo.z = knn_wave_min(lo.z);
	hi.x = knn_wave_max(hi.x); hi.y = knn_wave_max(hi.y); hi.z = knn_wave_max(hi.z);
	if (lane == 0) { boxes[2 * leaf] = lo; boxes[2 * leaf + 1] = hi; }
}

__global__ void __launch_bounds__(256) k_knn_node_boxes(int64_t n_child, int64_t n_node, const float4 *__restrict__ child, float4 *__restrict__ node)
{
	const int lane = threadIdx.x & 63;
	const size_t n = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (n >= (size_t)n_node) return;
	const size_t c = n * 64 + lane;
	const float inf = __builtin_inff();
	float4 lo = make_float4(inf, inf, inf, 0.0f), hi = make_float4(-inf, -inf, -inf, 0.0f);
	if (c < (size_t)n_child) { lo = child[2 * c]; hi = child[2 * c + 1]; }
	lo.x = knn_wave_min(lo.x); lo.y = knn_wave_min(lo.y); lo.z = knn_wave_min(lo.z);
	hi.x = knn_wave_max(hi.x); hi.y = knn_wave_max(hi.y); hi.z = knn_wave_max(hi.z);
	if (lane == 0) { node[2 * n] = lo; node[2 * n + 1] = hi; }
}

// ---- the search ------------------------------------------------------------------------------------------------------
// Exactness: the bound of a box is computed in the order of the pair distance, per-axis gap max(0, lo - q, q - hi) then
// (gx*gx + gy*gy) + gz*gz. For a point p in the box, |p.x - q.x| >= gap in exact arithmetic, and fp32 subtraction,
// squaring of non-negative values and addition are monotone under rounding, so the computed bound is <= the computed
// d(q, p) of every point in it. A point changes the three values only if d < b2 (an equal d leaves the same values), and
// b2 never grows, so a box whose bound is >= the current b2 of every lane holds nothing that could change them: the
// search skips only such boxes and returns the same bits as an exhaustive one. (The wave-level filter below uses the gap
// between the box and the box of the wave's queries against the largest b2 of the wave: smaller or equal again, by the
// same monotonicity, so it is a coarser form of the same test.)
__device__ __forceinline__ float knn_gap(float lo, float hi, float q) { return fmaxf(0.0f, fmaxf(lo - q, q - hi)); }
__device__ __forceinline__ float knn_box_bound(float4 lo, float4 hi, float4 q)
{
	const float gx = knn_gap(lo.x, hi.x, q.x), gy = knn_gap(lo.y, hi.y, q.y), gz = knn_gap(lo.z, hi.z, q.z);
	return (gx * gx + gy * gy) + gz * gz;
}
__device__ __forceinline__ float knn_box_box(float4 lo, float4 hi, float4 qlo, float4 qhi)
{
	const float gx = fmaxf(0.0f, fmaxf(lo.x - qhi.x, qlo.x - hi.x)), gy = fmaxf(0.0f, fmaxf(lo.y - qhi.y, qlo.y - hi.y)),
		gz = fmaxf(0.0f, fmaxf(lo.z - qhi.z, qlo.z - hi.z));
	return (gx * gx + gy * gy) + gz * gz;
}

__device__ __forceinline__ uint32_t knn_lane_u32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

// One wave per leaf; 4 waves per workgroup. The descent keeps, per level, the children of the current node still to visit
// as a 64-bit mask and the index of the first child, in lane `level` of three registers (read with readlane, written with
// a select): no stack in memory. Every node is taken at most once, so the loop is bounded by the node count.
__global__ void __launch_bounds__(256) k_knn_search(int P, int levels, const float4 *__restrict__ sorted, const float4 *__restrict__ boxes,
	float *__restrict__ out)
{
	__shared__ float4 s_pts[4][64];
	const int lane = threadIdx.x & 63;
	const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t n_leaves = (uint32_t)(((int64_t)P + 63) / 64);
	const uint32_t leaf = blockIdx.x * 4 + w;
	if (leaf >= n_leaves) return;

	// lane l: nodes of level l and the first of them in `boxes`
	uint32_t lv_n = 0, lv_off = 0;
	{
		uint64_t n = (uint64_t)P, off = 0;
		for (int l = 0; l < KNN_MAX_LEVELS; l++)
		{
			n = (n + 63) / 64;
			if (l == lane) { lv_n = (uint32_t)n; lv_off = (uint32_t)off; }
			off += n;
		}
	}

	const uint32_t first = leaf * 64;
	const int cnt = (int)min((uint32_t)64, (uint32_t)P - first);
	const float4 q = sorted[first + (uint32_t)min(lane, cnt - 1)];
	const bool valid = lane < cnt;
	const bool active = valid && isfinite(q.x) && isfinite(q.y) && isfinite(q.z);
	// an inactive lane starts at -1: no distance is below it, so it neither changes nor asks for a visit
	const float seed = active ? FLT_MAX : -1.0f;
	float b0 = seed, b1 = seed, b2 = seed;

	// the own leaf first (self excluded by sorted position)
	s_pts[w][lane] = q;
	FR_WAVE_LDS_SYNC();
	for (int j = 0; j < cnt; j++) knn_insert(knn_dist(q, s_pts[w][j]), j != lane, b0, b1, b2);
	FR_WAVE_LDS_SYNC();

	const float4 qlo = boxes[2 * (size_t)leaf], qhi = boxes[2 * (size_t)leaf + 1]; // the box of this wave's queries
	const int top = levels - 1;
	uint32_t st_lo = 0, st_hi = 0, st_base = 0;

	// children [base, base + 64) of level cl that the wave-level filter keeps
	auto filter = [&](int cl, uint32_t base) -> uint64_t {
		const float maxb2 = knn_wave_max(b2);
		const uint32_t n_cl = knn_lane_u32(lv_n, cl), off_cl = knn_lane_u32(lv_off, cl);
		const uint32_t c = base + lane;
		const bool ok = c < n_cl && !(cl == 0 && c == leaf);
		bool keep = false;
		if (ok)
		{
			const float4 lo = boxes[2 * (size_t)(off_cl + c)], hi = boxes[2 * (size_t)(off_cl + c) + 1];
			keep = knn_box_box(lo, hi, qlo, qhi) < maxb2;
		}
		return __ballot(keep);
	};

	int lvl = top;
	{
		const uint64_t m = filter(top, 0);
		if (lane == top) { st_lo = (uint32_t)m; st_hi = (uint32_t)(m >> 32); }
	}
	while (true)
	{
		uint64_t m = ((uint64_t)knn_lane_u32(st_hi, lvl) << 32) | knn_lane_u32(st_lo, lvl);
		if (m == 0)
		{
			if (lvl == top) break;
			lvl++;
			continue;
		}
		const uint32_t node = knn_lane_u32(st_base, lvl) + (uint32_t)__builtin_ctzll(m);
		m &= m - 1;
		if (lane == lvl) { st_lo = (uint32_t)m; st_hi = (uint32_t)(m >> 32); }
		const size_t bi = 2 * (size_t)(knn_lane_u32(lv_off, lvl) + node);
		const float4 lo = boxes[bi], hi = boxes[bi + 1];
		if (__ballot(knn_box_bound(lo, hi, q) < b2) == 0) continue;
		if (lvl == 0)
		{
			const uint32_t f = node * 64;
			const int c = (int)min((uint32_t)64, (uint32_t)P - f);
			s_pts[w][lane] = sorted[f + (uint32_t)min(lane, c - 1)];
			FR_WAVE_LDS_SYNC();
			for (int j = 0; j < c; j++) knn_insert(knn_dist(q, s_pts[w][j]), true, b0, b1, b2);
			FR_WAVE_LDS_SYNC();
		}
		else
		{
			const uint32_t base = node * 64;
			const uint64_t cm = filter(lvl - 1, base);
			lvl--;
			if (lane == lvl) { st_lo = (uint32_t)cm; st_hi = (uint32_t)(cm >> 32); st_base = base; }
		}
	}
	if (valid)
	{
		const uint32_t idx = __float_as_uint(q.w);
		if (idx < (uint32_t)P) out[idx] = active ? ((b0 + b1) + b2) / 3.0f : __builtin_nanf("");
	}
}

int launch_knn(int P, const float *pts, float *out, void *ws, hipStream_t stream)
{
	const KnnLayout L = knn_layout(P);
	char *base = (char *)ws;
	float *rows = (float *)(base + L.bounds);
	uint32_t *counts = (uint32_t *)(base + L.counts), *totals = (uint32_t *)(base + L.totals);
	uint32_t *keys_a = (uint32_t *)(base + L.x), *vals_a = keys_a + P;
	uint32_t *keys_b = (uint32_t *)(base + L.b), *vals_b = keys_b + P;
	float4 *sorted = (float4 *)(base + L.x), *boxes = (float4 *)(base + L.boxes);
	const unsigned tiles = (unsigned)L.tiles;

	hipLaunchKernelGGL(k_knn_bounds, dim3((unsigned)L.rows), dim3(256), 0, stream, P, pts, rows);
	hipLaunchKernelGGL(k_knn_morton, dim3(tiles), dim3(256), 0, stream, P, (int)L.rows, L.tiles, pts, rows, keys_a, counts);
	int rc = check_launch("knn_morton", stream, false);
	if (rc) return rc;
	// pass 0: a -> b, 1: b -> a, 2: a -> b, 3: b -> sorted points (over a's storage, no longer read)
	for (int pass = 0; pass < 4; pass++)
	{
		const int shift = 8 * pass;
		const uint32_t *ki = pass & 1 ? keys_b : keys_a, *vi = pass & 1 ? vals_b : vals_a;
		uint32_t *ko = pass & 1 ? keys_a : keys_b, *vo = pass & 1 ? vals_a : vals_b;
		if (pass > 0) hipLaunchKernelGGL(k_knn_hist, dim3(tiles), dim3(256), 0, stream, P, L.tiles, shift, ki, counts);
		hipLaunchKernelGGL(k_knn_scan, dim3(256), dim3(256), 0, stream, L.tiles, counts, totals);
		if (pass == 0)
			hipLaunchKernelGGL(k_knn_scatter<KNN_PASS_FIRST>, dim3(tiles), dim3(256), 0, stream, P, L.tiles, shift, ki, vi, ko, vo, pts, sorted, counts, totals);
		else if (pass < 3)
			hipLaunchKernelGGL(k_knn_scatter<KNN_PASS_MID>, dim3(tiles), dim3(256), 0, stream, P, L.tiles, shift, ki, vi, ko, vo, pts, sorted, counts, totals);
		else
			hipLaunchKernelGGL(k_knn_scatter<KNN_PASS_LAST>, dim3(tiles), dim3(256), 0, stream, P, L.tiles, shift, ki, vi, ko, vo, pts, sorted, counts, totals);
	}
	rc = check_launch("knn_sort", stream, false);
	if (rc) return rc;
	hipLaunchKernelGGL(k_knn_leaf_boxes, dim3((unsigned)((L.level_n[0] + 3) / 4)), dim3(256), 0, stream, P, L.level_n[0], sorted, boxes);
	for (int l = 1; l < L.levels; l++)
		hipLaunchKernelGGL(k_knn_node_boxes, dim3((unsigned)((L.level_n[l] + 3) / 4)), dim3(256), 0, stream, L.level_n[l - 1], L.level_n[l],
			boxes + 2 * L.level_off[l - 1], boxes + 2 * L.level_off[l]);
	hipLaunchKernelGGL(k_knn_search, dim3((unsigned)((L.level_n[0] + 3) / 4)), dim3(256), 0, stream, P, L.levels, sorted, boxes, out);
	return check_launch("knn_search", stream, false);
}

} // namespace fr
