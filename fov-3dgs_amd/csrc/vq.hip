// fovraster -- LightGaussian's VecTree SH vector quantisation (LightGaussian/vectree/vq.py, vectree.py): the nearest-code search
// on the f32 matrix cores, the EMA codebook step, the dead-code replacement and the container's bit packing.
//
// Reference, per training iteration (vq.py:262-299, vectree.py:196-204; n sampled rows, K codes, D = 27 or 48):
//   torch.cdist into n x K, argmax, F.one_hot into an int64 n x K, a cast, a product with the weights, a second n x K x D GEMM
//   against the one-hot matrix only to sum rows per code, two topk and an indexed write. Here the n x K matrix never exists:
//   k_vq_norms        ||e_c||^2, one fmaf chain per code
//   k_vq_search       32 rows per wave held as MFMA A fragments, code slabs of 128 streamed through LDS, x . e on
//                     v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain), score = ||e||^2 - 2 x . e, a running (best, index)
//                     per accumulator register, strict `<` in ascending code order + a lexicographic lane reduction: the lowest
//                     index wins an exact tie
//   k_vq_gather       quantize = embed[ind] (optionally through fp16) and the exact sum (x - e)^2 per row, from the differences
//   k_vq_sum          one workgroup, double, fixed order: sum w, sum cluster_size, the MSE
//   k_vq_rank / colscan / segscan / place    a stable counting sort of the rows by code (ascending row position inside a code):
//                     integer atomics only where one wave owns the counter, so the order is a function of the input
//   k_vq_segsum       one wave per code walks its segment in that order, lanes across D: sum w' x, sum w', the cluster_size EMA
//   k_vq_embed        Laplace smoothing and the embed EMA (a code with no member decays by exactly `decay`)
//   k_vq_select / k_vq_copy   the k smallest cluster sizes and the k largest sampled weights, sorted, ties to the lowest index,
//                     and the row copy (vectree.py:202-204)
//   k_pack_bits / k_unpack_bits   `bits` per value, MSB first: np.packbits of the reference's dec2bin matrix
// No float atomics, no host round trip, nothing allocated: every output is one bit pattern, run after run.
#include "common.h"
#include <hip/hip_fp16.h>
#include <math.h>

#pragma clang fp contract(off)

namespace fr {


#define VQ_SLAB 128        // codes per LDS slab (four 32-code column tiles of two MFMA tiles each)
#define VQ_TILE 1024       // rows per counting-sort tile (one wave walks a tile in order)
#define VQ_MAX_D 64
#define VQ_MAX_K 65536
#define VQ_MAX_EXPIRE 64

struct VqLayout {
	size_t norms, scal, dist2, esum, total, seg, rank, perm, sel, table, bytes;
	int64_t tiles;
};
// scal: double[0] = sum w, double[1] = sum cluster_size, double[2] = sum dist2; float view at +32 bytes: [0] = sum w, [1] = sum cluster_size
static VqLayout vq_layout(int64_t n, int64_t K, int64_t D, int training)
{
	VqLayout L; size_t off = 0;
	L.tiles = (n + VQ_TILE - 1) / VQ_TILE;
	L.norms = off; off = align_up(off + (size_t)K * 4);
	L.scal = off; off = align_up(off + 64);
	L.dist2 = off; off = align_up(off + (size_t)n * 4);
	L.esum = L.total = L.seg = L.rank = L.perm = L.sel = L.table = off;
	if (training)
	{
		L.esum = off; off = align_up(off + (size_t)K * D * 4);
		L.total = off; off = align_up(off + (size_t)K * 4);
		L.seg = off; off = align_up(off + (size_t)(K + 1) * 4);
		L.rank = off; off = align_up(off + (size_t)n * 4);
		L.perm = off; off = align_up(off + (size_t)n * 4);
		L.sel = off; off = align_up(off + 2 * VQ_MAX_EXPIRE * 4);
		L.table = off; off = align_up(off + (size_t)L.tiles * K * 4);
	}
	L.bytes = off + 256;
	return L;
}

// the rows of a call: row i of the input is feats[rows[i]] (rows: int32 or int64, or null: feats[i]); N = rows of feats, and an index
// outside 0 .. N-1 is clamped into it (nothing is ever read out of bounds; the Python layer validates what it is handed)
struct VqRows { const void *rows; int rows64; int64_t N; };
__device__ __forceinline__ int64_t vq_src(const VqRows R, int64_t i)
{
	int64_t s = i;
	if (R.rows) s = R.rows64 ? ((const int64_t *)R.rows)[i] : (int64_t)((const int32_t *)R.rows)[i];
	return s < 0 ? 0 : (s >= R.N ? R.N - 1 : s);
}

// ---- nearest code ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_vq_norms(int K, int D, const float *__restrict__ embed, float *__restrict__ norms)
{
	const int c = blockIdx.x * 256 + threadIdx.x;
	if (c >= K) return;
	float s = 0.0f;
	for (int d = 0; d < D; d++) { const float e = embed[(size_t)c * D + d]; s = fmaf(e, e, s); }
	norms[c] = s;
}

// NS k-steps of 2 (NS even: the instruction takes 4): D <= 2 NS, zero-padded (fma(0, 0, c) = c: the padding is exact). A wave's 32 rows
// are two 16-row tiles, a 32-code column tile two 16-code tiles: four independent accumulators (the shape's 40-cycle dependent
// latency against its 32-cycle issue). Measured against the 32x32x2 shape (one accumulator of 16 registers per 32 x 32 tile,
// tools/scratch/vq_mfma32.patch, tools/vq_bench.py --alt-lib): same indices; all 6 M rows 1.4-2 % faster beyond the spread in both
// sessions, the 80 000-row search within +-5 % with the sign changing between sessions (VecTree).
typedef float vq_f32x4 __attribute__((ext_vector_type(4)));
template <int NS>
__global__ void __launch_bounds__(256) k_vq_search(int64_t n, int K, int D, const float *__restrict__ feats, const VqRows R, const float *__restrict__ embed, const float *__restrict__ norms, int32_t *__restrict__ ind)
{
	constexpr int DP = 2 * NS, LD = DP + 1, N4 = NS / 2;
	static_assert(NS % 2 == 0, "k steps of 4");
	__shared__ float es[VQ_SLAB * LD];
	__shared__ float en[VQ_SLAB];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int r = lane & 15, h = lane >> 4;
	const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
	// A fragments: lane l holds x[row l & 15][k = 4 s + (l >> 4)] of step s, for both row tiles
	float a[2][N4];
#pragma unroll
	for (int rt = 0; rt < 2; rt++)
	{
		const int64_t i = row0 + rt * 16 + r;
		const float *xr = nullptr;
		if (i < n) xr = feats + vq_src(R, i) * D;
#pragma unroll
		for (int s = 0; s < N4; s++) { const int d = 4 * s + h; a[rt][s] = (xr && d < D) ? xr[d] : 0.0f; }
	}
	float best[2][4]; int bidx[2][4];
#pragma unroll
	for (int rt = 0; rt < 2; rt++)
#pragma unroll
		for (int q = 0; q < 4; q++) { best[rt][q] = INFINITY; bidx[rt][q] = 0; }
	for (int c0 = 0; c0 < K; c0 += VQ_SLAB)
	{
		__syncthreads();
		for (int t = threadIdx.x; t < VQ_SLAB * DP; t += 256)
		{
			const int c = t / DP, d = t % DP;
			float v = 0.0f;
			if (c0 + c < K && d < D) v = embed[(size_t)(c0 + c) * D + d];
			es[c * LD + d] = v;
		}
		if (threadIdx.x < VQ_SLAB) en[threadIdx.x] = c0 + (int)threadIdx.x < K ? norms[c0 + threadIdx.x] : INFINITY;
		__syncthreads();
		const int left = K - c0;
		const int nsub = left >= VQ_SLAB ? VQ_SLAB / 32 : (left + 31) / 32;
		for (int sub = 0; sub < nsub; sub++)
		{
			vq_f32x4 acc[2][2];
#pragma unroll
			for (int rt = 0; rt < 2; rt++)
#pragma unroll
				for (int ct = 0; ct < 2; ct++)
#pragma unroll
					for (int q = 0; q < 4; q++) acc[rt][ct][q] = 0.0f;
			const float *eb = es + (sub * 32 + r) * LD + h;
#pragma unroll
			for (int s = 0; s < N4; s++)
			{
				const float b0 = eb[4 * s], b1 = eb[16 * LD + 4 * s];
				acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][s], b0, acc[0][0], 0, 0, 0);
				acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][s], b0, acc[1][0], 0, 0, 0);
				acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][s], b1, acc[0][1], 0, 0, 0);
				acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][s], b1, acc[1][1], 0, 0, 0);
			}
			// C: column (code) = l & 15, row = 4 (l >> 4) + q
#pragma unroll
			for (int ct = 0; ct < 2; ct++)
			{
				const int code = c0 + sub * 32 + ct * 16 + r;
				const float nn = en[sub * 32 + ct * 16 + r];
#pragma unroll
				for (int rt = 0; rt < 2; rt++)
#pragma unroll
					for (int q = 0; q < 4; q++)
					{
						const float sc = nn - 2.0f * acc[rt][ct][q];
						if (sc < best[rt][q]) { best[rt][q] = sc; bidx[rt][q] = code; }
					}
			}
		}
	}
#pragma unroll
	for (int rt = 0; rt < 2; rt++)
#pragma unroll
		for (int q = 0; q < 4; q++)
		{
			float b = best[rt][q]; int bi = bidx[rt][q];
#pragma unroll
			for (int m = 1; m < 16; m <<= 1)
			{
				const float ob = __shfl_xor(b, m); const int oi = __shfl_xor(bi, m);
				if (ob < b || (ob == b && oi < bi)) { b = ob; bi = oi; }
			}
			const int64_t i = row0 + rt * 16 + 4 * h + q;
			if (r == 0 && i < n) ind[i] = bi < K ? bi : K - 1;
		}
}

// ---- gather, distance ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float vq_wave_sum(float v)
{
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
	return v;
}

__global__ void __launch_bounds__(256) k_vq_gather(int64_t n, int K, int D, const float *__restrict__ feats, const VqRows R, const float *__restrict__ embed, const int32_t *__restrict__ ind, int to_half, float *__restrict__ quantize, float *__restrict__ dist2)
{
	const int lane = threadIdx.x & 63;
	const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (i >= n) return;
	int c = ind[i];
	if ((unsigned)c >= (unsigned)K) c = 0;
	float v = 0.0f;
	if (lane < D)
	{
		const float e = embed[(size_t)c * D + lane];
		if (feats) { const float diff = feats[vq_src(R, i) * D + lane] - e; v = diff * diff; }
		if (quantize) quantize[i * D + lane] = to_half ? __half2float(__float2half(e)) : e;
	}
	if (dist2) { v = vq_wave_sum(v); if (lane == 0) dist2[i] = v; }
}

// one workgroup: the sum of n floats in double, in a fixed order. outf[0] = float(sum * scale)
__global__ void __launch_bounds__(1024) k_vq_sum(int64_t n, const float *__restrict__ v, const VqRows R, double scale,
	double *__restrict__ outd, float *__restrict__ outf)
{
	__shared__ double sh[1024];
	double s = 0.0;
#pragma unroll 8
	for (int64_t i = threadIdx.x; i < n; i += 1024) s += (double)v[vq_src(R, i)]; // (independent loads: several in flight)
	sh[threadIdx.x] = s;
	__syncthreads();
	for (int m = 512; m >= 1; m >>= 1)
	{
		if ((int)threadIdx.x < m) sh[threadIdx.x] += sh[threadIdx.x + m];
		__syncthreads();
	}
	if (threadIdx.x == 0) { if (outd) outd[0] = sh[0]; if (outf) outf[0] = (float)(sh[0] * scale); }
}

// ---- stable counting sort of the rows by code --------------------------------------------------------------------------
// One wave per tile of VQ_TILE rows, 64 rows at a time in order: rank[i] = rows of the same code earlier in the tile. table[t][c]
// is touched by tile t's wave alone, and the returned value is used (stored) before the next group's atomic is issued.
__global__ void __launch_bounds__(256) k_vq_rank(int64_t n, int K, const int32_t *__restrict__ ind, uint32_t *__restrict__ table, uint32_t *__restrict__ rank)
{
	const int lane = threadIdx.x & 63;
	const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	const int64_t lo = t * VQ_TILE;
	if (lo >= n) return;
	for (int g = 0; g < VQ_TILE / 64; g++)
	{
		const int64_t i = lo + g * 64 + lane;
		int c = -1;
		if (i < n) { c = ind[i]; if ((unsigned)c >= (unsigned)K) c = 0; }
		int before = 0, total = 0, leader = lane;
		for (int j = 63; j >= 0; j--)
		{
			const int cj = __shfl(c, j);
			if (cj == c) { total++; leader = j; if (j < lane) before++; }
		}
		uint32_t base = 0;
		if (c >= 0 && leader == lane) base = atomicAdd(&table[(size_t)t * K + c], (uint32_t)total);
		base = __shfl(base, leader);
		if (c >= 0) rank[i] = base + before;
	}
}

// per code: the tile counts become exclusive running sums over the tiles; total[c] = rows of code c
__global__ void __launch_bounds__(256) k_vq_colscan(int64_t tiles, int K, uint32_t *__restrict__ table, uint32_t *__restrict__ total)
{
	const int c = blockIdx.x * 256 + threadIdx.x;
	if (c >= K) return;
	uint32_t run = 0;
	for (int64_t t = 0; t < tiles; t++) { const uint32_t v = table[(size_t)t * K + c]; table[(size_t)t * K + c] = run; run += v; }
	total[c] = run;
}

// one workgroup: seg[c] = sum of total[< c], seg[K] = n
__global__ void __launch_bounds__(1024) k_vq_segscan(int K, const uint32_t *__restrict__ total, uint32_t *__restrict__ seg)
{
	__shared__ uint32_t sh[1024];
	const int per = (K + 1023) / 1024;
	const int lo = threadIdx.x * per, hi = min(K, lo + per);
	uint32_t s = 0;
	for (int c = lo; c < hi; c++) s += total[c];
	sh[threadIdx.x] = s;
	__syncthreads();
	if (threadIdx.x == 0) { uint32_t run = 0; for (int t = 0; t < 1024; t++) { const uint32_t v = sh[t]; sh[t] = run; run += v; } seg[K] = run; }
	__syncthreads();
	uint32_t run = sh[threadIdx.x];
	for (int c = lo; c < hi; c++) { seg[c] = run; run += total[c]; }
}

__global__ void __launch_bounds__(256) k_vq_place(int64_t n, int K, const int32_t *__restrict__ ind, const uint32_t *__restrict__ rank,
	const uint32_t *__restrict__ table, const uint32_t *__restrict__ seg, uint32_t *__restrict__ perm)
{
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	int c = ind[i];
	if ((unsigned)c >= (unsigned)K) c = 0;
	const uint64_t p = (uint64_t)seg[c] + table[(size_t)(i / VQ_TILE) * K + c] + rank[i];
	if (p < (uint64_t)n) perm[p] = (uint32_t)i;
}

// ---- the EMA step ----------------------------------------------------------------------------------------------------
// One wave per code, lanes across D, the segment walked in ascending row position: embed_sum[c] = sum w' x, batch = sum w',
// cluster_size[c] = cluster_size[c] decay + (1 - decay) batch (vq.py:285-294, ema_inplace). w' = w n / sum w (vq.py:264), 1 without weights.
__global__ void __launch_bounds__(256) k_vq_segsum(int64_t n, int K, int D, const float *__restrict__ feats, const VqRows R,
	const float *__restrict__ weights, const float *__restrict__ sum_w, const uint32_t *__restrict__ seg, const uint32_t *__restrict__ perm,
	float decay, float one_minus_decay, float *__restrict__ esum, float *__restrict__ cluster_size)
{
	const int lane = threadIdx.x & 63;
	const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (c >= K) return;
	const uint32_t s = seg[c], e = min(seg[c + 1], (uint32_t)n);
	const float nf = (float)n, sw = weights ? sum_w[0] : 1.0f;
	float acc = 0.0f, bs = 0.0f;
	for (uint32_t base = s; base < e; base += 64)
	{
		const int cnt = (int)min(64u, e - base);
		int src = 0; float w = 1.0f;
		if (lane < cnt)
		{
			uint32_t i = perm[base + lane];
			if (i >= (uint32_t)n) i = 0;
			src = (int)vq_src(R, i);
			if (weights) w = (weights[src] * nf) / sw;
		}
		for (int j = 0; j < cnt; j++)
		{
			const int sj = __shfl(src, j); const float wj = __shfl(w, j);
			const float x = lane < D ? feats[(size_t)sj * D + lane] : 0.0f;
			acc = acc + wj * x;
			bs = bs + wj;
		}
	}
	if (lane < D) esum[(size_t)c * D + lane] = acc;
	if (lane == 0) { const float cs = cluster_size[c] * decay; cluster_size[c] = cs + one_minus_decay * bs; }
}

// smoothed = (cs + eps) / (S + K eps) * S (laplace_smoothing x sum, vq.py:296); embed = embed decay + (1 - decay) esum / smoothed
__global__ void __launch_bounds__(256) k_vq_embed(int K, int D, const float *__restrict__ esum, const float *__restrict__ cluster_size,
	const float *__restrict__ sum_cs, float eps, float k_eps, float decay, float one_minus_decay, float *__restrict__ embed)
{
	const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= (int64_t)K * D) return;
	const int c = (int)(t / D);
	const float S = sum_cs[0];
	const float smoothed = ((cluster_size[c] + eps) / (S + k_eps)) * S;
	const float e = embed[t] * decay;
	embed[t] = e + one_minus_decay * (esum[t] / smoothed);
}

// ---- replacement -----------------------------------------------------------------------------------------------------
// block 0: the k smallest cluster sizes, ascending; block 1: the k largest sampled weights, descending; ties to the lowest index.
// Round t takes the least (key, index) above round t - 1's.
__global__ void __launch_bounds__(1024) k_vq_select(int64_t n, int K, int k, const float *__restrict__ cluster_size, const float *__restrict__ weights,
	const VqRows R, int32_t *__restrict__ sel)
{
	__shared__ float shk[1024];
	__shared__ int shi[1024];
	const bool largest = blockIdx.x == 1;
	const int64_t count = largest ? n : K;
	float pkey = -INFINITY; int pidx = -1;
	for (int t = 0; t < k; t++)
	{
		float bk = INFINITY; int bi = 0x7fffffff;
#pragma unroll 8
		for (int64_t i = threadIdx.x; i < count; i += 1024)
		{
			const float key = largest ? -(weights ? weights[vq_src(R, i)] : 1.0f) : cluster_size[i];
			const bool above = key > pkey || (key == pkey && (int)i > pidx);
			if (above && (key < bk || (key == bk && (int)i < bi))) { bk = key; bi = (int)i; }
		}
		shk[threadIdx.x] = bk; shi[threadIdx.x] = bi;
		__syncthreads();
		for (int m = 512; m >= 1; m >>= 1)
		{
			if ((int)threadIdx.x < m)
			{
				const float ok = shk[threadIdx.x + m]; const int oi = shi[threadIdx.x + m];
				if (ok < shk[threadIdx.x] || (ok == shk[threadIdx.x] && oi < shi[threadIdx.x])) { shk[threadIdx.x] = ok; shi[threadIdx.x] = oi; }
			}
			__syncthreads();
		}
		pkey = shk[0]; pidx = shi[0];
		__syncthreads();
		if (threadIdx.x == 0) sel[(largest ? VQ_MAX_EXPIRE : 0) + t] = pidx < count ? pidx : 0; // (nothing left above: NaN keys)
	}
}

__global__ void __launch_bounds__(64) k_vq_copy(int D, const float *__restrict__ feats, const VqRows R,
	const int32_t *__restrict__ sel, float *__restrict__ embed)
{
	const int t = blockIdx.x, d = threadIdx.x;
	if (d >= D) return;
	embed[(size_t)sel[t] * D + d] = feats[vq_src(R, sel[VQ_MAX_EXPIRE + t]) * D + d];
}

// ---- bits ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pack_bits(int64_t count, int bits, const int32_t *__restrict__ values, uint8_t *__restrict__ out)
{
	const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
	const int64_t nbits = count * bits;
	if (b * 8 >= nbits) return;
	uint32_t byte = 0;
	for (int q = 0; q < 8; q++)
	{
		const int64_t p = b * 8 + q;
		uint32_t bit = 0;
		if (p < nbits) { const int64_t v = p / bits; const int j = (int)(p % bits); bit = ((uint32_t)values[v] >> (bits - 1 - j)) & 1u; }
		byte = byte << 1 | bit;
	}
	out[b] = (uint8_t)byte;
}

__global__ void __launch_bounds__(256) k_unpack_bits(int64_t count, int bits, const uint8_t *__restrict__ in, int32_t *__restrict__ values)
{
	const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (v >= count) return;
	uint32_t x = 0;
	for (int j = 0; j < bits; j++) { const int64_t p = v * bits + j; x = x << 1 | ((in[p >> 3] >> (7 - (int)(p & 7))) & 1u); }
	values[v] = (int32_t)x;
}

// ---- launchers -------------------------------------------------------------------------------------------------------
static int vq_check_shape(const char *what, int64_t n, int K, int D)
{
	if (n < 0 || n > 2147483647LL) { set_error("%s: bad size n=%lld", what, (long long)n); return FR_ERR_INVALID; }
	if (K < 1 || K > VQ_MAX_K) { set_error("%s: K=%d is not in 1..%d", what, K, VQ_MAX_K); return FR_ERR_INVALID; }
	if (D < 1 || D > VQ_MAX_D) { set_error("%s: D=%d is not in 1..%d", what, D, VQ_MAX_D); return FR_ERR_INVALID; }
	return FR_OK;
}
static int vq_check_ws(const char *what, const void *ws)
{
	if (!ws) { set_error("%s: a required pointer is null", what); return FR_ERR_INVALID; }
	if ((uintptr_t)ws % 16) { set_error("%s: the vq workspace must be 16-byte aligned", what); return FR_ERR_INVALID; }
	return FR_OK;
}
static unsigned vq_grid(int64_t items, int per) { return (unsigned)((items + per - 1) / per); }

} // namespace fr

using namespace fr;

extern "C" {

size_t fr_vq_workspace_bytes(int64_t n, int32_t K, int32_t D, int32_t training)
{
	if (n < 0 || n > 2147483647LL || K < 1 || K > VQ_MAX_K || D < 1 || D > VQ_MAX_D) return 0;
	return vq_layout(n, K, D, training).bytes;
}

int fr_vq_nearest(int64_t n, int32_t K, int32_t D, const float *feats, int64_t N, const void *rows, int32_t rows64, const float *embed, int32_t *ind,
	void *workspace, void *stream)
{
	int rc = vq_check_shape("vq_nearest", n, K, D);
	if (rc) return rc;
	if (n > 0 && (N < 1 || N > 2147483647LL || (!rows && N < n))) { set_error("vq_nearest: N=%lld rows of feats for n=%lld", (long long)N, (long long)n); return FR_ERR_INVALID; }
	const VqRows R{rows, rows64 != 0, N};
	if (n == 0) return FR_OK;
	if (!feats || !embed || !ind) { set_error("vq_nearest: a required pointer is null"); return FR_ERR_INVALID; }
	if ((rc = vq_check_ws("vq_nearest", workspace))) return rc;
	const VqLayout L = vq_layout(n, K, D, 0);
	float *norms = (float *)((char *)workspace + L.norms);
	hipStream_t s = (hipStream_t)stream;
	hipLaunchKernelGGL(k_vq_norms, dim3(vq_grid(K, 256)), dim3(256), 0, s, K, D, embed, norms);
	const dim3 grid(vq_grid(n, 128));
#define VQ_SEARCH(NS) hipLaunchKernelGGL(k_vq_search<NS>, grid, dim3(256), 0, s, n, K, D, feats, R, embed, norms, ind)
	if (D <= 4) VQ_SEARCH(2);
	else if (D <= 16) VQ_SEARCH(8);
	else if (D <= 28) VQ_SEARCH(14);
	else if (D <= 48) VQ_SEARCH(24);
	else VQ_SEARCH(32);
#undef VQ_SEARCH
	return check_launch("vq_nearest", s, false);
}

int fr_vq_gather(int64_t n, int32_t K, int32_t D, const float *feats, int64_t N, const void *rows, int32_t rows64, const float *embed, const int32_t *ind,
	int32_t to_half, float *quantize, float *dist2, float *loss, float loss_weight, void *workspace, void *stream)
{
	int rc = vq_check_shape("vq_gather", n, K, D);
	if (rc) return rc;
	if (n > 0 && (N < 1 || N > 2147483647LL || (!rows && N < n))) { set_error("vq_gather: N=%lld rows of feats for n=%lld", (long long)N, (long long)n); return FR_ERR_INVALID; }
	const VqRows R{rows, rows64 != 0, N};
	if (n == 0) return FR_OK;
	if (!embed || !ind) { set_error("vq_gather: a required pointer is null"); return FR_ERR_INVALID; }
	if ((dist2 || loss) && !feats) { set_error("vq_gather: distances need feats"); return FR_ERR_INVALID; }
	if (!quantize && !dist2 && !loss) return FR_OK;
	hipStream_t s = (hipStream_t)stream;
	float *d2 = dist2;
	char *ws = (char *)workspace;
	VqLayout L = vq_layout(n, K, D, 0);
	if (loss)
	{
		if ((rc = vq_check_ws("vq_gather", workspace))) return rc;
		if (!d2) d2 = (float *)(ws + L.dist2);
	}
	hipLaunchKernelGGL(k_vq_gather, dim3(vq_grid(n, 4)), dim3(256), 0, s, n, K, D, feats, R, embed, ind, to_half, quantize, d2);
	if (loss)
		hipLaunchKernelGGL(k_vq_sum, dim3(1), dim3(1024), 0, s, n, (const float *)d2, VqRows{nullptr, 0, n},
			(double)loss_weight / ((double)n * (double)D), (double *)(ws + L.scal) + 2, loss);
	return check_launch("vq_gather", s, false);
}

int fr_vq_update(int64_t n, int32_t K, int32_t D, const float *feats, int64_t N, const void *rows, int32_t rows64, const float *weights, const int32_t *ind,
	float decay, float eps, float *embed, float *cluster_size, void *workspace, void *stream)
{
	int rc = vq_check_shape("vq_update", n, K, D);
	if (rc) return rc;
	if (n > 0 && (N < 1 || N > 2147483647LL || (!rows && N < n))) { set_error("vq_update: N=%lld rows of feats for n=%lld", (long long)N, (long long)n); return FR_ERR_INVALID; }
	const VqRows R{rows, rows64 != 0, N};
	if (n == 0) { set_error("vq_update: no rows"); return FR_ERR_INVALID; }
	if (!feats || !ind || !embed || !cluster_size) { set_error("vq_update: a required pointer is null"); return FR_ERR_INVALID; }
	if ((rc = vq_check_ws("vq_update", workspace))) return rc;
	if (!(decay >= 0.0f && decay <= 1.0f)) { set_error("vq_update: decay=%g is not in 0..1", (double)decay); return FR_ERR_INVALID; }
	const VqLayout L = vq_layout(n, K, D, 1);
	char *ws = (char *)workspace;
	hipStream_t s = (hipStream_t)stream;
	double *scal = (double *)(ws + L.scal);
	float *scalf = (float *)(ws + L.scal + 32);
	uint32_t *table = (uint32_t *)(ws + L.table), *total = (uint32_t *)(ws + L.total), *seg = (uint32_t *)(ws + L.seg);
	uint32_t *rank = (uint32_t *)(ws + L.rank), *perm = (uint32_t *)(ws + L.perm);
	float *esum = (float *)(ws + L.esum);
	const float omd = (float)(1.0 - (double)decay);
	if (hipMemsetAsync(table, 0, (size_t)L.tiles * K * 4, s) != hipSuccess) { set_error("vq_update: memset failed"); return FR_ERR_HIP; }
	if (weights) hipLaunchKernelGGL(k_vq_sum, dim3(1), dim3(1024), 0, s, n, weights, R, 1.0, scal, scalf);
	hipLaunchKernelGGL(k_vq_rank, dim3(vq_grid(L.tiles, 4)), dim3(256), 0, s, n, K, ind, table, rank);
	hipLaunchKernelGGL(k_vq_colscan, dim3(vq_grid(K, 256)), dim3(256), 0, s, L.tiles, K, table, total);
	hipLaunchKernelGGL(k_vq_segscan, dim3(1), dim3(1024), 0, s, K, (const uint32_t *)total, seg);
	hipLaunchKernelGGL(k_vq_place, dim3(vq_grid(n, 256)), dim3(256), 0, s, n, K, ind, (const uint32_t *)rank, (const uint32_t *)table, (const uint32_t *)seg, perm);
	hipLaunchKernelGGL(k_vq_segsum, dim3(vq_grid(K, 4)), dim3(256), 0, s, n, K, D, feats, R, weights, (const float *)scalf,
		(const uint32_t *)seg, (const uint32_t *)perm, decay, omd, esum, cluster_size);
	hipLaunchKernelGGL(k_vq_sum, dim3(1), dim3(1024), 0, s, (int64_t)K, (const float *)cluster_size, VqRows{nullptr, 0, (int64_t)K}, 1.0, scal + 1, scalf + 1);
	hipLaunchKernelGGL(k_vq_embed, dim3(vq_grid((int64_t)K * D, 256)), dim3(256), 0, s, K, D, (const float *)esum, (const float *)cluster_size,
		(const float *)(scalf + 1), eps, (float)((double)K * (double)eps), decay, omd, embed);
	return check_launch("vq_update", s, false);
}

int fr_vq_replace(int64_t n, int32_t K, int32_t D, int32_t k, const float *feats, int64_t N, const void *rows, int32_t rows64, const float *weights,
	float *embed, const float *cluster_size, void *workspace, void *stream)
{
	int rc = vq_check_shape("vq_replace", n, K, D);
	if (rc) return rc;
	if (n > 0 && (N < 1 || N > 2147483647LL || (!rows && N < n))) { set_error("vq_replace: N=%lld rows of feats for n=%lld", (long long)N, (long long)n); return FR_ERR_INVALID; }
	const VqRows R{rows, rows64 != 0, N};
	if (k < 0 || k > VQ_MAX_EXPIRE || k > K || k > n) { set_error("vq_replace: k=%d is not in 0..min(%d, K, n)", k, VQ_MAX_EXPIRE); return FR_ERR_INVALID; }
	if (k == 0) return FR_OK;
	if (!feats || !embed || !cluster_size) { set_error("vq_replace: a required pointer is null"); return FR_ERR_INVALID; }
	if ((rc = vq_check_ws("vq_replace", workspace))) return rc;
	const VqLayout L = vq_layout(n, K, D, 1);
	int32_t *sel = (int32_t *)((char *)workspace + L.sel);
	hipStream_t s = (hipStream_t)stream;
	hipLaunchKernelGGL(k_vq_select, dim3(2), dim3(1024), 0, s, n, K, k, cluster_size, weights, R, sel);
	hipLaunchKernelGGL(k_vq_copy, dim3(k), dim3(64), 0, s, D, feats, R, (const int32_t *)sel, embed);
	return check_launch("vq_replace", s, false);
}

static int bits_check(const char *what, int64_t count, int32_t bits, const void *a, const void *b)
{
	if (count < 0 || count > (1LL << 40)) { set_error("%s: bad count %lld", what, (long long)count); return FR_ERR_INVALID; }
	if (bits < 1 || bits > 16) { set_error("%s: bits=%d is not in 1..16", what, bits); return FR_ERR_INVALID; }
	if (count > 0 && (!a || !b)) { set_error("%s: a required pointer is null", what); return FR_ERR_INVALID; }
	return FR_OK;
}

int fr_pack_bits(int64_t count, int32_t bits, const int32_t *values, uint8_t *out, void *stream)
{
	const int rc = bits_check("pack_bits", count, bits, values, out);
	if (rc || count == 0) return rc;
	const int64_t bytes = (count * bits + 7) / 8;
	hipLaunchKernelGGL(k_pack_bits, dim3(vq_grid(bytes, 256)), dim3(256), 0, (hipStream_t)stream, count, bits, values, out);
	return check_launch("pack_bits", (hipStream_t)stream, false);
}

int fr_unpack_bits(int64_t count, int32_t bits, const uint8_t *in, int32_t *values, void *stream)
{
	const int rc = bits_check("unpack_bits", count, bits, in, values);
	if (rc || count == 0) return rc;
	hipLaunchKernelGGL(k_unpack_bits, dim3(vq_grid(count, 256)), dim3(256), 0, (hipStream_t)stream, count, bits, in, values);
	return check_launch("unpack_bits", (hipStream_t)stream, false);
}

} // extern "C"
