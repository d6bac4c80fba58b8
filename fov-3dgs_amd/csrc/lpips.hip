// fovraster -- LPIPS (VGG16, version 0.1), the fourth quality figure of the reference's tables, with the network's weights as
// inputs: nothing is downloaded, nothing is rebuilt per call, and the activations live in a caller-owned workspace.
//
// Reference behaviour (fov3dgs/lpipsPyTorch, the same files under LightGaussian/lpipsPyTorch):
//   __init__.py:6-21            lpips(x, y, net_type, version) builds LPIPS(net_type, version) -- the torchvision VGG16 and both
//                               weight downloads -- for every picture pair.
//   modules/networks.py:41-51   z_score: (x - mean) / std, mean = (-.030, -.088, -.188), std = (.458, .448, .450), applied to the
//                               picture as it is handed in (the scripts pass [0, 1] pictures; no rescaling to [-1, 1]).
//   modules/networks.py:53-64   forward: the layers in order, the outputs of layers 4, 9, 16, 23, 30 (counted from 1: relu1_2,
//                               relu2_2, relu3_3, relu4_3, relu5_3, the maps in front of the pools) through normalize_activation.
//   modules/networks.py:89-96   VGG16: vgg16().features (13 3x3 convolutions, padding 1, bias, ReLU; channels 3-64-64 | 128-128 |
//                               256 x3 | 512 x3 | 512 x3; a 2x2 stride-2 max pool behind the first four groups, flooring odd sizes).
//   modules/utils.py:6-8        normalize_activation: a / (sqrt(sum_c a_c^2) + 1e-10).
//   modules/lpips.py:30-36      forward: d = sum_c w_c (n(fx)_c - n(fy)_c)^2 (the 1x1 `lin` convolution), its mean over H x W per
//                               tap, and torch.sum(torch.cat(res, 0), 0, True): ONE [1,1,1,1] value, the sum over the five taps
//                               AND over the batch (the scripts pass N = 1). That quirk is kept.
// Here:
//   fr_lpips_pack_weights   a host routine, once per criterion: the 13 OIHW weights into the slabs k_lpips_conv copies to LDS.
//   k_lpips_conv0           3 -> 64, K = 27, plain fmaf chains, the z-score applied on load (padding is zero AFTER the z-score).
//   k_lpips_conv            3x3 convolution + bias + ReLU as an implicit GEMM in exact f32 on v_mfma_f32_16x16x4_f32: a workgroup
//                           owns 16 x 16 pixels x 64 output channels, K runs over (8-channel chunk, tap, channel); per chunk the
//                           18 x 18 halo tile and the 9 x 8 x 64 weight slab are staged in LDS (28 800 bytes), each wave holds
//                           4 pixel rows x 4 channel tiles = 16 independent accumulators. Every output is a k-ordered chain per
//                           chunk and the chunks' sums in chunk order: no split K across workgroups, no atomics.
//   k_lpips_head            ONE pass over a tap of both pictures: both channel norms, the weighted squared difference, the
//                           workgroup's sum in a fixed order, AND the 2x2 max pool of both maps (chosen: the tap is read once).
//                           The difference is expanded, sum w ax^2 / nx^2 - 2 sum w ax ay / (nx ny) + sum w ay^2 / ny^2, so that no
//                           activation is kept or read twice; the five sums are exact products added in double, which leaves the
//                           cancellation ~1e-13 of a term (a float expansion would lose the value), and equal pictures give
//                           q - 2 q + q = 0 exactly.
//   k_lpips_finish          one workgroup, double, fixed order (as k_quality_finish): the tap's value into its slot, the running
//                           total into the call's scalar.
// Activations are kept as [image][C / 8][H][W][8] (x's pictures, then y's): a chunk of a halo row is one contiguous run, and a
// lane's four accumulator registers are one 16-byte store. Two buffers ping-pong; tap k's head runs before its buffer is reused.
#include "common.h"
#include <math.h>
#include <string.h>

#pragma clang fp contract(off)

namespace fr {

#define LP_LAYERS 13
#define LP_TAPS 5
#define LP_TILE 16                       // pixels per workgroup tile edge (k_lpips_conv)
#define LP_HALO (LP_TILE + 2)
#define LP_NPIX (LP_HALO * LP_HALO)      // 324 halo pixels
#define LP_SLAB (9 * 2 * 64 * 4)         // floats of one weight slab: [tap][channel group of 4][64 outputs][4 channels]
#define LP_HEAD_W 32                     // pixels across a head workgroup (4 waves of 8), 2 rows
#define LP_MAX_N 512
#define LP_MAX_HW 16384

static const int lp_cin[LP_LAYERS] = { 3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512 };
static const int lp_cout[LP_LAYERS] = { 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512 };
static const int lp_tap_layer[LP_TAPS] = { 1, 3, 6, 9, 12 }; // the convolution whose output is tap k (relu1_2 .. relu5_3)
static const int lp_tap_c[LP_TAPS] = { 64, 128, 256, 512, 512 };

// packed weights, in floats: per layer its weights then its bias, then the five lin vectors
struct LpPacked { size_t w[LP_LAYERS], b[LP_LAYERS], lin[LP_TAPS], floats; };
static LpPacked lp_packed()
{
	LpPacked P; size_t off = 0;
	for (int l = 0; l < LP_LAYERS; l++)
	{
		P.w[l] = off; off += (size_t)9 * lp_cin[l] * lp_cout[l];
		P.b[l] = off; off += lp_cout[l];
	}
	for (int k = 0; k < LP_TAPS; k++) { P.lin[k] = off; off += lp_tap_c[k]; }
	P.floats = off;
	return P;
}

struct LpWorkspace { size_t scal, partials, buf[2], bytes; size_t buf_floats; long long head_blocks; };
static long long lp_head_blocks(int H, int W) { return (long long)((W + LP_HEAD_W - 1) / LP_HEAD_W) * ((H + 1) / 2); }
static LpWorkspace lp_workspace(int N, int H, int W)
{
	LpWorkspace L; size_t off = 0;
	L.head_blocks = lp_head_blocks(H, W); // the first tap has the most
	L.scal = off; off = align_up(off + 64);
	L.partials = off; off = align_up(off + (size_t)N * L.head_blocks * sizeof(double));
	L.buf_floats = (size_t)2 * N * 64 * H * W; // relu1_1 / relu1_2 of both pictures: the largest maps
	L.buf[0] = off; off = align_up(off + L.buf_floats * 4);
	L.buf[1] = off; off = align_up(off + L.buf_floats * 4);
	L.bytes = off;
	return L;
}

static bool lp_sizes_ok(int N, int H, int W) { return N >= 1 && N <= LP_MAX_N && H >= 16 && W >= 16 && H <= LP_MAX_HW && W <= LP_MAX_HW; }

// ---- first layer: 3 -> 64, z-score on load --------------------------------------------------------------------------------
// x: [N,3,H,W] planes. One thread per pixel and block of 8 outputs; w: [27][64] (k = 9 ci + 3 ky + kx), b: [64].
__global__ void __launch_bounds__(256) k_lpips_conv0(int H, int W, const float *__restrict__ x, int img0, const float *__restrict__ w,
	const float *__restrict__ b, float *__restrict__ out)
{
	__shared__ float sw[27][8], sb[8];
	const int cb = blockIdx.y, n = blockIdx.z;
	if (threadIdx.x < 27 * 8) sw[threadIdx.x >> 3][threadIdx.x & 7] = w[(threadIdx.x >> 3) * 64 + cb * 8 + (threadIdx.x & 7)];
	if (threadIdx.x < 8) sb[threadIdx.x] = b[cb * 8 + threadIdx.x];
	__syncthreads();
	const size_t plane = (size_t)H * W;
	const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (p >= plane) return;
	const int py = (int)(p / W), px = (int)(p - (size_t)py * W);
	const float mean[3] = { -.030f, -.088f, -.188f }, sd[3] = { .458f, .448f, .450f };
	float acc[8];
#pragma unroll
	for (int j = 0; j < 8; j++) acc[j] = 0.0f;
#pragma unroll
	for (int ci = 0; ci < 3; ci++)
	{
		const float *X = x + ((size_t)n * 3 + ci) * plane;
#pragma unroll
		for (int ky = 0; ky < 3; ky++)
#pragma unroll
			for (int kx = 0; kx < 3; kx++)
			{
				const int gy = py + ky - 1, gx = px + kx - 1;
				float z = 0.0f;
				if (gy >= 0 && gy < H && gx >= 0 && gx < W) z = (X[(size_t)gy * W + gx] - mean[ci]) / sd[ci];
#pragma unroll
				for (int j = 0; j < 8; j++) acc[j] = fmaf(z, sw[ci * 9 + ky * 3 + kx][j], acc[j]);
			}
	}
	float4 o0, o1;
	o0.x = fmaxf(acc[0] + sb[0], 0.0f); o0.y = fmaxf(acc[1] + sb[1], 0.0f); o0.z = fmaxf(acc[2] + sb[2], 0.0f); o0.w = fmaxf(acc[3] + sb[3], 0.0f);
	o1.x = fmaxf(acc[4] + sb[4], 0.0f); o1.y = fmaxf(acc[5] + sb[5], 0.0f); o1.z = fmaxf(acc[6] + sb[6], 0.0f); o1.w = fmaxf(acc[7] + sb[7], 0.0f);
	float4 *O = (float4 *)(out + (((size_t)(img0 + n) * 8 + cb) * plane + p) * 8);
	O[0] = o0; O[1] = o1;
}

// ---- 3x3 convolution + bias + ReLU, implicit GEMM on the f32 matrix cores ----------------------------------------------------
// in: [images][Cin / 8][H][W][8], out: [images][Cout / 8][H][W][8]; wp: [Cout / 64][Cin / 8] slabs of LP_SLAB floats.
// grid (tiles across, tiles down, images * Cout / 64). The MFMA's A operand is the weights (row = output channel l & 15, k = l >> 4),
// its B operand the pixels (k = l >> 4, column = pixel l & 15 of a row of the tile): lane l then holds D[row 4 (l >> 4) + q][column
// l & 15], four consecutive output channels of one pixel. Both operands are read from LDS as 64 consecutive words (no bank conflict).
typedef float lp_f32x4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) k_lpips_conv(int H, int W, int Cin, int Cout, const float *__restrict__ in, const float *__restrict__ wp,
	const float *__restrict__ bias, float *__restrict__ out)
{
	__shared__ __attribute__((aligned(16))) float wl[LP_SLAB];
	__shared__ __attribute__((aligned(16))) float il[2 * LP_NPIX * 4];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int r16 = lane & 15, h = lane >> 4;
	const int cob = Cout >> 6, cib = Cin >> 3;
	const int img = blockIdx.z / cob, ob = blockIdx.z - img * cob;
	const int tx0 = blockIdx.x * LP_TILE, ty0 = blockIdx.y * LP_TILE;
	const size_t plane = (size_t)H * W;
	// [output-channel tile][pixel row of this wave]. Two levels: a chunk's 72 products are one MFMA chain from zero, the chunks'
	// sums are added in chunk order. One chain over K = 4608 would carry ~0.4 ulp sqrt(K) of rounding into every output, layer upon
	// layer; chains of 72 and then K / 72 addends carry sqrt(72 + K / 72) instead, a sixth of it.
	lp_f32x4 tot[4][4];
#pragma unroll
	for (int mt = 0; mt < 4; mt++)
#pragma unroll
		for (int r = 0; r < 4; r++)
#pragma unroll
			for (int q = 0; q < 4; q++) tot[mt][r][q] = 0.0f;
	for (int ck = 0; ck < cib; ck++)
	{
		lp_f32x4 acc[4][4];
#pragma unroll
		for (int mt = 0; mt < 4; mt++)
#pragma unroll
			for (int r = 0; r < 4; r++)
#pragma unroll
				for (int q = 0; q < 4; q++) acc[mt][r][q] = 0.0f;
		__syncthreads(); // the previous chunk's reads are done
		const float4 *slab = (const float4 *)(wp + ((size_t)ob * cib + ck) * LP_SLAB);
		for (int i = threadIdx.x; i < LP_SLAB / 4; i += 256) ((float4 *)wl)[i] = slab[i];
		const float *base = in + ((size_t)img * cib + ck) * plane * 8;
		for (int i = threadIdx.x; i < 2 * LP_NPIX; i += 256)
		{
			const int pix = i >> 1, cg = i & 1;
			const int py = pix / LP_HALO, px = pix - py * LP_HALO;
			const int gy = ty0 + py - 1, gx = tx0 + px - 1;
			float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
			if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *(const float4 *)(base + ((size_t)gy * W + gx) * 8 + 4 * cg);
			((float4 *)il)[cg * LP_NPIX + pix] = v;
		}
		__syncthreads();
#pragma unroll
		for (int dy = 0; dy < 3; dy++)
#pragma unroll
			for (int dx = 0; dx < 3; dx++)
#pragma unroll
				for (int cg = 0; cg < 2; cg++)
				{
					const float *wa = wl + (((dy * 3 + dx) * 2 + cg) * 64 + r16) * 4 + h;
					const float *ib = il + (cg * LP_NPIX + (wave * 4 + dy) * LP_HALO + r16 + dx) * 4 + h;
					float a[4], b[4];
#pragma unroll
					for (int mt = 0; mt < 4; mt++) a[mt] = wa[mt * 64];
#pragma unroll
					for (int r = 0; r < 4; r++) b[r] = ib[r * LP_HALO * 4];
#pragma unroll
					for (int mt = 0; mt < 4; mt++)
#pragma unroll
						for (int r = 0; r < 4; r++)
							acc[mt][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[r], acc[mt][r], 0, 0, 0);
				}
#pragma unroll
		for (int mt = 0; mt < 4; mt++)
#pragma unroll
			for (int r = 0; r < 4; r++) tot[mt][r] += acc[mt][r];
	}
	const int gx = tx0 + r16;
	if (gx >= W) return;
#pragma unroll
	for (int mt = 0; mt < 4; mt++)
	{
		const int co = ob * 64 + mt * 16 + 4 * h; // this lane's four consecutive output channels
		const float4 bv = *(const float4 *)(bias + co);
#pragma unroll
		for (int r = 0; r < 4; r++)
		{
			const int gy = ty0 + wave * 4 + r;
			if (gy >= H) continue;
			float4 o;
			o.x = fmaxf(tot[mt][r][0] + bv.x, 0.0f); o.y = fmaxf(tot[mt][r][1] + bv.y, 0.0f);
			o.z = fmaxf(tot[mt][r][2] + bv.z, 0.0f); o.w = fmaxf(tot[mt][r][3] + bv.w, 0.0f);
			*(float4 *)(out + (((size_t)img * (Cout >> 3) + (co >> 3)) * plane + (size_t)gy * W + gx) * 8 + (co & 7)) = o;
		}
	}
}

// ---- head: norms, weighted squared difference, sum; 2x2 max pool of both maps ----------------------------------------------
// feat: [2 N][C / 8][H][W][8], x's pictures then y's. A wave owns 2 rows x 8 pixels (four pool windows); lane = half + 2 xx + 16 r +
// 32 par holds the channels 4 half .. 4 half + 3 of the blocks par, par + 2, ... of pixel (2 qy + r, x0 + xx): 8 pixels x 32 bytes of
// a row and block are one 256-byte run. pooled (optional): [2 N][C / 8][H / 2][W / 2][8]. features (optional): x's tap, [N,C,H,W].
// partials[n * gridDim.y * gridDim.x + block] = the sum of d over the block's pixels, waves added in wave order.
__global__ void __launch_bounds__(256) k_lpips_head(int N, int C, int H, int W, const float *__restrict__ feat, const float *__restrict__ lin,
	float *__restrict__ pooled, float *__restrict__ features, double *__restrict__ partials)
{
	__shared__ double s_w[4];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int half = lane & 1, xx = (lane >> 1) & 7, r = (lane >> 4) & 1, par = lane >> 5;
	const int n = blockIdx.z, CB = C >> 3;
	const int gy = 2 * blockIdx.y + r, gx = blockIdx.x * LP_HEAD_W + wave * 8 + xx;
	const bool in = gy < H && gx < W;
	const int Hp = H >> 1, Wp = W >> 1;
	const bool pool_out = pooled != nullptr && r == 0 && (xx & 1) == 0 && (int)blockIdx.y < Hp && (gx >> 1) < Wp;
	const size_t plane = (size_t)H * W, pplane = (size_t)Hp * Wp;
	const size_t pix = (size_t)gy * W + gx, ppix = (size_t)blockIdx.y * Wp + (gx >> 1);
	double sxx = 0.0, syy = 0.0, wxx = 0.0, wyy = 0.0, wxy = 0.0;
	for (int cb = par; cb < CB; cb += 2)
	{
		float4 ax = make_float4(0.0f, 0.0f, 0.0f, 0.0f), ay = ax;
		if (in)
		{
			ax = *(const float4 *)(feat + (((size_t)n * CB + cb) * plane + pix) * 8 + 4 * half);
			ay = *(const float4 *)(feat + (((size_t)(N + n) * CB + cb) * plane + pix) * 8 + 4 * half);
		}
		const float4 wv = *(const float4 *)(lin + cb * 8 + 4 * half);
		const float xa[4] = { ax.x, ax.y, ax.z, ax.w }, ya[4] = { ay.x, ay.y, ay.z, ay.w }, wa[4] = { wv.x, wv.y, wv.z, wv.w };
#pragma unroll
		for (int j = 0; j < 4; j++)
		{
			const double a = (double)xa[j], b = (double)ya[j], wj = (double)wa[j];
			const double aa = a * a, bb = b * b, ab = a * b; // exact: 24 x 24 bits
			sxx += aa; syy += bb; wxx += wj * aa; wyy += wj * bb; wxy += wj * ab;
		}
		if (features != nullptr && in)
		{
			float *F = features + ((size_t)n * C + cb * 8 + 4 * half) * plane + pix;
			F[0] = ax.x; F[plane] = ax.y; F[2 * plane] = ax.z; F[3 * plane] = ax.w;
		}
		if (pooled != nullptr) // uniform: every lane takes part in the exchanges
		{
			float mx[4], my[4];
#pragma unroll
			for (int j = 0; j < 4; j++)
			{
				mx[j] = fmaxf(xa[j], __shfl_xor(xa[j], 2)); my[j] = fmaxf(ya[j], __shfl_xor(ya[j], 2));
				mx[j] = fmaxf(mx[j], __shfl_xor(mx[j], 16)); my[j] = fmaxf(my[j], __shfl_xor(my[j], 16));
			}
			if (pool_out)
			{
				*(float4 *)(pooled + (((size_t)n * CB + cb) * pplane + ppix) * 8 + 4 * half) = make_float4(mx[0], mx[1], mx[2], mx[3]);
				*(float4 *)(pooled + (((size_t)(N + n) * CB + cb) * pplane + ppix) * 8 + 4 * half) = make_float4(my[0], my[1], my[2], my[3]);
			}
		}
	}
	// the pixel's five sums: the two halves, then the two block parities
	sxx += __shfl_xor(sxx, 1); syy += __shfl_xor(syy, 1); wxx += __shfl_xor(wxx, 1); wyy += __shfl_xor(wyy, 1); wxy += __shfl_xor(wxy, 1);
	sxx += __shfl_xor(sxx, 32); syy += __shfl_xor(syy, 32); wxx += __shfl_xor(wxx, 32); wyy += __shfl_xor(wyy, 32); wxy += __shfl_xor(wxy, 32);
	const double nx = sqrt(sxx) + 1e-10, ny = sqrt(syy) + 1e-10;
	const double q1 = wxx / (nx * nx), q2 = wxy / (nx * ny), q3 = wyy / (ny * ny);
	double d = in ? (q1 - 2.0 * q2) + q3 : 0.0; // equal pictures: q - 2 q + q = 0 exactly
	// the wave's 16 pixels (every lane of a pixel holds the same d)
	d += __shfl_xor(d, 2); d += __shfl_xor(d, 4); d += __shfl_xor(d, 8); d += __shfl_xor(d, 16);
	if (lane == 0) s_w[wave] = d;
	__syncthreads();
	if (threadIdx.x == 0)
		partials[((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// one workgroup: value = (sum of the partials, in double, a fixed order) / (H W) -- the tap's mean summed over the batch.
// scal[0] = the call's running total (tap 0 starts it); out_taps[k] (optional) and out[0] as floats.
__global__ void __launch_bounds__(1024) k_lpips_finish(long long count, double hw, int k, const double *__restrict__ partials, double *__restrict__ scal,
	float *__restrict__ out_taps, float *__restrict__ out)
{
	__shared__ double s[1024];
	double a = 0.0;
	for (long long i = threadIdx.x; i < count; i += 1024) a += partials[i];
	s[threadIdx.x] = a;
	__syncthreads();
	for (int off = 512; off > 0; off >>= 1)
	{
		if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
		__syncthreads();
	}
	if (threadIdx.x == 0)
	{
		const double v = s[0] / hw;
		const double total = k == 0 ? v : scal[0] + v;
		scal[0] = total;
		if (out_taps != nullptr) out_taps[k] = (float)v;
		out[0] = (float)total;
	}
}

} // namespace fr

using namespace fr;

extern "C" size_t fr_lpips_packed_bytes(void)
{
	return lp_packed().floats * sizeof(float);
}

extern "C" int fr_lpips_pack_weights(const float *const *conv_weights, const float *const *conv_biases, const float *const *lin_weights, void *packed)
{
	if (!conv_weights) { set_error("lpips_pack_weights: conv_weights is null"); return FR_ERR_INVALID; }
	if (!conv_biases) { set_error("lpips_pack_weights: conv_biases is null"); return FR_ERR_INVALID; }
	if (!lin_weights) { set_error("lpips_pack_weights: lin_weights is null"); return FR_ERR_INVALID; }
	if (!packed) { set_error("lpips_pack_weights: packed is null"); return FR_ERR_INVALID; }
	for (int l = 0; l < LP_LAYERS; l++)
	{
		if (!conv_weights[l]) { set_error("lpips_pack_weights: conv_weights[%d] is null", l); return FR_ERR_INVALID; }
		if (!conv_biases[l]) { set_error("lpips_pack_weights: conv_biases[%d] is null", l); return FR_ERR_INVALID; }
	}
	for (int k = 0; k < LP_TAPS; k++)
		if (!lin_weights[k]) { set_error("lpips_pack_weights: lin_weights[%d] is null", k); return FR_ERR_INVALID; }
	const LpPacked P = lp_packed();
	float *out = (float *)packed;
	// first layer: [27][64], k = 9 ci + 3 ky + kx (the OIHW order of one output's weights)
	for (int co = 0; co < 64; co++)
		for (int k = 0; k < 27; k++) out[P.w[0] + (size_t)k * 64 + co] = conv_weights[0][co * 27 + k];
	for (int l = 1; l < LP_LAYERS; l++)
	{
		const int ci_n = lp_cin[l], cib = ci_n / 8;
		const float *w = conv_weights[l];
		float *o = out + P.w[l];
		for (int co = 0; co < lp_cout[l]; co++)
			for (int ci = 0; ci < ci_n; ci++)
				for (int t = 0; t < 9; t++)
				{
					const size_t slab = (size_t)(co / 64) * cib + ci / 8;
					const int cg = (ci & 7) >> 2, hh = ci & 3;
					o[slab * LP_SLAB + ((size_t)(t * 2 + cg) * 64 + (co & 63)) * 4 + hh] = w[((size_t)co * ci_n + ci) * 9 + t];
				}
	}
	for (int l = 0; l < LP_LAYERS; l++) memcpy(out + P.b[l], conv_biases[l], (size_t)lp_cout[l] * sizeof(float));
	for (int k = 0; k < LP_TAPS; k++) memcpy(out + P.lin[k], lin_weights[k], (size_t)lp_tap_c[k] * sizeof(float));
	return FR_OK;
}

extern "C" int64_t fr_lpips_workspace_bytes(int32_t N, int32_t H, int32_t W)
{
	if (!lp_sizes_ok(N, H, W))
	{
		set_error("lpips_workspace_bytes: bad sizes N=%d H=%d W=%d (N 1 .. %d, H and W 16 .. %d)", N, H, W, LP_MAX_N, LP_MAX_HW);
		return -1;
	}
	return (int64_t)lp_workspace(N, H, W).bytes;
}

extern "C" int fr_lpips_forward(const fr_lpips_args *a)
{
	if (!a) { set_error("lpips_forward: args is null"); return FR_ERR_INVALID; }
	if (a->size < sizeof(fr_lpips_args)) { set_error("lpips_forward: size=%u is smaller than fr_lpips_args (%zu)", a->size, sizeof(fr_lpips_args)); return FR_ERR_INVALID; }
	if (a->N < 1 || a->N > LP_MAX_N) { set_error("lpips_forward: N=%d is outside 1 .. %d", a->N, LP_MAX_N); return FR_ERR_INVALID; }
	if (a->H < 16 || a->H > LP_MAX_HW) { set_error("lpips_forward: H=%d is outside 16 .. %d (the fourth pool needs 16 rows)", a->H, LP_MAX_HW); return FR_ERR_INVALID; }
	if (a->W < 16 || a->W > LP_MAX_HW) { set_error("lpips_forward: W=%d is outside 16 .. %d (the fourth pool needs 16 columns)", a->W, LP_MAX_HW); return FR_ERR_INVALID; }
	if (!a->x) { set_error("lpips_forward: x is null"); return FR_ERR_INVALID; }
	if (!a->y) { set_error("lpips_forward: y is null"); return FR_ERR_INVALID; }
	if (!a->packed) { set_error("lpips_forward: packed is null"); return FR_ERR_INVALID; }
	if (!a->workspace) { set_error("lpips_forward: workspace is null"); return FR_ERR_INVALID; }
	if (!a->out) { set_error("lpips_forward: out is null"); return FR_ERR_INVALID; }
	if (((uintptr_t)a->packed & 15) || ((uintptr_t)a->workspace & 255)) { set_error("lpips_forward: packed must be 16-byte and workspace 256-byte aligned"); return FR_ERR_INVALID; }
	const int N = a->N, NI = 2 * a->N;
	const bool debug = a->debug != 0;
	hipStream_t stream = (hipStream_t)a->stream;
	const LpPacked P = lp_packed();
	const LpWorkspace L = lp_workspace(N, a->H, a->W);
	const float *pk = (const float *)a->packed;
	char *ws = (char *)a->workspace;
	double *scal = (double *)(ws + L.scal), *partials = (double *)(ws + L.partials);
	float *buf[2] = { (float *)(ws + L.buf[0]), (float *)(ws + L.buf[1]) };
	int H = a->H, W = a->W, cur = 0, rc, stage = 0;
	auto mark = [&]() { if (a->stage_events && a->stage_events[stage]) (void)hipEventRecord((hipEvent_t)a->stage_events[stage], stream); stage++; };
	mark();
	{
		const dim3 grid((unsigned)(((size_t)H * W + 255) / 256), 8, N);
		hipLaunchKernelGGL(k_lpips_conv0, grid, dim3(256), 0, stream, H, W, a->x, 0, pk + P.w[0], pk + P.b[0], buf[0]);
		hipLaunchKernelGGL(k_lpips_conv0, grid, dim3(256), 0, stream, H, W, a->y, N, pk + P.w[0], pk + P.b[0], buf[0]);
		if ((rc = check_launch("lpips_forward (first layer)", stream, debug)) != FR_OK) return rc;
		mark();
	}
	int tap = 0;
	for (int l = 1; l < LP_LAYERS; l++)
	{
		const dim3 grid((W + LP_TILE - 1) / LP_TILE, (H + LP_TILE - 1) / LP_TILE, NI * (lp_cout[l] / 64));
		hipLaunchKernelGGL(k_lpips_conv, grid, dim3(256), 0, stream, H, W, lp_cin[l], lp_cout[l], buf[cur], pk + P.w[l], pk + P.b[l], buf[cur ^ 1]);
		if ((rc = check_launch("lpips_forward (convolution)", stream, debug)) != FR_OK) return rc;
		mark();
		cur ^= 1;
		if (l != lp_tap_layer[tap]) continue;
		const bool last = tap == LP_TAPS - 1;
		const dim3 hgrid((W + LP_HEAD_W - 1) / LP_HEAD_W, (H + 1) / 2, N);
		hipLaunchKernelGGL(k_lpips_head, hgrid, dim3(256), 0, stream, N, lp_tap_c[tap], H, W, buf[cur], pk + P.lin[tap], last ? nullptr : buf[cur ^ 1],
			a->out_features[tap], partials);
		hipLaunchKernelGGL(k_lpips_finish, dim3(1), dim3(1024), 0, stream, (long long)N * hgrid.x * hgrid.y, (double)H * (double)W, tap, partials, scal,
			a->out_taps, a->out);
		if ((rc = check_launch("lpips_forward (head)", stream, debug)) != FR_OK) return rc;
		mark();
		cur ^= 1; H >>= 1; W >>= 1; tap++;
	}
	return FR_OK;
}
