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
//
// As a training loss (the reference's nn.Module under torch.autograd: lpips(render, gt).backward()):
//   fr_lpips_forward_keep   the same kernels, x's 13 post-ReLU maps written to a caller-owned kept state instead of ping-ponging
//                           (y's still ping-pong), and k_lpips_head<true>: the head also writes the gradient of the tap's value with
//                           respect to x's tap map, scaled by 1 / (H_k W_k), while both pictures' taps are in hand -- chosen over
//                           keeping y's five taps for the backward: the same bytes kept, one pass over them less.
//   fr_lpips_backward       layers 12 .. 1: k_lpips_conv's main loop on the transposed, flipped weights with the epilogues
//                           LP_EPI_MASK (the ReLU rule) and LP_EPI_POOL_TAP (pool scatter to the first maximum + the tap's own
//                           gradient + the ReLU rule, behind the four pooled taps); then k_lpips_conv0_bwd, 64 -> 3, 1 / std and
//                           the upstream scalar, read on the device. The gradient at a layer's output ping-pongs in the workspace.
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

// the differentiable forward's kept state: x's 13 post-ReLU maps in the convolution's layout, and the five tap gradients
// (d value / d tap map of x, k_lpips_head<true>) in the same layout. y's maps are not kept.
struct LpKeep { size_t act[LP_LAYERS], tg[LP_TAPS], bytes; };
static int lp_layer_shift(int l) { return l < 2 ? 0 : l < 4 ? 1 : l < 7 ? 2 : l < 10 ? 3 : 4; } // pools in front of layer l
static LpKeep lp_keep(int N, int H, int W)
{
	LpKeep K; size_t off = 0;
	for (int l = 0; l < LP_LAYERS; l++)
	{
		K.act[l] = off; off = align_up(off + (size_t)N * lp_cout[l] * (H >> lp_layer_shift(l)) * (W >> lp_layer_shift(l)) * 4);
	}
	for (int k = 0; k < LP_TAPS; k++)
	{
		K.tg[k] = off; off = align_up(off + (size_t)N * lp_tap_c[k] * (H >> k) * (W >> k) * 4);
	}
	K.bytes = off;
	return K;
}

// backward weights, in floats: the first layer's [chunk][tap][8][3], then the slabs of the layers 1 .. 12
struct LpBackPacked { size_t w[LP_LAYERS], floats; };
static LpBackPacked lp_back_packed()
{
	LpBackPacked P; size_t off = 0;
	for (int l = 0; l < LP_LAYERS; l++) { P.w[l] = off; off += (size_t)9 * lp_cin[l] * lp_cout[l]; }
	P.floats = off;
	return P;
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
//
// The backward pass runs the same main loop on the transposed, flipped weights (fr_lpips_pack_backward_weights; no bias) with one
// of two other epilogues. `act` is the kept post-ReLU map the gradient arrives at, in the layout of `out`:
//   LP_EPI_MASK      out = sum * (act > 0): the ReLU rule, for a layer that no pool follows.
//   LP_EPI_POOL_TAP  H x W is the POOLED size, act / tapgrad / out are the tap map in front of the pool, Ht x Wt. A pooled value
//                    goes to the first maximum of its 2 x 2 window in row-major order (torch's `val > maxval`), zero to the other
//                    three; the tap's own gradient is added at all four and the sum is masked by act > 0. The row Ht - 1 of an odd
//                    Ht lies in no window: the lane that owns the pooled pixel (H - 1, gx) writes tapgrad * mask at (Ht - 1, 2 gx)
//                    and (Ht - 1, 2 gx + 1); likewise the column Wt - 1 of an odd Wt by the owner of (gy, W - 1), and the corner
//                    (Ht - 1, Wt - 1) by the owner of (H - 1, W - 1). Every pooled pixel has exactly one owner per channel, so
//                    every element of the tap map is written exactly once.
// The masks are selections, not products: a gradient at a dead activation is dropped whatever its value.
enum { LP_EPI_RELU = 0, LP_EPI_MASK = 1, LP_EPI_POOL_TAP = 2 };
typedef float lp_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 lp_mask(const float4 a, const float4 v)
{
	return make_float4(a.x > 0.0f ? v.x : 0.0f, a.y > 0.0f ? v.y : 0.0f, a.z > 0.0f ? v.z : 0.0f, a.w > 0.0f ? v.w : 0.0f);
}
template <int EPI>
__global__ void __launch_bounds__(256) k_lpips_conv(int H, int W, int Cin, int Cout, const float *__restrict__ in, const float *__restrict__ wp,
	const float *__restrict__ bias, float *__restrict__ out, const float *__restrict__ act, const float *__restrict__ tapgrad, int Ht, int Wt)
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
		if constexpr (EPI == LP_EPI_RELU)
		{
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
		else if constexpr (EPI == LP_EPI_MASK)
		{
#pragma unroll
			for (int r = 0; r < 4; r++)
			{
				const int gy = ty0 + wave * 4 + r;
				if (gy >= H) continue;
				const size_t at = (((size_t)img * (Cout >> 3) + (co >> 3)) * plane + (size_t)gy * W + gx) * 8 + (co & 7);
				*(float4 *)(out + at) = lp_mask(*(const float4 *)(act + at), make_float4(tot[mt][r][0], tot[mt][r][1], tot[mt][r][2], tot[mt][r][3]));
			}
		}
		else
		{
			const size_t cbase = ((size_t)img * (Cout >> 3) + (co >> 3)) * ((size_t)Ht * Wt) * 8 + (co & 7);
			// the tap's own gradient, masked, at a position no window covers -- or with `v` added, at a position of a window
			auto put = [&](int y, int x, const float4 v) {
				const size_t at = cbase + ((size_t)y * Wt + x) * 8;
				const float4 t = *(const float4 *)(tapgrad + at);
				*(float4 *)(out + at) = lp_mask(*(const float4 *)(act + at), make_float4(v.x + t.x, v.y + t.y, v.z + t.z, v.w + t.w));
			};
			const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
			const bool edge_c = (Wt & 1) && gx == W - 1;
#pragma unroll
			for (int r = 0; r < 4; r++)
			{
				const int gy = ty0 + wave * 4 + r;
				if (gy >= H) continue;
				float a[4][4]; // [window position 2 j + i][channel]
#pragma unroll
				for (int p = 0; p < 4; p++)
				{
					const float4 v = *(const float4 *)(act + cbase + ((size_t)(2 * gy + (p >> 1)) * Wt + 2 * gx + (p & 1)) * 8);
					a[p][0] = v.x; a[p][1] = v.y; a[p][2] = v.z; a[p][3] = v.w;
				}
				int first[4];
#pragma unroll
				for (int q = 0; q < 4; q++)
				{
					float best = a[0][q];
					first[q] = 0;
#pragma unroll
					for (int p = 1; p < 4; p++)
						if (a[p][q] > best) { best = a[p][q]; first[q] = p; }
				}
#pragma unroll
				for (int p = 0; p < 4; p++)
					put(2 * gy + (p >> 1), 2 * gx + (p & 1), make_float4(first[0] == p ? tot[mt][r][0] : 0.0f, first[1] == p ? tot[mt][r][1] : 0.0f,
						first[2] == p ? tot[mt][r][2] : 0.0f, first[3] == p ? tot[mt][r][3] : 0.0f));
				const bool edge_r = (Ht & 1) && gy == H - 1;
				if (edge_r) { put(Ht - 1, 2 * gx, zero); put(Ht - 1, 2 * gx + 1, zero); }
				if (edge_c) { put(2 * gy, Wt - 1, zero); put(2 * gy + 1, Wt - 1, zero); }
				if (edge_r && edge_c) put(Ht - 1, Wt - 1, zero);
			}
		}
	}
}

// ---- head: norms, weighted squared difference, sum; 2x2 max pool of both maps ----------------------------------------------
// featx, featy: [N][C / 8][H][W][8], the tap of x's and of y's pictures. A wave owns 2 rows x 8 pixels (four pool windows); lane = half + 2 xx + 16 r +
// 32 par holds the channels 4 half .. 4 half + 3 of the blocks par, par + 2, ... of pixel (2 qy + r, x0 + xx): 8 pixels x 32 bytes of
// a row and block are one 256-byte run. pooledx, pooledy (optional, both or none): [N][C / 8][H / 2][W / 2][8]. features (optional):
// x's tap, [N,C,H,W]. partials[n * gridDim.y * gridDim.x + block] = the sum of d over the block's pixels, waves added in wave order.
// KEEP (the differentiable forward) adds a second pass over the channels that writes tapgrad, in featx's layout: the gradient of the
// tap's value with respect to x's tap map, masked by the ReLU rule. With s = sqrt(sum a^2), n = s + 1e-10, u_c = w_c (a_c / nx -
// b_c / ny):   d value / d a_c = (2 u_c / nx - 2 a_c (sum_j u_j a_j) / (nx^2 s)) / (H W),   sum_j u_j a_j = wxx / nx - wxy / ny
// from the sums of the first pass. Everything is formed in double from the float inputs; equal pictures give a_c / nx - b_c / ny = 0
// and wxx / nx - wxy / ny = 0 exactly, so every element is exactly 0. At s = 0 (a tap vector that is all zero) the second term is
// taken as 0, its limit -- the reference's sqrt backward yields inf * 0 = NaN there -- and the mask drops the first.
template <bool KEEP>
__global__ void __launch_bounds__(256) k_lpips_head(int C, int H, int W, const float *__restrict__ featx, const float *__restrict__ featy,
	const float *__restrict__ lin, float *__restrict__ pooledx, float *__restrict__ pooledy, float *__restrict__ features, double *__restrict__ partials,
	float *__restrict__ tapgrad)
{
	__shared__ double s_w[4];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int half = lane & 1, xx = (lane >> 1) & 7, r = (lane >> 4) & 1, par = lane >> 5;
	const int n = blockIdx.z, CB = C >> 3;
	const int gy = 2 * blockIdx.y + r, gx = blockIdx.x * LP_HEAD_W + wave * 8 + xx;
	const bool in = gy < H && gx < W;
	const int Hp = H >> 1, Wp = W >> 1;
	const bool pool_out = pooledx != nullptr && r == 0 && (xx & 1) == 0 && (int)blockIdx.y < Hp && (gx >> 1) < Wp;
	const size_t plane = (size_t)H * W, pplane = (size_t)Hp * Wp;
	const size_t pix = (size_t)gy * W + gx, ppix = (size_t)blockIdx.y * Wp + (gx >> 1);
	double sxx = 0.0, syy = 0.0, wxx = 0.0, wyy = 0.0, wxy = 0.0;
	for (int cb = par; cb < CB; cb += 2)
	{
		float4 ax = make_float4(0.0f, 0.0f, 0.0f, 0.0f), ay = ax;
		if (in)
		{
			ax = *(const float4 *)(featx + (((size_t)n * CB + cb) * plane + pix) * 8 + 4 * half);
			ay = *(const float4 *)(featy + (((size_t)n * CB + cb) * plane + pix) * 8 + 4 * half);
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
		if (pooledx != nullptr) // uniform: every lane takes part in the exchanges
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
				*(float4 *)(pooledx + (((size_t)n * CB + cb) * pplane + ppix) * 8 + 4 * half) = make_float4(mx[0], mx[1], mx[2], mx[3]);
				*(float4 *)(pooledy + (((size_t)n * CB + cb) * pplane + ppix) * 8 + 4 * half) = make_float4(my[0], my[1], my[2], my[3]);
			}
		}
	}
	// the pixel's five sums: the two halves, then the two block parities
	sxx += __shfl_xor(sxx, 1); syy += __shfl_xor(syy, 1); wxx += __shfl_xor(wxx, 1); wyy += __shfl_xor(wyy, 1); wxy += __shfl_xor(wxy, 1);
	sxx += __shfl_xor(sxx, 32); syy += __shfl_xor(syy, 32); wxx += __shfl_xor(wxx, 32); wyy += __shfl_xor(wyy, 32); wxy += __shfl_xor(wxy, 32);
	const double nx = sqrt(sxx) + 1e-10, ny = sqrt(syy) + 1e-10;
	const double q1 = wxx / (nx * nx), q2 = wxy / (nx * ny), q3 = wyy / (ny * ny);
	double d = in ? (q1 - 2.0 * q2) + q3 : 0.0; // equal pictures: q - 2 q + q = 0 exactly
	if constexpr (KEEP)
	{
		if (in) // every lane of a pixel holds the pixel's sums
		{
			const double sx = sqrt(sxx), rnx = 1.0 / nx, rny = 1.0 / ny, rhw = 1.0 / ((double)H * (double)W);
			const double ua = wxx * rnx - wxy * rny;
			const double k2 = sx > 0.0 ? ua * rnx * rnx / sx : 0.0;
			for (int cb = par; cb < CB; cb += 2)
			{
				const size_t at = (((size_t)n * CB + cb) * plane + pix) * 8 + 4 * half;
				const float4 ax = *(const float4 *)(featx + at), ay = *(const float4 *)(featy + at), wv = *(const float4 *)(lin + cb * 8 + 4 * half);
				const float xa[4] = { ax.x, ax.y, ax.z, ax.w }, ya[4] = { ay.x, ay.y, ay.z, ay.w }, wa[4] = { wv.x, wv.y, wv.z, wv.w };
				float g[4];
#pragma unroll
				for (int j = 0; j < 4; j++)
				{
					const double a = (double)xa[j], u = (double)wa[j] * (a * rnx - (double)ya[j] * rny);
					g[j] = xa[j] > 0.0f ? (float)((2.0 * u * rnx - 2.0 * a * k2) * rhw) : 0.0f;
				}
				*(float4 *)(tapgrad + at) = make_float4(g[0], g[1], g[2], g[3]);
			}
		}
	}
	// the wave's 16 pixels (every lane of a pixel holds the same d)
	d += __shfl_xor(d, 2); d += __shfl_xor(d, 4); d += __shfl_xor(d, 8); d += __shfl_xor(d, 16);
	if (lane == 0) s_w[wave] = d;
	__syncthreads();
	if (threadIdx.x == 0)
		partials[((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// ---- backward of the first layer: 64 -> 3, the z-score's 1 / std and the upstream gradient ---------------------------------
// dact: [N][8][H][W][8], the gradient at relu1_1 (already masked). A workgroup owns 16 x 16 pixels, a thread one pixel and its three
// channels; per 8-channel chunk the 18 x 18 halo tile goes through LDS, so the map is read once. wb: [chunk][tap][8][3], the flipped
// taps (fr_lpips_pack_backward_weights). Two levels as in k_lpips_conv: a chunk's 72 products per channel are one fmaf chain from
// zero, the eight chunk sums are added in chunk order. upstream[0] is read on the device. dx: [N,3,H,W] planes.
__global__ void __launch_bounds__(256) k_lpips_conv0_bwd(int H, int W, const float *__restrict__ dact, const float *__restrict__ wb,
	const float *__restrict__ upstream, float *__restrict__ dx)
{
	__shared__ __attribute__((aligned(16))) float sw[8 * 9 * 8 * 3];
	__shared__ __attribute__((aligned(16))) float il[2 * LP_NPIX * 4];
	const int n = blockIdx.z, tx0 = blockIdx.x * LP_TILE, ty0 = blockIdx.y * LP_TILE;
	const int px = threadIdx.x & 15, py = threadIdx.x >> 4;
	const size_t plane = (size_t)H * W;
	for (int i = threadIdx.x; i < 8 * 9 * 8 * 3; i += 256) sw[i] = wb[i];
	float tot[3] = { 0.0f, 0.0f, 0.0f };
	for (int ck = 0; ck < 8; ck++)
	{
		__syncthreads(); // the previous chunk's reads are done (and, the first time, sw is written)
		const float *base = dact + ((size_t)n * 8 + ck) * plane * 8;
		for (int i = threadIdx.x; i < 2 * LP_NPIX; i += 256)
		{
			const int pix = i >> 1, cg = i & 1;
			const int hy = pix / LP_HALO, hx = pix - hy * LP_HALO;
			const int gy = ty0 + hy - 1, gx = tx0 + hx - 1;
			float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
			if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *(const float4 *)(base + ((size_t)gy * W + gx) * 8 + 4 * cg);
			((float4 *)il)[cg * LP_NPIX + pix] = v;
		}
		__syncthreads();
		float acc[3] = { 0.0f, 0.0f, 0.0f };
#pragma unroll
		for (int t = 0; t < 9; t++)
#pragma unroll
			for (int cg = 0; cg < 2; cg++)
			{
				const float4 v = ((const float4 *)il)[cg * LP_NPIX + (py + t / 3) * LP_HALO + px + t % 3];
				const float va[4] = { v.x, v.y, v.z, v.w };
				const float *w = sw + ((ck * 9 + t) * 8 + 4 * cg) * 3;
#pragma unroll
				for (int c = 0; c < 4; c++)
#pragma unroll
					for (int ci = 0; ci < 3; ci++) acc[ci] = fmaf(va[c], w[c * 3 + ci], acc[ci]);
			}
#pragma unroll
		for (int ci = 0; ci < 3; ci++) tot[ci] += acc[ci];
	}
	const int gy = ty0 + py, gx = tx0 + px;
	if (gy >= H || gx >= W) return;
	const float sd[3] = { .458f, .448f, .450f };
	const float up = upstream[0];
#pragma unroll
	for (int ci = 0; ci < 3; ci++) dx[((size_t)n * 3 + ci) * plane + (size_t)gy * W + gx] = tot[ci] / sd[ci] * up;
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
		hipLaunchKernelGGL(k_lpips_conv<LP_EPI_RELU>, grid, dim3(256), 0, stream, H, W, lp_cin[l], lp_cout[l], (const float *)buf[cur], pk + P.w[l], pk + P.b[l],
			buf[cur ^ 1], (const float *)nullptr, (const float *)nullptr, 0, 0);
		if ((rc = check_launch("lpips_forward (convolution)", stream, debug)) != FR_OK) return rc;
		mark();
		cur ^= 1;
		if (l != lp_tap_layer[tap]) continue;
		const bool last = tap == LP_TAPS - 1;
		const dim3 hgrid((W + LP_HEAD_W - 1) / LP_HEAD_W, (H + 1) / 2, N);
		const size_t ys = (size_t)N * lp_tap_c[tap] * H * W, yp = (size_t)N * lp_tap_c[tap] * (H >> 1) * (W >> 1); // y's pictures follow x's
		hipLaunchKernelGGL(k_lpips_head<false>, hgrid, dim3(256), 0, stream, lp_tap_c[tap], H, W, (const float *)buf[cur], (const float *)buf[cur] + ys,
			pk + P.lin[tap], last ? nullptr : buf[cur ^ 1], last ? nullptr : buf[cur ^ 1] + yp, a->out_features[tap], partials, (float *)nullptr);
		hipLaunchKernelGGL(k_lpips_finish, dim3(1), dim3(1024), 0, stream, (long long)N * hgrid.x * hgrid.y, (double)H * (double)W, tap, partials, scal,
			a->out_taps, a->out);
		if ((rc = check_launch("lpips_forward (head)", stream, debug)) != FR_OK) return rc;
		mark();
		cur ^= 1; H >>= 1; W >>= 1; tap++;
	}
	return FR_OK;
}

// ---- the differentiable path: backward weights, the forward that keeps x's maps, the backward pass -----------------------------

extern "C" size_t fr_lpips_backward_packed_bytes(void)
{
	return lp_back_packed().floats * sizeof(float);
}

extern "C" int fr_lpips_pack_backward_weights(const float *const *conv_weights, void *packed_backward)
{
	if (!conv_weights) { set_error("lpips_pack_backward_weights: conv_weights is null"); return FR_ERR_INVALID; }
	if (!packed_backward) { set_error("lpips_pack_backward_weights: packed_backward is null"); return FR_ERR_INVALID; }
	for (int l = 0; l < LP_LAYERS; l++)
		if (!conv_weights[l]) { set_error("lpips_pack_backward_weights: conv_weights[%d] is null", l); return FR_ERR_INVALID; }
	const LpBackPacked P = lp_back_packed();
	float *out = (float *)packed_backward;
	// first layer: [chunk of 8 outputs][tap][8][3 inputs], the taps flipped (tap t reads W[.][.][8 - t])
	for (int co = 0; co < 64; co++)
		for (int ci = 0; ci < 3; ci++)
			for (int t = 0; t < 9; t++) out[P.w[0] + (((size_t)(co >> 3) * 9 + t) * 8 + (co & 7)) * 3 + ci] = conv_weights[0][(co * 3 + ci) * 9 + 8 - t];
	// W'[ci][co][t] = W[co][ci][8 - t] in k_lpips_conv's slabs: the backward convolution's outputs are the forward's inputs
	for (int l = 1; l < LP_LAYERS; l++)
	{
		const int ci_n = lp_cin[l], co_n = lp_cout[l], kb = co_n / 8; // kb: 8-channel chunks of the backward's K
		const float *w = conv_weights[l];
		float *o = out + P.w[l];
		for (int co = 0; co < co_n; co++)
			for (int ci = 0; ci < ci_n; ci++)
				for (int t = 0; t < 9; t++)
				{
					const size_t slab = (size_t)(ci / 64) * kb + co / 8;
					const int cg = (co & 7) >> 2, hh = co & 3;
					o[slab * LP_SLAB + ((size_t)(t * 2 + cg) * 64 + (ci & 63)) * 4 + hh] = w[((size_t)co * ci_n + ci) * 9 + 8 - t];
				}
	}
	return FR_OK;
}

extern "C" int64_t fr_lpips_keep_workspace_bytes(int32_t N, int32_t H, int32_t W)
{
	if (!lp_sizes_ok(N, H, W))
	{
		set_error("lpips_keep_workspace_bytes: bad sizes N=%d H=%d W=%d (N 1 .. %d, H and W 16 .. %d)", N, H, W, LP_MAX_N, LP_MAX_HW);
		return -1;
	}
	return (int64_t)lp_keep(N, H, W).bytes;
}

extern "C" int64_t fr_lpips_keep_activation_offset(int32_t N, int32_t H, int32_t W, int32_t layer)
{
	if (!lp_sizes_ok(N, H, W))
	{
		set_error("lpips_keep_activation_offset: bad sizes N=%d H=%d W=%d (N 1 .. %d, H and W 16 .. %d)", N, H, W, LP_MAX_N, LP_MAX_HW);
		return -1;
	}
	if (layer < 0 || layer >= LP_LAYERS) { set_error("lpips_keep_activation_offset: layer=%d is outside 0 .. %d", layer, LP_LAYERS - 1); return -1; }
	return (int64_t)lp_keep(N, H, W).act[layer];
}

// the checks the forward, the keeping forward and the backward share; `who` names the call
static int lp_check_sizes(const char *who, uint32_t size, size_t want, const char *strct, int N, int H, int W)
{
	if (size < want) { set_error("%s: size=%u is smaller than %s (%zu)", who, size, strct, want); return FR_ERR_INVALID; }
	if (N < 1 || N > LP_MAX_N) { set_error("%s: N=%d is outside 1 .. %d", who, N, LP_MAX_N); return FR_ERR_INVALID; }
	if (H < 16 || H > LP_MAX_HW) { set_error("%s: H=%d is outside 16 .. %d (the fourth pool needs 16 rows)", who, H, LP_MAX_HW); return FR_ERR_INVALID; }
	if (W < 16 || W > LP_MAX_HW) { set_error("%s: W=%d is outside 16 .. %d (the fourth pool needs 16 columns)", who, W, LP_MAX_HW); return FR_ERR_INVALID; }
	return FR_OK;
}

extern "C" int fr_lpips_forward_keep(const fr_lpips_keep_args *a)
{
	int rc;
	if (!a) { set_error("lpips_forward_keep: args is null"); return FR_ERR_INVALID; }
	if ((rc = lp_check_sizes("lpips_forward_keep", a->size, sizeof(fr_lpips_keep_args), "fr_lpips_keep_args", a->N, a->H, a->W)) != FR_OK) return rc;
	if (!a->x) { set_error("lpips_forward_keep: x is null"); return FR_ERR_INVALID; }
	if (!a->y) { set_error("lpips_forward_keep: y is null"); return FR_ERR_INVALID; }
	if (!a->packed) { set_error("lpips_forward_keep: packed is null"); return FR_ERR_INVALID; }
	if (!a->workspace) { set_error("lpips_forward_keep: workspace is null"); return FR_ERR_INVALID; }
	if (!a->keep) { set_error("lpips_forward_keep: keep is null"); return FR_ERR_INVALID; }
	if (!a->out) { set_error("lpips_forward_keep: out is null"); return FR_ERR_INVALID; }
	if (((uintptr_t)a->packed & 15) || ((uintptr_t)a->workspace & 255) || ((uintptr_t)a->keep & 255))
	{
		set_error("lpips_forward_keep: packed must be 16-byte, workspace and keep 256-byte aligned");
		return FR_ERR_INVALID;
	}
	const int N = a->N;
	const bool debug = a->debug != 0;
	hipStream_t stream = (hipStream_t)a->stream;
	const LpPacked P = lp_packed();
	const LpWorkspace L = lp_workspace(N, a->H, a->W);
	const LpKeep K = lp_keep(N, a->H, a->W);
	const float *pk = (const float *)a->packed;
	char *ws = (char *)a->workspace, *kp = (char *)a->keep;
	double *scal = (double *)(ws + L.scal), *partials = (double *)(ws + L.partials);
	// y's pictures ping-pong in the first half of the two buffers; the second half takes x's pooled tap, the next group's input
	float *buf[2] = { (float *)(ws + L.buf[0]), (float *)(ws + L.buf[1]) };
	const size_t half = L.buf_floats / 2;
	int H = a->H, W = a->W, cur = 0, stage = 0;
	auto mark = [&]() { if (a->stage_events && a->stage_events[stage]) (void)hipEventRecord((hipEvent_t)a->stage_events[stage], stream); stage++; };
	mark();
	{
		const dim3 grid((unsigned)(((size_t)H * W + 255) / 256), 8, N);
		hipLaunchKernelGGL(k_lpips_conv0, grid, dim3(256), 0, stream, H, W, a->x, 0, pk + P.w[0], pk + P.b[0], (float *)(kp + K.act[0]));
		hipLaunchKernelGGL(k_lpips_conv0, grid, dim3(256), 0, stream, H, W, a->y, 0, pk + P.w[0], pk + P.b[0], buf[0]);
		if ((rc = check_launch("lpips_forward_keep (first layer)", stream, debug)) != FR_OK) return rc;
		mark();
	}
	const float *xin = (const float *)(kp + K.act[0]);
	int tap = 0;
	for (int l = 1; l < LP_LAYERS; l++)
	{
		const dim3 grid((W + LP_TILE - 1) / LP_TILE, (H + LP_TILE - 1) / LP_TILE, N * (lp_cout[l] / 64));
		float *xout = (float *)(kp + K.act[l]);
		hipLaunchKernelGGL(k_lpips_conv<LP_EPI_RELU>, grid, dim3(256), 0, stream, H, W, lp_cin[l], lp_cout[l], xin, pk + P.w[l], pk + P.b[l], xout,
			(const float *)nullptr, (const float *)nullptr, 0, 0);
		hipLaunchKernelGGL(k_lpips_conv<LP_EPI_RELU>, grid, dim3(256), 0, stream, H, W, lp_cin[l], lp_cout[l], (const float *)buf[cur], pk + P.w[l], pk + P.b[l],
			buf[cur ^ 1], (const float *)nullptr, (const float *)nullptr, 0, 0);
		if ((rc = check_launch("lpips_forward_keep (convolution)", stream, debug)) != FR_OK) return rc;
		mark();
		cur ^= 1; xin = xout;
		if (l != lp_tap_layer[tap]) continue;
		const bool last = tap == LP_TAPS - 1;
		const dim3 hgrid((W + LP_HEAD_W - 1) / LP_HEAD_W, (H + 1) / 2, N);
		hipLaunchKernelGGL(k_lpips_head<true>, hgrid, dim3(256), 0, stream, lp_tap_c[tap], H, W, xin, (const float *)buf[cur], pk + P.lin[tap],
			last ? nullptr : buf[cur ^ 1] + half, last ? nullptr : buf[cur ^ 1], (float *)nullptr, partials, (float *)(kp + K.tg[tap]));
		hipLaunchKernelGGL(k_lpips_finish, dim3(1), dim3(1024), 0, stream, (long long)N * hgrid.x * hgrid.y, (double)H * (double)W, tap, partials, scal,
			a->out_taps, a->out);
		if ((rc = check_launch("lpips_forward_keep (head)", stream, debug)) != FR_OK) return rc;
		mark();
		cur ^= 1; xin = buf[cur] + half; H >>= 1; W >>= 1; tap++;
	}
	return FR_OK;
}

extern "C" int fr_lpips_backward(const fr_lpips_backward_args *a)
{
	int rc;
	if (!a) { set_error("lpips_backward: args is null"); return FR_ERR_INVALID; }
	if ((rc = lp_check_sizes("lpips_backward", a->size, sizeof(fr_lpips_backward_args), "fr_lpips_backward_args", a->N, a->H, a->W)) != FR_OK) return rc;
	if (!a->packed_backward) { set_error("lpips_backward: packed_backward is null"); return FR_ERR_INVALID; }
	if (!a->keep) { set_error("lpips_backward: keep is null"); return FR_ERR_INVALID; }
	if (!a->workspace) { set_error("lpips_backward: workspace is null"); return FR_ERR_INVALID; }
	if (!a->grad_out) { set_error("lpips_backward: grad_out is null"); return FR_ERR_INVALID; }
	if (!a->grad_x) { set_error("lpips_backward: grad_x is null"); return FR_ERR_INVALID; }
	if (((uintptr_t)a->packed_backward & 15) || ((uintptr_t)a->workspace & 255) || ((uintptr_t)a->keep & 255))
	{
		set_error("lpips_backward: packed_backward must be 16-byte, workspace and keep 256-byte aligned");
		return FR_ERR_INVALID;
	}
	const int N = a->N;
	const bool debug = a->debug != 0;
	hipStream_t stream = (hipStream_t)a->stream;
	const LpBackPacked P = lp_back_packed();
	const LpWorkspace L = lp_workspace(N, a->H, a->W);
	const LpKeep K = lp_keep(N, a->H, a->W);
	const float *pb = (const float *)a->packed_backward;
	const char *kp = (const char *)a->keep;
	char *ws = (char *)a->workspace;
	float *buf[2] = { (float *)(ws + L.buf[0]), (float *)(ws + L.buf[1]) }; // the gradient at a layer's output ping-pongs
	int cur = 0, stage = 0, tap = LP_TAPS - 1;
	auto mark = [&]() { if (a->stage_events && a->stage_events[stage]) (void)hipEventRecord((hipEvent_t)a->stage_events[stage], stream); stage++; };
	mark();
	const float *din = (const float *)(kp + K.tg[tap]); // the chain starts at relu5_3: the last tap's gradient, masked by the head
	for (int l = LP_LAYERS - 1; l >= 1; l--)
	{
		const int H = a->H >> lp_layer_shift(l), W = a->W >> lp_layer_shift(l);
		const dim3 grid((W + LP_TILE - 1) / LP_TILE, (H + LP_TILE - 1) / LP_TILE, N * (lp_cin[l] / 64));
		const float *act = (const float *)(kp + K.act[l - 1]);
		if (lp_layer_shift(l) != lp_layer_shift(l - 1)) // a pool in front of layer l: its input is the pooled tap
		{
			tap--;
			hipLaunchKernelGGL(k_lpips_conv<LP_EPI_POOL_TAP>, grid, dim3(256), 0, stream, H, W, lp_cout[l], lp_cin[l], din, pb + P.w[l], (const float *)nullptr,
				buf[cur], act, (const float *)(kp + K.tg[tap]), a->H >> lp_layer_shift(l - 1), a->W >> lp_layer_shift(l - 1));
		}
		else
			hipLaunchKernelGGL(k_lpips_conv<LP_EPI_MASK>, grid, dim3(256), 0, stream, H, W, lp_cout[l], lp_cin[l], din, pb + P.w[l], (const float *)nullptr,
				buf[cur], act, (const float *)nullptr, 0, 0);
		if ((rc = check_launch("lpips_backward (convolution)", stream, debug)) != FR_OK) return rc;
		mark();
		din = buf[cur]; cur ^= 1;
	}
	const dim3 grid((a->W + LP_TILE - 1) / LP_TILE, (a->H + LP_TILE - 1) / LP_TILE, N);
	hipLaunchKernelGGL(k_lpips_conv0_bwd, grid, dim3(256), 0, stream, a->H, a->W, din, pb + P.w[0], a->grad_out, a->grad_x);
	if ((rc = check_launch("lpips_backward (first layer)", stream, debug)) != FR_OK) return rc;
	mark();
	return FR_OK;
}
