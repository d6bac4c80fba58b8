// fovraster -- the quality metrics of the pruning loop's gate: mean SSIM, PSNR and mean L1 of a render against its ground
// truth, and a meter that adds them up over the views on the device.
//
// Reference behaviour:
//   fov3dgs/prune.py:137-174        test_ssim_loss / test_psnr_loss: every camera is rendered twice, ssim() and psnr().mean() are
//                                   added up as Python scalars (a host synchronisation per view) and divided by the view count;
//                                   :284-290, :327-331, :345-349 compare the two means with target_ssim / target_psnr.
//   fov3dgs/utils/loss_utils.py:37-76   ssim: the 11x11 Gaussian window (sigma 1.5), zero padding 5, C1 = 0.01^2, C2 = 0.03^2.
//   fov3dgs/utils/image_utils.py:14-19  mse = mean((a - b)^2) per row of view(shape[0], -1); psnr = 20 log10(1 / sqrt(mse)).
// Here ONE pass over the picture pair leaves three sums per 16x32 tile (the SSIM map with the arithmetic of k_l1_ssim_fwd in
// loss.hip, restated here so that loss.hip and its results stay untouched; the squared error; the absolute error), and a
// one-workgroup finish adds the tiles up in double in a fixed order (no float atomics: the same bits on every run), writes
// (ssim, psnr, l1, mse) into the view's slot of a caller-owned array and adds them to a caller-owned accumulator. Nothing
// leaves the device before the caller reads the array back.
#include "common.h"

namespace fr {

#define FR_Q_TW 16 // the tile of loss.hip: 16 wide, 32 tall, two vertically adjacent outputs per thread, a 5-pixel halo
#define FR_Q_TH 32
#define FR_Q_HALO 5
#define FR_Q_SW (FR_Q_TW + 2 * FR_Q_HALO)
#define FR_Q_SH (FR_Q_TH + 2 * FR_Q_HALO)

// normalised 1-D window gaussian(11, 1.5) of loss_utils.py:26-28 (the values of loss.hip's c_win)
static __device__ __constant__ float c_qwin[11] = {
	1.0283801239e-03f, 7.5987582095e-03f, 3.6000773311e-02f, 1.0936068743e-01f, 2.1300552785e-01f, 2.6601171494e-01f,
	2.1300552785e-01f, 1.0936068743e-01f, 3.6000773311e-02f, 7.5987582095e-03f, 1.0283801239e-03f };

// partials[3 b .. 3 b + 2] = (sum ssim_map, sum (x - y)^2, sum |x - y|) over tile b = (channel, tile row, tile column).
// SSIM = false skips the two separable passes (image_utils.mse / psnr need the errors only) and leaves the first sum 0.
template <bool SSIM>
__global__ void __launch_bounds__(256) k_quality_fwd(int H, int W, const float *__restrict__ x, const float *__restrict__ y, double *__restrict__ partials)
{
	__shared__ float sx[FR_Q_SH][FR_Q_SW + 1], sy[FR_Q_SH][FR_Q_SW + 1];
	__shared__ float hs[SSIM ? 5 : 1][SSIM ? FR_Q_SH : 1][FR_Q_TW + 1];
	__shared__ double s_red[3][4];
	const int tid = threadIdx.x, tx = tid & 15, ty2 = tid >> 4;
	const int bx = blockIdx.x * FR_Q_TW, by = blockIdx.y * FR_Q_TH, ch = blockIdx.z;
	const size_t plane = (size_t)H * W;
	const float *X = x + ch * plane, *Y = y + ch * plane;
	for (int i = tid; i < FR_Q_SH * FR_Q_SW; i += 256)
	{
		const int r = i / FR_Q_SW, c = i - r * FR_Q_SW;
		const int gy = by + r - FR_Q_HALO, gx = bx + c - FR_Q_HALO;
		const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
		sx[r][c] = in ? X[(size_t)gy * W + gx] : 0.0f;
		sy[r][c] = in ? Y[(size_t)gy * W + gx] : 0.0f;
	}
	__syncthreads();
	float acc[2][5];
	if (SSIM)
	{
		// rows: 42 x 8 pairs of adjacent columns, five running sums per column
		for (int i = tid; i < FR_Q_SH * (FR_Q_TW / 2); i += 256)
		{
			const int r = i >> 3, c = (i & 7) * 2;
			float a[12], b[12];
#pragma unroll
			for (int k = 0; k < 12; k++) { a[k] = sx[r][c + k]; b[k] = sy[r][c + k]; }
#pragma unroll
			for (int o = 0; o < 2; o++)
			{
				float m1 = 0, m2 = 0, e11 = 0, e22 = 0, e12 = 0;
#pragma unroll
				for (int k = 0; k < 11; k++)
				{
					const float w = c_qwin[k], av = a[k + o], bv = b[k + o];
					m1 = fmaf(w, av, m1); m2 = fmaf(w, bv, m2);
					e11 = fmaf(w, av * av, e11); e22 = fmaf(w, bv * bv, e22); e12 = fmaf(w, av * bv, e12);
				}
				hs[0][r][c + o] = m1; hs[1][r][c + o] = m2; hs[2][r][c + o] = e11; hs[3][r][c + o] = e22; hs[4][r][c + o] = e12;
			}
		}
		__syncthreads();
		// columns: two vertically adjacent outputs per thread
		float v[5][12];
#pragma unroll
		for (int q = 0; q < 5; q++)
#pragma unroll
			for (int k = 0; k < 12; k++) v[q][k] = hs[q][2 * ty2 + k][tx];
#pragma unroll
		for (int o = 0; o < 2; o++)
#pragma unroll
			for (int q = 0; q < 5; q++)
			{
				float t = 0;
#pragma unroll
				for (int k = 0; k < 11; k++) t = fmaf(c_qwin[k], v[q][k + o], t);
				acc[o][q] = t;
			}
	}
	const int px = bx + tx;
	float ssim_sum = 0.0f, l1_sum = 0.0f;
	double sq_sum = 0.0;
#pragma unroll
	for (int o = 0; o < 2; o++)
	{
		const int ly = 2 * ty2 + o, py = by + ly;
		if (px >= W || py >= H) continue;
		if (SSIM)
		{
			const float m1 = acc[o][0], m2 = acc[o][1], e11 = acc[o][2], e22 = acc[o][3], e12 = acc[o][4];
			const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
			const float mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu12 = m1 * m2;
			const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
			const float a1 = 2.0f * mu12 + C1, a2 = 2.0f * s12 + C2, b1 = mu1_sq + mu2_sq + C1, b2 = s1 + s2 + C2;
			const float inv = 1.0f / (b1 * b2);
			ssim_sum += a1 * a2 * inv;
		}
		const float xv = sx[ly + FR_Q_HALO][tx + FR_Q_HALO], yv = sy[ly + FR_Q_HALO][tx + FR_Q_HALO];
		l1_sum += fabsf(xv - yv); // fp32, the arithmetic of k_l1_ssim_fwd
		const double d = (double)xv - (double)yv; // exact, and so is its square's sum up to the double roundings
		sq_sum += d * d;
	}
	// workgroup sums, in a fixed order
#pragma unroll
	for (int off = 32; off > 0; off >>= 1)
	{
		l1_sum += __shfl_xor(l1_sum, off); ssim_sum += __shfl_xor(ssim_sum, off); sq_sum += __shfl_xor(sq_sum, off);
	}
	if ((tid & 63) == 0) { s_red[0][tid >> 6] = (double)ssim_sum; s_red[1][tid >> 6] = sq_sum; s_red[2][tid >> 6] = (double)l1_sum; }
	__syncthreads();
	if (tid < 3)
	{
		const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
		partials[3 * b + tid] = (s_red[tid][0] + s_red[tid][1]) + (s_red[tid][2] + s_red[tid][3]);
	}
}

// The tiles of `rows` consecutive groups of channels -> per_view[slot + r] = (ssim, psnr, l1, mse) of group r, one workgroup:
// every thread adds its stride of the group's partials in double, the 1024 sums are added in a fixed tree. accum (optional)
// += (ssim, psnr, l1, 1) per group: the meter's running sums and its view count, in double. One workgroup on one stream:
// the read-modify-write of accum needs no atomics, views are added in the order of the calls.
__global__ void __launch_bounds__(1024) k_quality_finish(int rows, long long blocks_per_row, double n, const double *__restrict__ partials,
	float *__restrict__ per_view, double *__restrict__ accum)
{
	__shared__ double s[3][1024];
	for (int r = 0; r < rows; r++)
	{
		const double *p = partials + 3 * (size_t)r * (size_t)blocks_per_row;
		double a = 0.0, b = 0.0, c = 0.0;
		for (long long i = threadIdx.x; i < blocks_per_row; i += 1024) { a += p[3 * i]; b += p[3 * i + 1]; c += p[3 * i + 2]; }
		s[0][threadIdx.x] = a; s[1][threadIdx.x] = b; s[2][threadIdx.x] = c;
		__syncthreads();
		for (int off = 512; off > 0; off >>= 1)
		{
			if ((int)threadIdx.x < off)
			{
				s[0][threadIdx.x] += s[0][threadIdx.x + off]; s[1][threadIdx.x] += s[1][threadIdx.x + off]; s[2][threadIdx.x] += s[2][threadIdx.x + off];
			}
			__syncthreads();
		}
		if (threadIdx.x == 0)
		{
			const double mse = s[1][0] / n;
			const float ssim = (float)(s[0][0] / n), psnr = (float)(20.0 * log10(1.0 / sqrt(mse))), l1 = (float)(s[2][0] / n);
			float *o = per_view + 4 * (size_t)r;
			o[0] = ssim; o[1] = psnr; o[2] = l1; o[3] = (float)mse;
			if (accum != nullptr)
			{
				accum[0] += (double)ssim; accum[1] += (double)psnr; accum[2] += (double)l1; accum[3] += 1.0;
			}
		}
		__syncthreads(); // s is reused by the next group
	}
}

static long long quality_blocks(int C, int H, int W)
{
	return (long long)C * ((H + FR_Q_TH - 1) / FR_Q_TH) * ((W + FR_Q_TW - 1) / FR_Q_TW);
}

static bool quality_sizes_ok(int C, int H, int W)
{
	return C > 0 && H > 0 && W > 0 && C <= 65535 && (H + FR_Q_TH - 1) / FR_Q_TH <= 65535 && quality_blocks(C, H, W) < (1ll << 31);
}

} // namespace fr

using namespace fr;

extern "C" int64_t fr_quality_blocks(int32_t C, int32_t H, int32_t W)
{
	return quality_sizes_ok(C, H, W) ? (int64_t)quality_blocks(C, H, W) : 0;
}

extern "C" int fr_quality_forward(int32_t C, int32_t H, int32_t W, int32_t with_ssim, const float *img, const float *target, double *partials,
	void *stream_)
{
	if (!quality_sizes_ok(C, H, W)) { set_error("quality_forward: bad sizes C=%d H=%d W=%d", C, H, W); return FR_ERR_INVALID; }
	if (!img || !target || !partials) { set_error("quality_forward: a required pointer is null"); return FR_ERR_INVALID; }
	if ((uintptr_t)partials & 7) { set_error("quality_forward: partials must be 8-byte aligned (it holds doubles)"); return FR_ERR_INVALID; }
	hipStream_t stream = (hipStream_t)stream_;
	const dim3 grid((W + FR_Q_TW - 1) / FR_Q_TW, (H + FR_Q_TH - 1) / FR_Q_TH, C);
	if (with_ssim) hipLaunchKernelGGL(k_quality_fwd<true>, grid, dim3(256), 0, stream, H, W, img, target, partials);
	else hipLaunchKernelGGL(k_quality_fwd<false>, grid, dim3(256), 0, stream, H, W, img, target, partials);
	return check_launch("quality_forward", stream, false);
}

extern "C" int fr_quality_finish(int32_t C, int32_t H, int32_t W, int32_t rows, const double *partials, float *per_view, int32_t slot,
	int32_t capacity, double *accum, void *stream_)
{
	if (!quality_sizes_ok(C, H, W)) { set_error("quality_finish: bad sizes C=%d H=%d W=%d", C, H, W); return FR_ERR_INVALID; }
	if (rows <= 0 || C % rows) { set_error("quality_finish: rows=%d does not divide C=%d", rows, C); return FR_ERR_INVALID; }
	if (slot < 0 || capacity < 0 || (int64_t)slot + rows > capacity) { set_error("quality_finish: slots %d..%d are outside the array of %d", slot, slot + rows - 1, capacity); return FR_ERR_INVALID; }
	if (!partials || !per_view) { set_error("quality_finish: a required pointer is null"); return FR_ERR_INVALID; }
	if (((uintptr_t)partials & 7) || ((uintptr_t)accum & 7)) { set_error("quality_finish: partials and accum must be 8-byte aligned (they hold doubles)"); return FR_ERR_INVALID; }
	hipStream_t stream = (hipStream_t)stream_;
	const long long bpr = quality_blocks(C / rows, H, W);
	hipLaunchKernelGGL(k_quality_finish, dim3(1), dim3(1024), 0, stream, rows, bpr, (double)(C / rows) * H * W, partials, per_view + 4 * (size_t)slot, accum);
	return check_launch("quality_finish", stream, false);
}
