// fovraster -- what the two metameric (HVS) losses share: csrc/hvs.hip (uniform pooling) and csrc/hvs_fov.hip (gaze-dependent
// pooling). The device helpers, the argument structures of the kernels both use, and host launchers of those kernels: the
// kernels themselves (the pyramid, its backward pass, the resize's adjoint, the final sum) are compiled once, in hvs.hip.
#pragma once
#include "common.h"

namespace fr {

#define HVS_T 16
#define HVS_LP (HVS_T + 4)
#define HVS_IM (HVS_T + 8)
#define HVS_MAXB 8
#define HVS_MAXL 6
#define HVS_VAR_FLOOR 1e-7

// ---------------------------------------------------------------- device helpers
__device__ __forceinline__ int hvs_reflect(int i, int n)
{
	if (i < 0) i = -i;
	if (i >= n) i = 2 * (n - 1) - i;
	return min(max(i, 0), n - 1); // (only positions no output uses get here out of range)
}

struct HvsLerp { int i0, i1; double l0, l1; };

// upsample_bilinear2d, align_corners=False: src = scale (d + .5) - .5, negative -> 0
__device__ __forceinline__ HvsLerp hvs_lerp(int d, double scale, int n_in)
{
	double src = scale * ((double)d + 0.5) - 0.5;
	if (src < 0.0) src = 0.0;
	HvsLerp r;
	r.i0 = min((int)src, n_in - 1);
	r.i1 = r.i0 + (r.i0 < n_in - 1 ? 1 : 0);
	r.l1 = src - (double)r.i0; r.l0 = 1.0 - r.l1;
	return r;
}

__device__ __forceinline__ double hvs_bilerp(const float *__restrict__ a, int pw, const HvsLerp &y, const HvsLerp &x)
{
	return y.l0 * (x.l0 * (double)a[y.i0 * pw + x.i0] + x.l1 * (double)a[y.i0 * pw + x.i1])
		+ y.l1 * (x.l0 * (double)a[y.i1 * pw + x.i0] + x.l1 * (double)a[y.i1 * pw + x.i1]);
}

// The statistics are evaluated in double (gfx950 runs vector fp64 at the fp32 rate; these kernels wait for memory): the L1 loss
// takes sign(a - b) of two statistics that can differ by less than an fp32 evaluation resolves (the reference's fp32 statistics
// are ~3e-9 rms off the float64 ones), and ONE flipped sign moves dL/dimage by ~1e-3 of its maximum.
struct HvsStat { double mean, std, var; };

__device__ __forceinline__ HvsStat hvs_stat(const float *__restrict__ pm, const float *__restrict__ pq, int pw, const HvsLerp &y, const HvsLerp &x)
{
	HvsStat s;
	s.mean = hvs_bilerp(pm, pw, y, x);
	s.var = hvs_bilerp(pq, pw, y, x) - s.mean * s.mean;
	s.std = sqrt(s.var < HVS_VAR_FLOOR ? HVS_VAR_FLOOR : s.var);
	return s;
}

__device__ __forceinline__ float hvs_dabs(double d, int mse) { return mse ? (float)(2.0 * d) : (d > 0.0 ? 1.0f : (d < 0.0 ? -1.0f : 0.0f)); }

__device__ __forceinline__ double hvs_block_sum(double v, double *s_red)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
	if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
	__syncthreads();
	return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// d loss / d (mean, mean-square) at one full-resolution pixel of one map
__device__ __forceinline__ void hvs_pix_grad(const HvsStat &A, const HvsStat &B, int mse, float wgt, float &dmean, float &dmsq)
{
	dmean = wgt * hvs_dabs(A.mean - B.mean, mse);
	dmsq = 0.0f;
	if (!(A.var < HVS_VAR_FLOOR))
	{
		dmsq = (float)((double)(wgt * hvs_dabs(A.std - B.std, mse)) / (2.0 * A.std));
		dmean = (float)((double)dmean - 2.0 * A.mean * (double)dmsq);
	}
}

// ---------------------------------------------------------------- the kernels both losses launch (defined in hvs.hip)
struct HvsLevelArgs
{
	int h, w, nb, level0, rgb;
	const float *src[2]; float *ws[2];
	long long low_in, maps, low_out;
	const float *filt;
	int hs, wsrc;                                // RESIZED: the pictures are [3,hs,wsrc], sampled at scale ry = hs / h, rx = wsrc / w
	double ry, rx;
};

// gpool: the uniform loss's pooled gradients [2,nmc,ph,pw]; for the foveated loss (the kernels' FOV instantiation) the finished
// gradient of every map [nmc,h,w], and ph, pw, identity, wst and maps are unused
struct HvsGArgs { int h, w, ph, pw, nmc, mse, identity; float wgt; const float *wsi, *wst; long long maps; const float *gpool; };

struct HvsBwdLevelArgs
{
	HvsGArgs g;
	int nb, m0, last, pad;
	float wres;
	const float *filt, *glow_next, *low_i, *low_t;
	float *glow;
};

struct HvsBwdImageArgs { HvsGArgs g; int rgb, pad; const float *filt, *glow0, *gscale; float *dimg; };

struct HvsBwdResizeArgs { int h, w, hs, wsrc; double ry, rx; const float *g, *gscale; float *dimg; };

// grid: (tiles x, tiles y, 3 * sides); resized: the level-0 load samples the [3,hs,wsrc] pictures
void hvs_launch_level(bool resized, dim3 grid, hipStream_t stream, const HvsLevelArgs &a);
// fov: the maps' gradients are read from a.g.gpool [nmc,h,w] instead of being gathered from the pooling windows
void hvs_launch_bwd_level(bool fov, dim3 grid, hipStream_t stream, const HvsBwdLevelArgs &a);
void hvs_launch_bwd_image(bool fov, dim3 grid, hipStream_t stream, const HvsBwdImageArgs &a);
void hvs_launch_bwd_resize(hipStream_t stream, const HvsBwdResizeArgs &a);
// sum of |x - y| or (x - y)^2 over n elements times wgt -> partials[ceil(n / 1024)]
void hvs_launch_cmp_direct(hipStream_t stream, const float *x, const float *y, long long n, int mse, float wgt, float *partials);
void hvs_launch_finish(hipStream_t stream, int n, const float *partials, float *out);
int hvs_resize_check(int Hs, int Ws, int H, int W);

} // namespace fr
