// fovraster -- two steps of the reference's efficiency-aware pruning loop (fov3dgs/prune.py) beside the metric pruning of
// prune.hip: the scale-decay loss of every training step and the opacity cap after every pruning round.
//
// Reference behaviour:
//   prune.py:257-261   scale_loss = (max(get_scaling, dim=1) * (gs_count - 4) * (gs_count > 4)).mean(): about eight
//                      elementwise / reduce kernels over all P rows, and their autograd graph.
//   fov3dgs/scene/gaussian_model.py:421-431, :447-452   reset_opacity / reset_opacity_max / reset_opacity_upper_bound:
//                      inverse_sigmoid(min(sigmoid(raw), max)), and :609-622 replace_tensor_to_optimizer: two zeros_like.
// Here the loss is one forward launch (per-workgroup sums in double) plus a one-workgroup finish in a fixed order (no float
// atomics: the same bits on every run) and one backward launch that reads the upstream gradient on the device; the cap is one
// launch that writes the new raw opacities and both zeroed Adam moments.
#include "common.h"

namespace fr {

#define FR_SD_THREADS 256

// the row's maximum and its column; ties go to the lowest column and a NaN wins, as torch.max(dim=1) documents
__device__ __forceinline__ float scale_row_max(const float *__restrict__ s, int raw, int *col)
{
	float m = s[0];
	int c = 0;
#pragma unroll
	for (int j = 1; j < 3; j++)
	{
		const float v = s[j];
		if (v > m || (v != v && m == m)) { m = v; c = j; }
	}
	*col = c;
	return raw ? expf(m) : m; // exp is monotone: the maximum of the log-scales is the row of the maximum scale
}

__global__ void __launch_bounds__(FR_SD_THREADS) k_scale_decay_fwd(int P, const float *__restrict__ scaling, const int32_t *__restrict__ counts,
	int threshold, int raw, double *__restrict__ partials)
{
	__shared__ double s_red[FR_SD_THREADS / 64];
	const long long i = (long long)blockIdx.x * FR_SD_THREADS + threadIdx.x;
	double term = 0.0;
	if (i < P)
	{
		const long long over = (long long)counts[i] - threshold;
		if (over > 0) // a row at or under the threshold adds exactly 0, whatever its scale
		{
			int col;
			term = (double)scale_row_max(scaling + 3 * i, raw, &col) * (double)over;
		}
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) term += __shfl_xor(term, off);
	if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = term;
	__syncthreads();
	if (threadIdx.x == 0) partials[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ void __launch_bounds__(1024) k_scale_decay_finish(int nblocks, double P, const double *__restrict__ partials, float *__restrict__ out)
{
	__shared__ double s[1024];
	double a = 0.0;
	for (int i = threadIdx.x; i < nblocks; i += 1024) a += partials[i];
	s[threadIdx.x] = a;
	__syncthreads();
	for (int off = 512; off > 0; off >>= 1)
	{
		if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
		__syncthreads();
	}
	if (threadIdx.x == 0) out[0] = (float)(s[0] / P);
}

// dL/dscaling [P,3], written in full: g (count - threshold)+ / P in the column of the maximum (times exp(raw) there when the
// input holds the log-scales), 0 elsewhere; g = *grad_scale, the upstream gradient as a device scalar, or 1.
__global__ void __launch_bounds__(FR_SD_THREADS) k_scale_decay_bwd(int P, const float *__restrict__ scaling, const int32_t *__restrict__ counts,
	int threshold, int raw, const float *__restrict__ grad_scale, float *__restrict__ dL_dscaling)
{
	const long long i = (long long)blockIdx.x * FR_SD_THREADS + threadIdx.x;
	if (i >= P) return;
	const double gs = grad_scale ? (double)*grad_scale : 1.0;
	const long long over = (long long)counts[i] - threshold;
	float g[3] = { 0.0f, 0.0f, 0.0f };
	if (over > 0)
	{
		int col;
		const float m = scale_row_max(scaling + 3 * i, raw, &col);
		const double d = gs * ((double)over / (double)P);
		g[col] = (float)(raw ? d * (double)m : d);
	}
	float *o = dL_dscaling + 3 * i;
	o[0] = g[0]; o[1] = g[1]; o[2] = g[2];
}

// out = cap_logit where sigmoid(raw) > max_opacity (fp32, the arithmetic of get_opacity), the input's bits elsewhere (a NaN
// compares false and stays); exp_avg = exp_avg_sq = 0 (either may be NULL: a group without Adam state).
__global__ void __launch_bounds__(256) k_opacity_cap(int P, const float *__restrict__ raw, float max_opacity, float cap_logit, float *__restrict__ out,
	float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i >= P) return;
	const float x = raw[i];
	const float o = 1.0f / (1.0f + expf(-x));
	out[i] = o > max_opacity ? cap_logit : x;
	if (exp_avg) exp_avg[i] = 0.0f;
	if (exp_avg_sq) exp_avg_sq[i] = 0.0f;
}

} // namespace fr

using namespace fr;

extern "C" int64_t fr_scale_decay_blocks(int32_t P)
{
	return P > 0 ? ((int64_t)P + FR_SD_THREADS - 1) / FR_SD_THREADS : 0;
}

extern "C" int fr_scale_decay_forward(int32_t P, const float *scaling, const int32_t *counts, int32_t threshold, int32_t raw, double *partials,
	float *out, void *stream_)
{
	if (P <= 0) { set_error("scale_decay_forward: bad size P=%d (the mean of no rows is undefined)", P); return FR_ERR_INVALID; }
	if (!scaling || !counts || !partials || !out) { set_error("scale_decay_forward: a required pointer is null"); return FR_ERR_INVALID; }
	if ((uintptr_t)partials & 7) { set_error("scale_decay_forward: partials must be 8-byte aligned (it holds doubles)"); return FR_ERR_INVALID; }
	hipStream_t stream = (hipStream_t)stream_;
	const int nb = (int)fr_scale_decay_blocks(P);
	hipLaunchKernelGGL(k_scale_decay_fwd, dim3(nb), dim3(FR_SD_THREADS), 0, stream, P, scaling, counts, threshold, raw != 0, partials);
	int rc = check_launch("scale_decay_forward", stream, false);
	if (rc != FR_OK) return rc;
	hipLaunchKernelGGL(k_scale_decay_finish, dim3(1), dim3(1024), 0, stream, nb, (double)P, partials, out);
	return check_launch("scale_decay_finish", stream, false);
}

extern "C" int fr_scale_decay_backward(int32_t P, const float *scaling, const int32_t *counts, int32_t threshold, int32_t raw, const float *grad_scale,
	float *dL_dscaling, void *stream_)
{
	if (P <= 0) { set_error("scale_decay_backward: bad size P=%d", P); return FR_ERR_INVALID; }
	if (!scaling || !counts || !dL_dscaling) { set_error("scale_decay_backward: a required pointer is null"); return FR_ERR_INVALID; }
	hipStream_t stream = (hipStream_t)stream_;
	hipLaunchKernelGGL(k_scale_decay_bwd, dim3((int)fr_scale_decay_blocks(P)), dim3(FR_SD_THREADS), 0, stream, P, scaling, counts, threshold, raw != 0,
		grad_scale, dL_dscaling);
	return check_launch("scale_decay_backward", stream, false);
}

extern "C" int fr_opacity_cap(int32_t P, const float *raw_opacity, float max_opacity, float cap_logit, float *out, float *exp_avg, float *exp_avg_sq,
	void *stream_)
{
	if (P < 0) { set_error("opacity_cap: bad size P=%d", P); return FR_ERR_INVALID; }
	if (!(max_opacity > 0.0f) || !(max_opacity < 1.0f)) { set_error("opacity_cap: max_opacity %g is not inside (0, 1)", (double)max_opacity); return FR_ERR_INVALID; }
	if (P == 0) return FR_OK;
	if (!raw_opacity || !out) { set_error("opacity_cap: a required pointer is null"); return FR_ERR_INVALID; }
	hipStream_t stream = (hipStream_t)stream_;
	hipLaunchKernelGGL(k_opacity_cap, dim3((unsigned)(((int64_t)P + 255) / 256)), dim3(256), 0, stream, P, raw_opacity, max_opacity, cap_logit, out, exp_avg, exp_avg_sq);
	return check_launch("opacity_cap", stream, false);
}
