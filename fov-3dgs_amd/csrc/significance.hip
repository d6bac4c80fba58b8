// fovraster -- LightGaussian's global-significance pruning (the models of the multi-model baseline, MMFR): what follows the
// counting render (render.hip, FR_VARIANT_COUNT) and the order statistic (prune.hip, fr_select_kth).
//
// Reference (LightGaussian/): prune.py:112-128 calculate_v_imp_score -- torch.prod, a full descending torch.sort for ONE
// element, a division, torch.pow and a product, five passes over all P rows -- and scene/gaussian_model.py:776-782
// prune_gaussians -- a second full torch.sort for one element, a comparison, then prune_points. Here:
//   k_volume          volume[i] = (s0 * s1) * s2, each product rounded once (torch.prod over dim 1); raw: s = exp(raw) first
//   k_v_importance    out[i] = powf(volume[i] / *kth, v_pow) * imp[i], the threshold read from device memory
//   k_mask_le         mask[i] = values[i] <= *threshold (IEEE for fp32: a NaN row is never pruned; int32 for the counts)
// All on the caller's stream, no atomics, no host round trip: every output is one bit pattern, run after run. The rows the
// mask marks are cut by the row compaction of prune.hip.
#include "common.h"

// the score must round exactly as written: no contraction, a correctly rounded division
#pragma clang fp contract(off)

namespace fr {

static unsigned sig_grid(int P) { return (unsigned)(((int64_t)P + 255) / 256); }

template <bool RAW>
__global__ void __launch_bounds__(256) k_volume(int P, const float *__restrict__ scaling, float *__restrict__ volume)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)P) return;
	float s0 = scaling[3 * i], s1 = scaling[3 * i + 1], s2 = scaling[3 * i + 2];
	if (RAW) { s0 = act_scale(s0); s1 = act_scale(s1); s2 = act_scale(s2); }
	volume[i] = (s0 * s1) * s2;
}

// (out may be volume: every thread reads its own row before it writes it)
__global__ void __launch_bounds__(256) k_v_importance(int P, const float *volume, const float *__restrict__ kth_volume, float v_pow,
	const float *__restrict__ imp, float *out)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)P) return;
	const float ratio = volume[i] / kth_volume[0];
	out[i] = powf(ratio, v_pow) * imp[i];
}

template <typename T>
__global__ void __launch_bounds__(256) k_mask_le(int P, const T *__restrict__ values, const T *__restrict__ threshold, uint8_t *__restrict__ mask)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)P) return;
	mask[i] = values[i] <= threshold[0] ? 1 : 0;
}

int launch_volume(int P, const float *scaling, int raw, float *volume, hipStream_t stream)
{
	if (raw) hipLaunchKernelGGL(k_volume<true>, dim3(sig_grid(P)), dim3(256), 0, stream, P, scaling, volume);
	else hipLaunchKernelGGL(k_volume<false>, dim3(sig_grid(P)), dim3(256), 0, stream, P, scaling, volume);
	return check_launch("volume", stream, false);
}

int launch_v_importance(int P, const float *volume, const float *kth_volume, float v_pow, const float *imp, float *out, hipStream_t stream)
{
	hipLaunchKernelGGL(k_v_importance, dim3(sig_grid(P)), dim3(256), 0, stream, P, volume, kth_volume, v_pow, imp, out);
	return check_launch("v_importance", stream, false);
}

int launch_mask_le(int P, const void *values, int dtype, const void *threshold, uint8_t *mask, hipStream_t stream)
{
	if (dtype == 1) hipLaunchKernelGGL(k_mask_le<int32_t>, dim3(sig_grid(P)), dim3(256), 0, stream, P, (const int32_t *)values, (const int32_t *)threshold, mask);
	else hipLaunchKernelGGL(k_mask_le<float>, dim3(sig_grid(P)), dim3(256), 0, stream, P, (const float *)values, (const float *)threshold, mask);
	return check_launch("mask_le", stream, false);
}

} // namespace fr
