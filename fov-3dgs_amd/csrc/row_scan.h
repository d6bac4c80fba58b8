// Row tiles and the workgroup prefix sum shared by the kernels that cut rows out of the per-Gaussian tensors (prune.hip) and
// that add rows to them (densify.hip).
#pragma once
#include "common.h"

namespace fr {

#define PRUNE_TILE 1024      // rows per tile: 256 threads x 4 consecutive rows (one 16-byte load of metrics, one 4-byte load / store of mask)
#define PRUNE_PER_THREAD 4
#define PRUNE_SCAN_CHUNK 256 // tiles k_prune_scan takes per round (one per thread), a carry runs from round to round

// exclusive prefix sum over the 256 threads of a workgroup (s_w: 4 words of LDS); *total gets the sum
__device__ __forceinline__ uint32_t prune_block_scan(uint32_t v, uint32_t *s_w, uint32_t *total)
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

} // namespace fr
