// fovraster -- densification: the steps of the training loop that ADD rows to the model, its Adam moments and `indexes`.
//
// Reference (fov3dgs/scene/gaussian_model.py): cat_tensors_to_optimizer / densification_postfix (:666-706), densify_and_clone
// and densify_and_split (:731-755, :803-818), densify_and_prune (:820-834), Fov-3DGS's idx_ / scale_ / big_size splits and
// position_grad_densify (:709-729, :757-801, :836-851), add_densification_stats (:865-867). densify_and_prune rewrites the
// whole training state four times (cat for the clones, cat for the children, prune_points for the split parents, prune_points
// for the opacity / size cut), with a nonzero and a host synchronisation per tensor[mask] and per .sum().
//
// Here every decision is taken per SOURCE row, so the sequence is one plan (class byte per row, per-tile counts, their
// running sums) and one pass over the state. Contract (include/fovraster.h) -- the layout of every output:
//   kept originals | surviving clones | surviving children of copy 0 | ... | of copy N - 1, each in index order,
// and child c of the r-th split row (r over ALL split rows in index order) reads noise[c * n_split + r].
//
// Two quirks of the reference's densify_and_prune are kept:
//   - densification_postfix zeroes max_radii2D before the final cut, so `max_radii2D > max_screen_size` is false for every
//     non-negative max_screen_size: the argument only switches the world-size test on;
//   - clones carry padded_grad 0 and are small, so they are never split.
//
// Kernels, all on the caller's stream, integer atomics nowhere (the tile totals come out of the workgroup prefix sum),
// cross-workgroup totals as plain stores that the next kernel consumes, no allocation, one bit pattern run after run:
//   k_densify_stats     accum += |grad.xy|, denom += 1 where the filter is set
//   k_densify_classify  class byte of every row (padded with zeros to whole tiles) and each tile's rows per segment
//   k_densify_scan      workgroup s: exclusive running sum of segment s over the tiles, and its total
//   k_densify_rows      grid (tiles, tensors): a tile's rows of each segment go to LDS in index order and leave as consecutive
//                       words to 2 + N destination runs; the children of the xyz and scaling tensors are computed, staged in
//                       LDS and leave the same way
#include "common.h"
#include "row_scan.h"

// the children's arithmetic rounds as written
#pragma clang fp contract(off)

namespace fr {

#define DENSIFY_KEEP 1u   // class bits
#define DENSIFY_CLONE 2u
#define DENSIFY_SPLIT 4u
#define DENSIFY_CHILD 8u
#define DENSIFY_SEGMENTS 4 // running sums per tile: kept originals, surviving clones, split rows, surviving children (per copy)

struct DensifyLayout {
	size_t bytes;
	size_t cls, first; // byte offsets
	int64_t tiles;
};

static DensifyLayout densify_layout(int64_t P)
{
	DensifyLayout L{};
	L.tiles = (P + PRUNE_TILE - 1) / PRUNE_TILE;
	size_t o = 0;
	L.cls = o;   o = align_up(o + (size_t)L.tiles * PRUNE_TILE);                                  // one byte per row, whole tiles
	L.first = o; o = align_up(o + (size_t)DENSIFY_SEGMENTS * L.tiles * sizeof(uint32_t));        // [segment][tile]
	L.bytes = o;
	return L;
}

size_t densify_workspace_bytes(int P) { return P > 0 ? densify_layout(P).bytes : 0; }

// ---- statistics ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_densify_stats(int P, const float *__restrict__ grad, const uint8_t *__restrict__ filter,
	float *__restrict__ accum, float *__restrict__ denom)
{
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * 256)
	{
		if (!filter[i]) continue;
		const float gx = grad[3 * i], gy = grad[3 * i + 1];
		accum[i] += sqrtf(gx * gx + gy * gy);
		denom[i] += 1.0f;
	}
}

// ---- plan ------------------------------------------------------------------------------------------------------------
struct DensifyPlan {
	int P, mode, use_world, n_grad;
	float max_grad, min_opacity, t_dense, t_world, child_div;
	const float *accum, *denom, *scaling, *opacity;
	const uint8_t *mask;
	uint8_t *cls;     // [tiles * PRUNE_TILE]
	uint32_t *first;  // [DENSIFY_SEGMENTS][tiles]
	int64_t tiles;
};

__device__ __forceinline__ uint32_t densify_class(const DensifyPlan &p, size_t i)
{
	bool clone = false, split = false, dead = false, child_dead = false;
	if (p.mode == FR_DENSIFY_CLONE_MASK) clone = p.mask[i] != 0;
	else if (p.mode == FR_DENSIFY_SPLIT_MASK) split = p.mask[i] != 0;
	else
	{
		float g = 0.0f;
		if (i < (size_t)p.n_grad)
		{
			g = p.accum[i];
			if (p.denom) { g = g / p.denom[i]; if (g != g) g = 0.0f; }
		}
		const float s0 = expf(p.scaling[3 * i]), s1 = expf(p.scaling[3 * i + 1]), s2 = expf(p.scaling[3 * i + 2]);
		const float smax = fmaxf(fmaxf(s0, s1), s2);
		if (p.mode != FR_DENSIFY_SPLIT_GRAD) clone = fabsf(g) >= p.max_grad && smax <= p.t_dense;
		if (p.mode != FR_DENSIFY_CLONE_GRAD) split = g >= p.max_grad && smax > p.t_dense;
		if (p.mode == FR_DENSIFY_AND_PRUNE)
		{
			const bool faint = act_opacity(p.opacity[i]) < p.min_opacity;
			const float cmax = fmaxf(fmaxf(expf(logf(s0 / p.child_div)), expf(logf(s1 / p.child_div))), expf(logf(s2 / p.child_div)));
			dead = faint || (p.use_world && smax > p.t_world);
			child_dead = faint || (p.use_world && cmax > p.t_world);
		}
	}
	return (!split && !dead ? DENSIFY_KEEP : 0u) | (clone && !dead ? DENSIFY_CLONE : 0u) | (split ? DENSIFY_SPLIT : 0u) |
		(split && !child_dead ? DENSIFY_CHILD : 0u);
}

// Thread t takes rows t, t + 256, ... of its tile (the loads of consecutive lanes are consecutive rows); the class bytes of
// the rows past P, up to the end of the last tile, are written as 0, so k_densify_rows reads whole words without a tail.
__global__ void __launch_bounds__(256) k_densify_classify(const DensifyPlan p)
{
	__shared__ uint32_t s_w[4];
	const int t = threadIdx.x;
	uint32_t v0 = 0, v1 = 0; // (kept | clones << 16), (split | children << 16): a tile has at most 1024 of each
#pragma unroll
	for (int j = 0; j < PRUNE_PER_THREAD; j++)
	{
		const size_t i = (size_t)blockIdx.x * PRUNE_TILE + (size_t)j * 256 + t;
		const uint32_t c = i < (size_t)p.P ? densify_class(p, i) : 0u;
		p.cls[i] = (uint8_t)c;
		v0 += (c & 1u) + ((c >> 1 & 1u) << 16);
		v1 += (c >> 2 & 1u) + ((c >> 3 & 1u) << 16);
	}
	uint32_t tot0, tot1;
	prune_block_scan(v0, s_w, &tot0);
	prune_block_scan(v1, s_w, &tot1);
	if (t == 0)
	{
		p.first[0 * p.tiles + blockIdx.x] = tot0 & 0xffffu;
		p.first[1 * p.tiles + blockIdx.x] = tot0 >> 16;
		p.first[2 * p.tiles + blockIdx.x] = tot1 & 0xffffu;
		p.first[3 * p.tiles + blockIdx.x] = tot1 >> 16;
	}
}

// Workgroup s: vals[s][i] -> sum of vals[s][0 .. i) in place, PRUNE_SCAN_CHUNK tiles per round; totals[s] gets the sum.
__global__ void __launch_bounds__(256) k_densify_scan(int64_t n, uint32_t *__restrict__ first, int32_t *__restrict__ totals)
{
	__shared__ uint32_t s_w[4];
	uint32_t *__restrict__ vals = first + (size_t)blockIdx.x * n;
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
	if (threadIdx.x == 0) totals[blockIdx.x] = (int32_t)carry;
}

// ---- rows ------------------------------------------------------------------------------------------------------------
struct DensifyTensor { const uint32_t *src; uint32_t *dst; uint32_t row_words, role; };
struct DensifyTable {
	int P, N;
	uint32_t n_keep, n_clone, n_split, n_child;
	float child_div;
	const uint32_t *cls;   // the class bytes, four rows per word
	const uint32_t *first; // [DENSIFY_SEGMENTS][tiles]
	int64_t tiles;
	const float *scaling, *rotation, *noise;
	DensifyTensor t[FR_COMPACT_MAX_TENSORS];
};

// n rows of W words, rows[j] = the tile row that output row j copies: word e of the run is word e % W of row e / W, so
// consecutive lanes write consecutive words and read runs of W consecutive words
__device__ __forceinline__ void densify_copy_run(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, const uint16_t *rows,
	uint32_t n, uint32_t W, int t)
{
	const uint64_t total = (uint64_t)n * W;
	const uint32_t dj = 256u / W, dc = 256u % W; // what 256 words further means in (row, word) terms
	uint32_t j = (uint32_t)t / W, c = (uint32_t)t % W;
	for (uint64_t e = t; e < total; e += 256)
	{
		dst[e] = src[(size_t)rows[j] * W + c];
		j += dj; c += dc;
		if (c >= W) { c -= W; j++; }
	}
}

// Workgroup (x, y): tile x of tensor y. The tile's kept, cloned and child-bearing rows go to three LDS lists in index order
// (with each child-bearing row's rank among the tile's split rows); each list's rows are consecutive in its destination
// segment, from the tile's running sum on. A destination row beyond its segment's total is not written.
__global__ void __launch_bounds__(256) k_densify_rows(const DensifyTable p)
{
	__shared__ uint32_t s_w[4];
	__shared__ uint16_t s_keep[PRUNE_TILE], s_clone[PRUNE_TILE], s_child[PRUNE_TILE], s_rank[PRUNE_TILE];
	__shared__ uint32_t s_val[3 * PRUNE_TILE];
	const DensifyTensor ten = p.t[blockIdx.y];
	const uint32_t W = ten.row_words; // > 0: the launcher leaves zero-width tensors out
	const int t = threadIdx.x;
	const size_t tile = blockIdx.x, row0 = tile * PRUNE_TILE;
	const uint32_t c4 = p.cls[row0 / PRUNE_PER_THREAD + t];
	uint32_t v0 = 0, v1 = 0;
#pragma unroll
	for (int j = 0; j < PRUNE_PER_THREAD; j++)
	{
		const uint32_t c = c4 >> (8 * j);
		v0 += (c & 1u) + ((c >> 1 & 1u) << 16);
		v1 += (c >> 2 & 1u) + ((c >> 3 & 1u) << 16);
	}
	uint32_t tot0, tot1;
	const uint32_t at0 = prune_block_scan(v0, s_w, &tot0), at1 = prune_block_scan(v1, s_w, &tot1);
	uint32_t a_keep = at0 & 0xffffu, a_clone = at0 >> 16, a_split = at1 & 0xffffu, a_child = at1 >> 16;
#pragma unroll
	for (int j = 0; j < PRUNE_PER_THREAD; j++)
	{
		const uint32_t c = c4 >> (8 * j);
		const uint16_t r = (uint16_t)(t * PRUNE_PER_THREAD + j);
		if (c & DENSIFY_KEEP) s_keep[a_keep++] = r;
		if (c & DENSIFY_CLONE) s_clone[a_clone++] = r;
		if (c & DENSIFY_CHILD) { s_child[a_child] = r; s_rank[a_child] = (uint16_t)a_split; a_child++; }
		if (c & DENSIFY_SPLIT) a_split++;
	}
	__syncthreads();
	const uint32_t *__restrict__ src = ten.src + row0 * W;
	// kept originals
	{
		const uint32_t base = p.first[0 * p.tiles + tile], n = tot0 & 0xffffu;
		if (base < p.n_keep) densify_copy_run(src, ten.dst + (size_t)base * W, s_keep, min(n, p.n_keep - base), W, t);
	}
	// surviving clones
	{
		const uint32_t base = p.first[1 * p.tiles + tile], n = tot0 >> 16;
		if (base < p.n_clone)
		{
			const uint32_t n_out = min(n, p.n_clone - base);
			uint32_t *__restrict__ dst = ten.dst + ((size_t)p.n_keep + base) * W;
			if (ten.role == FR_DENSIFY_ZERO_NEW)
				for (uint64_t e = t; e < (uint64_t)n_out * W; e += 256) dst[e] = 0u;
			else densify_copy_run(src, dst, s_clone, n_out, W, t);
		}
	}
	// surviving children, copy by copy (everything below is uniform over the workgroup)
	const uint32_t base = p.first[3 * p.tiles + tile];
	if (base >= p.n_child) return;
	const uint32_t n_out = min(tot1 >> 16, p.n_child - base);
	if (n_out == 0) return;
	const uint32_t rank0 = p.first[2 * p.tiles + tile];
	const bool computed = ten.role == FR_DENSIFY_XYZ || ten.role == FR_DENSIFY_SCALING; // (W == 3: the entry point checks)
	for (int c = 0; c < p.N; c++)
	{
		uint32_t *__restrict__ dst = ten.dst + ((size_t)p.n_keep + p.n_clone + (size_t)c * p.n_child + base) * W;
		if (ten.role == FR_DENSIFY_ZERO_NEW)
		{
			for (uint64_t e = t; e < (uint64_t)n_out * W; e += 256) dst[e] = 0u;
			continue;
		}
		if (!computed) { densify_copy_run(src, dst, s_child, n_out, W, t); continue; }
		if (ten.role == FR_DENSIFY_XYZ || c == 0) // (the children's scaling is the same for every copy)
		{
			if (c > 0) __syncthreads(); // the previous copy's values have left
			for (uint32_t j = t; j < n_out; j += 256)
			{
				const size_t i = row0 + s_child[j];
				const float r0 = p.scaling[3 * i], r1 = p.scaling[3 * i + 1], r2 = p.scaling[3 * i + 2];
				float o0, o1, o2;
				if (ten.role == FR_DENSIFY_SCALING)
				{
					o0 = logf(expf(r0) / p.child_div); o1 = logf(expf(r1) / p.child_div); o2 = logf(expf(r2) / p.child_div);
				}
				else
				{
					const uint32_t r = rank0 + s_rank[j];
					float z0 = 0.0f, z1 = 0.0f, z2 = 0.0f;
					if (r < p.n_split)
					{
						const float *__restrict__ z = p.noise + 3 * ((size_t)c * p.n_split + r);
						z0 = z[0]; z1 = z[1]; z2 = z[2];
					}
					const float s0 = expf(r0) * z0, s1 = expf(r1) * z1, s2 = expf(r2) * z2;
					// build_rotation (utils/general_utils.py:78-99)
					const float qr = p.rotation[4 * i], qx = p.rotation[4 * i + 1], qy = p.rotation[4 * i + 2], qz = p.rotation[4 * i + 3];
					const float norm = sqrtf(qr * qr + qx * qx + qy * qy + qz * qz);
					const float w = qr / norm, x = qx / norm, y = qy / norm, z_ = qz / norm;
					const float R00 = 1.0f - 2.0f * (y * y + z_ * z_), R01 = 2.0f * (x * y - w * z_), R02 = 2.0f * (x * z_ + w * y);
					const float R10 = 2.0f * (x * y + w * z_), R11 = 1.0f - 2.0f * (x * x + z_ * z_), R12 = 2.0f * (y * z_ - w * x);
					const float R20 = 2.0f * (x * z_ - w * y), R21 = 2.0f * (y * z_ + w * x), R22 = 1.0f - 2.0f * (x * x + y * y);
					const float *__restrict__ m = (const float *)ten.src + 3 * i;
					o0 = (R00 * s0 + R01 * s1) + R02 * s2 + m[0];
					o1 = (R10 * s0 + R11 * s1) + R12 * s2 + m[1];
					o2 = (R20 * s0 + R21 * s1) + R22 * s2 + m[2];
				}
				s_val[3 * j] = __float_as_uint(o0); s_val[3 * j + 1] = __float_as_uint(o1); s_val[3 * j + 2] = __float_as_uint(o2);
			}
			__syncthreads();
		}
		for (uint32_t e = t; e < 3 * n_out; e += 256) dst[e] = s_val[e];
	}
}

// ---- launchers -------------------------------------------------------------------------------------------------------
int launch_densify_stats(int P, const float *grad, const uint8_t *filter, float *accum, float *denom, hipStream_t stream)
{
	const int64_t b = ((int64_t)P + 255) / 256;
	hipLaunchKernelGGL(k_densify_stats, dim3((unsigned)(b < 4096 ? b : 4096)), dim3(256), 0, stream, P, grad, filter, accum, denom);
	return check_launch("densify_stats", stream, false);
}

int launch_densify_plan(const fr_densify_plan_args *a, hipStream_t stream)
{
	const DensifyLayout L = densify_layout(a->P);
	DensifyPlan p;
	p.P = a->P; p.mode = a->mode; p.use_world = a->use_world_size; p.n_grad = a->n_grad;
	p.max_grad = a->max_grad; p.min_opacity = a->min_opacity; p.t_dense = a->t_dense; p.t_world = a->t_world;
	p.child_div = 0.8f * (float)a->N;
	p.accum = a->accum; p.denom = a->denom; p.scaling = a->scaling; p.opacity = a->opacity; p.mask = a->mask;
	p.cls = (uint8_t *)a->workspace + L.cls;
	p.first = (uint32_t *)((char *)a->workspace + L.first);
	p.tiles = L.tiles;
	hipLaunchKernelGGL(k_densify_classify, dim3((unsigned)L.tiles), dim3(256), 0, stream, p);
	hipLaunchKernelGGL(k_densify_scan, dim3(DENSIFY_SEGMENTS), dim3(256), 0, stream, L.tiles, p.first, a->counts_out);
	return check_launch("densify_plan", stream, false);
}

int launch_densify_rows(const fr_densify_rows_args *a, hipStream_t stream)
{
	const DensifyLayout L = densify_layout(a->P);
	DensifyTable p;
	p.P = a->P; p.N = a->N;
	p.n_keep = (uint32_t)a->n_keep; p.n_clone = (uint32_t)a->n_clone; p.n_split = (uint32_t)a->n_split; p.n_child = (uint32_t)a->n_child;
	p.child_div = 0.8f * (float)a->N;
	p.cls = (const uint32_t *)((const char *)a->workspace + L.cls);
	p.first = (const uint32_t *)((const char *)a->workspace + L.first);
	p.tiles = L.tiles;
	p.scaling = a->scaling; p.rotation = a->rotation; p.noise = a->noise;
	int n = 0;
	for (int k = 0; k < a->num_tensors; k++)
	{
		const fr_densify_tensor &t = a->tensors[k];
		if (t.row_words == 0) continue; // zero-width rows: nothing to copy
		p.t[n].src = (const uint32_t *)t.src; p.t[n].dst = (uint32_t *)t.dst;
		p.t[n].row_words = (uint32_t)t.row_words; p.t[n].role = (uint32_t)t.role;
		n++;
	}
	if (n == 0) return FR_OK;
	for (int k = n; k < FR_COMPACT_MAX_TENSORS; k++) p.t[k] = DensifyTensor{nullptr, nullptr, 0u, 0u};
	hipLaunchKernelGGL(k_densify_rows, dim3((unsigned)L.tiles, (unsigned)n), dim3(256), 0, stream, p);
	return check_launch("densify_rows", stream, false);
}

} // namespace fr
