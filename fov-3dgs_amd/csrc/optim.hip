// fovraster -- the optimizer step of a training iteration: Adam over every parameter tensor of the model in ONE launch.
//
// Reference behaviour (fov3dgs/scene/gaussian_model.py:289, torch.optim.Adam(l, lr=0.0, eps=1e-15), stepped by
// eff_finetune.py:147): per tensor, in torch's order of operations (torch/optim/adam.py, _single_tensor_adam),
//   m  = fma(1-b1, g - m, m)                 exp_avg.lerp_(grad, 1 - beta1)
//   v  = fma(1-b2, g g, b2 v)                exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//   d  = sqrt(v) / sqrt(1 - b2^t) + eps      (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
//   p += -(lr / (1 - b1^t)) (m / d)          param.addcdiv_(exp_avg, denom, value=-step_size)
// The two fused multiply-adds are where torch's own float32 GPU kernels fuse (ATen's lerp, and addcmul's a + alpha * (b * c)
// as the device compiler contracts it): with them both moments come out bit for bit as torch.optim.Adam's on the GPU
// (measured: 30 steps, every element of the six tensors). They are written out (fmaf): the library is built with
// -ffp-contract=off, so the compiler fuses nothing else, every other operation rounds once, and hipcc keeps fp32 division and
// sqrt correctly rounded. The arithmetic of an element therefore does not depend on the path (vector / scalar tail / sparse)
// that reached it. (torch's CPU kernels associate the second moment as fma((1-b2) g, g, b2 v): one rounding placed
// differently.) The bias corrections come from the host (double, per tensor).
//
// Three modes per tensor, one kernel: the work of all tensors is cut into chunks of ADAM_CHUNK elements, the chunk ->
// tensor lookup walks the (at most 16 entry) table that travels in the kernel arguments, a capped grid strides over the
// chunks. Purely HBM-bound: 16 B read and 12 B written per element, no LDS, no atomics.
//   dense: p, g, m, v as float4 where the four pointers are 16-byte aligned, scalar tail / scalar otherwise.
//   exact: the dense sweep over p, m, v; the gradient of row r is row pos of the compact [n, w] values when
//          rows[pos] == r and zero otherwise. pos comes from a 4 B / Gaussian inverse map (row_map, filled by a small kernel
//          in front of the step, never cleared: an entry is believed only if rows[entry] == r) or, without a map, from a
//          binary search in the increasing rows: one per chunk for its first compact row, then each lane within the
//          <= ADAM_CHUNK / w + 2 rows its chunk can hold. The search is a chain of ~21 dependent loads per chunk at 2 M rows
//          and runs at 2.1x the dense step's time (the map: 1.2x); the map is what optim.Adam uses (DESIGN.md has both numbers).
//   lazy:  the chunks run over the compact gradient: element e belongs to parameter element rows[e / w] * w + e % w.
//          Rows that are not listed are neither read nor written; a row outside [0, P) is skipped.
#include "common.h"

namespace fr {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_CHUNK = 1024;   // elements: one float4 per lane
constexpr int ADAM_MAX_BLOCKS = 2048; // 256 CUs x 8 workgroups

struct AdamTable
{
	fr_adam_tensor t[FR_ADAM_MAX_TENSORS];
	int64_t chunk_end[FR_ADAM_MAX_TENSORS]; // running sum of the tensors' chunk counts
	int32_t vec[FR_ADAM_MAX_TENSORS];       // dense / exact: p, m, v (and dense g) are 16-byte aligned
	int32_t n;
};

struct AdamCoef { float w1, b2, w2, bc2_sqrt, eps, neg_step; };

__device__ __forceinline__ void adam_update(const AdamCoef &c, float g, float &p, float &m, float &v)
{
	m = fmaf(c.w1, g - m, m);
	v = fmaf(c.w2, g * g, v * c.b2);
	const float d = sqrtf(v) / c.bc2_sqrt + c.eps;
	p = p + c.neg_step * (m / d);
}

// first position in rows[lo, hi) whose row is >= r
__device__ __forceinline__ int64_t lower_bound_rows(const int64_t *__restrict__ rows, int64_t lo, int64_t hi, int64_t r)
{
	while (lo < hi)
	{
		const int64_t mid = lo + ((hi - lo) >> 1);
		if (rows[mid] < r) lo = mid + 1; else hi = mid;
	}
	return lo;
}

__global__ void __launch_bounds__(ADAM_THREADS) k_adam(const AdamTable tab)
{
	const int64_t total = tab.chunk_end[tab.n - 1];
	int ti = 0;
	for (int64_t chunk = blockIdx.x; chunk < total; chunk += gridDim.x)
	{
		while (chunk >= tab.chunk_end[ti]) ti++; // (chunks only grow: the walk never restarts)
		const fr_adam_tensor &t = tab.t[ti];
		const int64_t local = chunk - (ti ? tab.chunk_end[ti - 1] : 0);
		const AdamCoef c = { t.one_minus_beta1, t.beta2, t.one_minus_beta2, t.bias_correction2_sqrt, t.eps, t.neg_step_size };
		float *__restrict__ P = t.param, *__restrict__ M = t.exp_avg, *__restrict__ V = t.exp_avg_sq;
		const float *__restrict__ G = t.grad;
		const int w = t.width;

		if (t.mode == FR_ADAM_LAZY)
		{
			const int64_t nel = t.n_rows * (int64_t)w, base = local * ADAM_CHUNK;
			const int64_t row0 = base / w;        // uniform: one 64-bit division per chunk
			const uint32_t col0 = (uint32_t)(base - row0 * w);
			const int64_t n_param_rows = t.numel / w;
#pragma unroll
			for (int k = 0; k < ADAM_CHUNK / ADAM_THREADS; k++)
			{
				const uint32_t o = (uint32_t)(k * ADAM_THREADS + threadIdx.x);
				const int64_t e = base + o;
				if (e >= nel) break;
				const uint32_t q = (col0 + o) / (uint32_t)w, col = (col0 + o) - q * (uint32_t)w;
				const int64_t r = t.rows[row0 + q];
				if (r < 0 || r >= n_param_rows) continue; // never dereferenced
				const int64_t i = r * w + col;
				float p = P[i], m = M[i], v = V[i];
				adam_update(c, G[e], p, m, v);
				P[i] = p; M[i] = m; V[i] = v;
			}
			continue;
		}

		const int64_t i0 = local * ADAM_CHUNK + (int64_t)threadIdx.x * 4;
		if (i0 >= t.numel) continue;
		const bool full = tab.vec[ti] && i0 + 4 <= t.numel;
		if (full && t.mode == FR_ADAM_DENSE) // the streaming case on its own: four 16-byte loads in flight, three stores
		{
			const float4 x = *(const float4 *)(G + i0);
			float4 p = *(float4 *)(P + i0), m = *(float4 *)(M + i0), v = *(float4 *)(V + i0);
			adam_update(c, x.x, p.x, m.x, v.x);
			adam_update(c, x.y, p.y, m.y, v.y);
			adam_update(c, x.z, p.z, m.z, v.z);
			adam_update(c, x.w, p.w, m.w, v.w);
			*(float4 *)(P + i0) = p; *(float4 *)(M + i0) = m; *(float4 *)(V + i0) = v;
			continue;
		}
		float g[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
		if (t.mode == FR_ADAM_DENSE)
		{
			for (int k = 0; k < 4; k++) if (i0 + k < t.numel) g[k] = G[i0 + k]; // tail, or a tensor that is not 16-byte aligned
		}
		else // FR_ADAM_EXACT
		{
			const int64_t cbase = local * ADAM_CHUNK;
			const int64_t rfirst = cbase / w; // uniform
			const int32_t *__restrict__ map = t.row_map;
			const int64_t *__restrict__ rows = t.rows;
			const int64_t n_rows = t.n_rows;
			int64_t lb = 0, hi = 0;
			if (!map)
			{
				int64_t clast = cbase + ADAM_CHUNK - 1;
				if (clast > t.numel - 1) clast = t.numel - 1;
				lb = lower_bound_rows(rows, 0, n_rows, rfirst); // uniform: the same walk in every lane
				hi = lb + (clast / w - rfirst + 1);             // the chunk's rows take at most that many compact positions
				if (hi > n_rows) hi = n_rows;
			}
			// compact position of row r, -1 when the row has no entry. The map is never cleared: an entry counts only if the
			// compact row it names is row r (whatever an earlier step or nobody at all left there fails that test)
			auto in_map = [&](int64_t r) -> int64_t {
				const uint32_t q = (uint32_t)map[r];
				return ((int64_t)q < n_rows && rows[q] == r) ? (int64_t)q : -1;
			};
			const uint32_t o = (uint32_t)(cbase - rfirst * w) + threadIdx.x * 4u; // < w + ADAM_CHUNK: 32-bit division per lane
			int64_t r = rfirst + o / (uint32_t)w;
			uint32_t col = o % (uint32_t)w;
			int64_t cur = map ? 0 : lower_bound_rows(rows, lb, hi, r); // search: first compact position whose row is >= r
			int64_t pos = map ? in_map(r) : (cur < hi && rows[cur] == r ? cur : -1);
#pragma unroll
			for (int k = 0; k < 4; k++)
			{
				if (i0 + k >= t.numel) break;
				if (pos >= 0) g[k] = G[pos * w + col];
				if (++col == (uint32_t)w && i0 + k + 1 < t.numel)
				{
					col = 0; r++;
					if (map) pos = in_map(r);
					else
					{
						if (pos >= 0) cur++; // rows are increasing: row r + 1 can only sit at the next position
						pos = cur < hi && rows[cur] == r ? cur : -1;
					}
				}
			}
		}
		if (full)
		{
			float4 p = *(float4 *)(P + i0), m = *(float4 *)(M + i0), v = *(float4 *)(V + i0);
			adam_update(c, g[0], p.x, m.x, v.x);
			adam_update(c, g[1], p.y, m.y, v.y);
			adam_update(c, g[2], p.z, m.z, v.z);
			adam_update(c, g[3], p.w, m.w, v.w);
			*(float4 *)(P + i0) = p; *(float4 *)(M + i0) = m; *(float4 *)(V + i0) = v;
		}
		else
			for (int k = 0; k < 4; k++)
				if (i0 + k < t.numel)
				{
					float p = P[i0 + k], m = M[i0 + k], v = V[i0 + k];
					adam_update(c, g[k], p, m, v);
					P[i0 + k] = p; M[i0 + k] = m; V[i0 + k] = v;
				}
	}
}

// row_map[rows[i]] = i for the rows inside [0, P): the exact mode's row -> compact position lookup (rows are unique: no two
// lanes write one entry)
__global__ void __launch_bounds__(ADAM_THREADS) k_adam_row_map(const int64_t *__restrict__ rows, int64_t n_rows, int64_t P, int32_t *__restrict__ map)
{
	for (int64_t i = (int64_t)blockIdx.x * ADAM_THREADS + threadIdx.x; i < n_rows; i += (int64_t)gridDim.x * ADAM_THREADS)
	{
		const int64_t r = rows[i];
		if (r >= 0 && r < P) map[r] = (int32_t)i;
	}
}

int launch_adam(const fr_adam_args *a, hipStream_t stream)
{
	// one map per call (fr_adam_step has checked that every tensor that names it shares rows, n_rows and row count)
	for (int k = 0; k < a->num_tensors; k++)
	{
		const fr_adam_tensor &t = a->tensors[k];
		if (t.mode != FR_ADAM_EXACT || !t.row_map || t.n_rows == 0 || t.numel == 0) continue;
		const int64_t blocks = (t.n_rows + ADAM_THREADS - 1) / ADAM_THREADS;
		hipLaunchKernelGGL(k_adam_row_map, dim3((unsigned)(blocks < ADAM_MAX_BLOCKS ? blocks : ADAM_MAX_BLOCKS)), dim3(ADAM_THREADS), 0, stream,
			t.rows, t.n_rows, t.numel / t.width, t.row_map);
		const int rc = check_launch("adam_row_map", stream, false);
		if (rc) return rc;
		break;
	}
	AdamTable tab = {};
	int64_t chunks = 0;
	int n = 0;
	for (int k = 0; k < a->num_tensors; k++)
	{
		const fr_adam_tensor &t = a->tensors[k];
		const int64_t work = t.mode == FR_ADAM_LAZY ? t.n_rows * (int64_t)t.width : t.numel;
		if (work == 0) continue; // an empty tensor, or a lazy step of a view that touched nothing
		chunks += (work + ADAM_CHUNK - 1) / ADAM_CHUNK;
		tab.t[n] = t;
		tab.chunk_end[n] = chunks;
		uintptr_t al = (uintptr_t)t.param | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq;
		if (t.mode == FR_ADAM_DENSE) al |= (uintptr_t)t.grad;
		tab.vec[n] = al % 16 == 0;
		n++;
	}
	if (n == 0) return FR_OK;
	tab.n = n;
	const unsigned grid = (unsigned)(chunks < ADAM_MAX_BLOCKS ? chunks : ADAM_MAX_BLOCKS);
	hipLaunchKernelGGL(k_adam, dim3(grid), dim3(ADAM_THREADS), 0, stream, tab);
	return check_launch("adam_step", stream, false);
}

} // namespace fr
