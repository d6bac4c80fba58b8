// fovraster -- the steerable pyramid's SYNTHESIS and the metamer built on it, fused: MetamerMSELoss.gen_metamer with
// avg_pooling_downup=True (the bilinear pyramid, the one csrc/hvs.hip analyses), the picture that MetamericLoss cannot tell from
// the target at a given gaze, and the L1 / MSE loss against it (include/fovraster.h: fr_hvs_metamer_*).
//
// Reference behaviour:
//   metamer/odak_perception/metamer_mse_loss.py:81-88   the target in YCrCb; its statistics maps (MetamericLoss.calc_statsmaps:
//                                                        blended mean and std per pixel of h and of every band; the variance
//                                                        floored at 1e-7, metameric_loss.py:107-109)
//                                       :89-93           noise = rand_like(target), its pyramid (the noise is NOT colour converted)
//                                       :97-107          match_level: level -= mean(level); level /= max(sqrt(mean(level^2)), 1e-6);
//                                                        level *= target_std; level += target_mean -- ONE mean and ONE root mean
//                                                        square per band, over all three channels
//                                       :109-116         h and every band of every level matched; the last lowpass is the target's
//                                       :118-123         reconstruct_from_pyramid, YCrCb -> RGB
//                                       :146-152         the loss: L1Loss / MSELoss (mean) between the image and the kept metamer
//   metamer/odak_perception/spatial_steerable_pyramid.py:182-223 image = last lowpass; per level, coarsest first: image = bilinear
//                                                        upsample (align_corners=False) to the level's size, image += conv(reflect-pad
//                                                        2 of band_b, -b_b) for b = 0 .. n-1 (F.conv2d: a correlation, no flip);
//                                                        then image = conv(pad(image), l0) + conv(pad(h), h0)
//   metamer/odak_perception/color_conversion.py:424-427 R = Y + 1.403 (Cr - .5), G = Y - .714 (Cr - .5) - .344 (Cb - .5),
//                                                        B = Y + 1.773 (Cb - .5)
//
// fr_hvs_metamer, everything on the caller's stream, in the caller's workspace:
//   k_fov_lod, k_hvs_level, k_fov_mip  (hvs_fov.hip, hvs.hip) the target's forward state exactly as the foveated loss keeps it: the
//                   LOD maps, the bands, the mip chains of every band and of its square. k_hvs_level once more for the noise.
//   k_met_sum       per band: the sum (or, second pass, the sum of squares of the values less the band's mean) of 1024 elements per
//                   workgroup, in double -> one partial per workgroup;
//   k_met_finish    one workgroup per band adds the partials in a fixed order -> the band's mean (first pass), its root mean
//                   square floored at 1e-6 (second pass). No atomics: the same bits on every run.
//   k_met_match     per pixel of every band: (noise - mean) / rms * std(y, x) + mean(y, x) in double, the target's blended
//                   statistics evaluated here (fov_stat), never written out as maps; in place over the noise's band.
//   k_met_level     per level, coarsest first, a 16x16 tile: the running image's bilinear sample (hvs_lerp, a gather from the
//                   coarser level) plus, band after band in the order 0 .. n-1, the 5x5 correlation with -b_b of the band's tile,
//                   staged in LDS with its 2-pixel halo, the reflection resolved at the load. Sums in double, one rounding.
//   k_met_final     l0 of the running image + h0 of the (matched) highpass residual, both from LDS tiles with the reflected halo,
//                   the three channels in one workgroup, then YCrCb -> RGB. No clamp: the reference's metamer leaves [0, 1] too.
// fr_hvs_metamer_roundtrip is the same synthesis from the picture's OWN pyramid (no noise, no statistics, no matching):
// reconstruct_from_pyramid(construct_pyramid(x)).
//
// The loss: k_met_loss sums |x - m| or (x - m)^2 in double, 4096 elements per workgroup in a fixed order, one partial per
// workgroup; the workgroup whose (integer) ticket is the last adds the partials in index order and writes the mean. One launch,
// no float atomics. k_met_loss_bwd is elementwise and reads the upstream gradient on the device.
#include "hvs_fov_common.h"

namespace fr {

#define MET_RMS_FLOOR 1e-6

struct MetPlan
{
	FovPlan f;
	int nbands;                                   // h and every band of every level
	long long n_maps[HVS_MAXL], n_low[HVS_MAXL];  // the noise's state: offsets (floats) of [nm,3,h,w] and of the next lowpass
	long long run[HVS_MAXL];                      // the running image of every level [3,h,w]
	int part_n;                                   // partial sums of one pass over the largest level
	// the workspace: doubles first (8-byte aligned), then floats
	long long d_lod, d_scal, d_part, n_doubles;   // offsets in doubles: LOD maps, [nbands][mean, rms], partials
	long long o_target, o_noise, o_run, floats;   // offsets in floats
};

static int met_band(const MetPlan &p, int l, int m) { return (l == 0 ? 0 : 1 + l * p.f.nb) + m; }

static int met_plan(int H, int W, int L, int nb, bool roundtrip, MetPlan *p)
{
	int rc = fov_plan("hvs_metamer", H, W, L, nb, &p->f);
	if (rc != FR_OK) return rc;
	p->nbands = 1 + (L - 1) * nb;
	long long ns = 0, nr = 0;
	for (int l = 0; l < L - 1; l++)
	{
		const long long plane = (long long)(H >> l) * (W >> l);
		p->n_maps[l] = ns; ns += (long long)p->f.lv[l].a.nmc * plane;
		p->n_low[l] = ns; ns += 3 * (plane / 4);
		p->run[l] = nr; nr += 3 * plane;
	}
	p->part_n = (int)((3ll * H * W + 1023) / 1024) * (nb + 1);
	p->d_lod = 0;
	p->d_scal = roundtrip ? 0 : p->f.lod_doubles;
	p->d_part = p->d_scal + (roundtrip ? 0 : 2 * p->nbands);
	p->n_doubles = p->d_part + (roundtrip ? 0 : p->part_n);
	p->o_target = 2 * p->n_doubles;
	p->o_noise = p->o_target + p->f.ws_floats;
	p->o_run = p->o_noise + (roundtrip ? 0 : ns);
	p->floats = p->o_run + nr;
	return FR_OK;
}

// ---------------------------------------------------------------- the band scalars
struct MetSumArgs { const float *maps; long long n; int centred; const double *scal; double *part; };

// band blockIdx.y = [3,h,w] = n contiguous floats; 1024 per workgroup
__global__ void __launch_bounds__(256) k_met_sum(MetSumArgs a)
{
	__shared__ double s_red[4];
	const float *x = a.maps + (size_t)blockIdx.y * a.n;
	const double mean = a.centred ? a.scal[2 * blockIdx.y] : 0.0;
	double acc = 0.0;
#pragma unroll
	for (int k = 0; k < 4; k++)
	{
		const long long i = (long long)blockIdx.x * 1024 + k * 256 + threadIdx.x;
		if (i < a.n) { const double d = (double)x[i] - mean; acc += a.centred ? d * d : d; }
	}
	const double t = hvs_block_sum(acc, s_red);
	if (threadIdx.x == 0) a.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// one workgroup per band: first pass scal[band][0] = mean; second pass scal[band][1] = max(sqrt(mean square), 1e-6)
__global__ void __launch_bounds__(1024) k_met_finish(int nblk, long long n, int centred, const double *__restrict__ part, double *__restrict__ scal)
{
	__shared__ double s0[1024];
	const double *p = part + (size_t)blockIdx.x * nblk;
	double a = 0.0;
	for (int i = threadIdx.x; i < nblk; i += 1024) a += p[i];
	s0[threadIdx.x] = a;
	__syncthreads();
	for (int off = 512; off > 0; off >>= 1)
	{
		if ((int)threadIdx.x < off) s0[threadIdx.x] += s0[threadIdx.x + off];
		__syncthreads();
	}
	if (threadIdx.x == 0)
	{
		const double m = s0[0] / (double)n;
		if (!centred) scal[2 * blockIdx.x] = m;
		else { const double r = sqrt(m); scal[2 * blockIdx.x + 1] = r < MET_RMS_FLOOR ? MET_RMS_FLOOR : r; }
	}
}

// ---------------------------------------------------------------- the match
struct MetMatchArgs { FovMaps a; const float *wst; float *band; const double *lod, *scal; };

__global__ void __launch_bounds__(256) k_met_match(MetMatchArgs a)
{
	const int pix = blockIdx.x * 256 + threadIdx.x, mc = blockIdx.y;
	if (pix >= a.a.h * a.a.w) return;
	const int y = pix / a.a.w, x = pix - y * a.a.w;
	const HvsStat T = fov_stat(a.wst, a.a, mc, y, x, fov_lod_of(a.lod, pix));
	const double *s = a.scal + 2 * (mc / 3);
	const size_t o = (size_t)mc * a.a.h * a.a.w + pix;
	a.band[o] = (float)((((double)a.band[o] - s[0]) / s[1]) * T.std + T.mean);
}

// ---------------------------------------------------------------- the synthesis
// a 16x16 tile of one channel of one band with its 2-pixel halo; reflection acts on the picture's coordinates
__device__ __forceinline__ void met_stage(float (*T)[HVS_LP + 1], const float *__restrict__ src, int by, int bx, int h, int w)
{
	for (int i = threadIdx.x; i < HVS_LP * HVS_LP; i += 256)
	{
		const int r = i / HVS_LP, c = i - r * HVS_LP;
		T[r][c] = src[(size_t)hvs_reflect(by + r - 2, h) * w + hvs_reflect(bx + c - 2, w)];
	}
}

// F.conv2d's correlation: sum_k f[ky][kx] x[y + ky - 2][x + kx - 2]; the filter is not flipped
__device__ __forceinline__ double met_corr(const float (*T)[HVS_LP + 1], const float *f, int ty, int tx)
{
	double t = 0.0;
#pragma unroll
	for (int ky = 0; ky < 5; ky++)
#pragma unroll
		for (int kx = 0; kx < 5; kx++) t += (double)f[ky * 5 + kx] * (double)T[ty + ky][tx + kx];
	return t;
}

struct MetLevelArgs { int h, w, nb, m0; const float *bands, *prev, *filt; float *out; };

// out[ch] = bilinear-up(prev[ch] of (h/2, w/2)) + sum_b corr(reflect-pad band_b[ch], -filt_b), b ascending
__global__ void __launch_bounds__(256) k_met_level(MetLevelArgs a)
{
	__shared__ float T[HVS_LP][HVS_LP + 1], F[HVS_MAXB * 25];
	const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, ch = blockIdx.z;
	const int bx = blockIdx.x * HVS_T, by = blockIdx.y * HVS_T, h = a.h, w = a.w;
	const int py = by + ty, px = bx + tx;
	const bool in = py < h && px < w;
	const size_t plane = (size_t)h * w;
	for (int i = tid; i < a.nb * 25; i += 256) F[i] = a.filt[50 + i];
	double acc = 0.0;
	if (in)
	{
		const int h2 = h >> 1, w2 = w >> 1;
		acc = hvs_bilerp(a.prev + (size_t)ch * h2 * w2, w2, hvs_lerp(py, (double)h2 / (double)h, h2), hvs_lerp(px, (double)w2 / (double)w, w2));
	}
	for (int b = 0; b < a.nb; b++)
	{
		__syncthreads();
		met_stage(T, a.bands + ((size_t)(a.m0 + b) * 3 + ch) * plane, by, bx, h, w);
		__syncthreads();
		if (in) acc -= met_corr(T, F + b * 25, ty, tx); // (+ corr with -f: the same number)
	}
	if (in) a.out[(size_t)ch * plane + (size_t)py * w + px] = (float)acc;
}

struct MetFinalArgs { int h, w, rgb; const float *run, *high, *filt; float *out; };

// out = l0 * run + h0 * high per channel, then YCrCb -> RGB (rgb = 0: the channels as they are)
__global__ void __launch_bounds__(256) k_met_final(MetFinalArgs a)
{
	__shared__ float T[HVS_LP][HVS_LP + 1], F[50];
	const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
	const int bx = blockIdx.x * HVS_T, by = blockIdx.y * HVS_T, h = a.h, w = a.w;
	const int py = by + ty, px = bx + tx;
	const bool in = py < h && px < w;
	const size_t plane = (size_t)h * w;
	if (tid < 50) F[tid] = a.filt[tid];
	double c[3];
#pragma unroll
	for (int ch = 0; ch < 3; ch++)
	{
		__syncthreads();
		met_stage(T, a.run + ch * plane, by, bx, h, w);
		__syncthreads();
		double t = in ? met_corr(T, F, ty, tx) : 0.0;
		__syncthreads();
		met_stage(T, a.high + ch * plane, by, bx, h, w);
		__syncthreads();
		if (in) t += met_corr(T, F + 25, ty, tx);
		c[ch] = t;
	}
	if (!in) return;
	const size_t o = (size_t)py * w + px;
	if (a.rgb)
	{
		const double cr = c[1] - 0.5, cb = c[2] - 0.5;
		a.out[o] = (float)(c[0] + 1.403 * cr);
		a.out[plane + o] = (float)(c[0] - 0.714 * cr - 0.344 * cb);
		a.out[2 * plane + o] = (float)(c[0] + 1.773 * cb);
	}
	else
	{
		a.out[o] = (float)c[0]; a.out[plane + o] = (float)c[1]; a.out[2 * plane + o] = (float)c[2];
	}
}

// one picture's pyramid into a state: `offsets` of the foveated layout (plan levels) or the noise's own
static void met_analyse(hipStream_t stream, const MetPlan &p, const float *src, float *state, bool noise, int rgb, const float *filters)
{
	for (int l = 0; l < p.f.L - 1; l++)
	{
		const FovLevel &v = p.f.lv[l];
		HvsLevelArgs a;
		a.h = v.a.h; a.w = v.a.w; a.nb = p.f.nb; a.level0 = l == 0; a.rgb = rgb;
		a.src[0] = src; a.src[1] = nullptr; a.ws[0] = state; a.ws[1] = nullptr;
		a.low_in = noise ? (l == 0 ? 0 : p.n_low[l - 1]) : v.low_in;
		a.maps = noise ? p.n_maps[l] : v.a.maps;
		a.low_out = noise ? p.n_low[l] : v.low_out;
		a.filt = filters; a.hs = a.wsrc = 0; a.ry = a.rx = 1.0;
		hvs_launch_level(false, dim3((a.w + HVS_T - 1) / HVS_T, (a.h + HVS_T - 1) / HVS_T, 3), stream, a);
	}
}

// bands: the state the bands and h are read from, at offsets maps[l]; low: the coarsest lowpass [3,lh,lw]
static void met_synthesise(hipStream_t stream, const MetPlan &p, const float *bands, const long long *maps, const float *low, float *run, int rgb,
	const float *filters, float *out)
{
	for (int l = p.f.L - 2; l >= 0; l--)
	{
		MetLevelArgs a;
		a.h = p.f.H >> l; a.w = p.f.W >> l; a.nb = p.f.nb; a.m0 = l == 0 ? 1 : 0;
		a.bands = bands + maps[l]; a.prev = l == p.f.L - 2 ? low : run + p.run[l + 1]; a.filt = filters; a.out = run + p.run[l];
		hipLaunchKernelGGL(k_met_level, dim3((a.w + HVS_T - 1) / HVS_T, (a.h + HVS_T - 1) / HVS_T, 3), dim3(256), 0, stream, a);
	}
	MetFinalArgs f;
	f.h = p.f.H; f.w = p.f.W; f.rgb = rgb; f.run = run + p.run[0]; f.high = bands + maps[0]; f.filt = filters; f.out = out;
	hipLaunchKernelGGL(k_met_final, dim3((f.w + HVS_T - 1) / HVS_T, (f.h + HVS_T - 1) / HVS_T, 1), dim3(256), 0, stream, f);
}

static int met_flag(const char *who, const char *name, int v)
{
	if (v == 0 || v == 1) return FR_OK;
	set_error("%s: %s must be 0 or 1, got %d", who, name, v);
	return FR_ERR_INVALID;
}

static int met_pointer(const char *who, const char *name, const void *p, bool doubles)
{
	if (!p) { set_error("%s: %s is null", who, name); return FR_ERR_INVALID; }
	if ((uintptr_t)p & (doubles ? 7 : 3)) { set_error("%s: %s must be %d-byte aligned", who, name, doubles ? 8 : 4); return FR_ERR_INVALID; }
	return FR_OK;
}

// ---------------------------------------------------------------- the loss
#define MET_LOSS_PER_BLOCK 4096
#define MET_LOSS_MAX_BLOCKS 4096

static int met_loss_blocks(long long n)
{
	const long long b = (n + MET_LOSS_PER_BLOCK - 1) / MET_LOSS_PER_BLOCK;
	return (int)(b < MET_LOSS_MAX_BLOCKS ? b : MET_LOSS_MAX_BLOCKS);
}

// workspace: part[gridDim.x] doubles, then the ticket counter (an unsigned int, zero before the launch and zero after it).
// Workgroup b adds elements b * 4096 + j * gridDim.x * 4096 + .. in a fixed order. The hand-off of the partials to the workgroup
// that draws the last ticket: a plain store, an agent-scope release and the wait for its write-back, then the relaxed agent-scope
// ticket; the last workgroup's every wave acquires at agent scope before it loads, and loads past its L1.
__global__ void __launch_bounds__(256) k_met_loss(long long n, int mse, const float *__restrict__ x, const float *__restrict__ m, double *part, float *__restrict__ out)
{
	__shared__ double s_red[4];
	__shared__ int s_last;
	unsigned int *ticket = (unsigned int *)(part + gridDim.x);
	double acc = 0.0;
	for (long long base = (long long)blockIdx.x * MET_LOSS_PER_BLOCK; base < n; base += (long long)gridDim.x * MET_LOSS_PER_BLOCK)
#pragma unroll 4
		for (int k = 0; k < MET_LOSS_PER_BLOCK / 256; k++)
		{
			const long long i = base + k * 256 + threadIdx.x;
			if (i < n) { const double d = (double)x[i] - (double)m[i]; acc += mse ? d * d : fabs(d); }
		}
	const double t = hvs_block_sum(acc, s_red);
	if (threadIdx.x == 0)
	{
		part[blockIdx.x] = t;
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		const unsigned int prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		s_last = prev == gridDim.x - 1 ? 1 : 0;
	}
	__syncthreads();
	if (!s_last) return;
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	double a = 0.0;
	for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) a += __hip_atomic_load(part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	__syncthreads(); // (s_red is read above by every wave)
	const double s = hvs_block_sum(a, s_red);
	if (threadIdx.x == 0)
	{
		out[0] = (float)(s / (double)n);
		__hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// d mean|x - m| / dx = sign(x - m) / n, d mean (x - m)^2 / dx = 2 (x - m) / n, times the upstream gradient (a device scalar)
__global__ void __launch_bounds__(256) k_met_loss_bwd(long long n, int mse, const float *__restrict__ x, const float *__restrict__ m,
	const float *__restrict__ gscale, float *__restrict__ dx)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const float g = gscale ? *gscale : 1.0f;
	const double d = (double)x[i] - (double)m[i];
	const float w = mse ? (float)(2.0 * d / (double)n) : (d > 0.0 ? 1.0f : (d < 0.0 ? -1.0f : 0.0f)) * (float)(1.0 / (double)n);
	dx[i] = g * w;
}

} // namespace fr

using namespace fr;

extern "C" int64_t fr_hvs_metamer_workspace_floats(int32_t H, int32_t W, int32_t n_levels, int32_t n_orientations, int32_t roundtrip)
{
	MetPlan p;
	if (met_flag("hvs_metamer", "roundtrip", roundtrip) != FR_OK) return -1;
	if (met_plan(H, W, n_levels, n_orientations, roundtrip != 0, &p) != FR_OK) return -1;
	return p.floats;
}

extern "C" int fr_hvs_metamer(int32_t H, int32_t W, double alpha, double real_image_width, double real_viewing_distance, int32_t mode,
	double gaze_x, double gaze_y, int32_t n_levels, int32_t n_orientations, int32_t rgb, const float *filters, const float *target,
	const float *noise, float *workspace, float *out, void *stream_)
{
	static const char *who = "hvs_metamer";
	MetPlan p;
	int rc = met_plan(H, W, n_levels, n_orientations, false, &p);
	if (rc != FR_OK) return rc;
	if ((rc = fov_check_view(who, alpha, real_image_width, real_viewing_distance, gaze_x, gaze_y)) != FR_OK) return rc;
	if (mode != 0 && mode != 1) { set_error("%s: mode must be 0 (linear) or 1 (quadratic), got %d", who, mode); return FR_ERR_INVALID; }
	if ((rc = met_flag(who, "rgb", rgb)) != FR_OK) return rc;
	if ((rc = met_pointer(who, "filters", filters, false)) != FR_OK || (rc = met_pointer(who, "target", target, false)) != FR_OK
		|| (rc = met_pointer(who, "noise", noise, false)) != FR_OK || (rc = met_pointer(who, "workspace", workspace, true)) != FR_OK
		|| (rc = met_pointer(who, "out", out, false)) != FR_OK)
		return rc;
	hipStream_t stream = (hipStream_t)stream_;
	double *dws = (double *)workspace, *lod = dws + p.d_lod, *scal = dws + p.d_scal, *part = dws + p.d_part;
	float *st = workspace + p.o_target, *sn = workspace + p.o_noise, *run = workspace + p.o_run;
	// the target's statistics (:81-88) and the noise's pyramid (:92-93)
	met_analyse(stream, p, target, st, false, rgb, filters);
	met_analyse(stream, p, noise, sn, true, 0, filters);
	for (int l = 0; l < p.f.L - 1; l++)
	{
		const FovLevel &v = p.f.lv[l];
		const long long plane = (long long)v.a.h * v.a.w, n = 3 * plane;
		FovLodArgs q;
		q.h = v.a.h; q.w = v.a.w; q.quadratic = mode; q.alpha = alpha; q.width = real_image_width; q.distance = real_viewing_distance;
		q.gx = gaze_x; q.gy = gaze_y; q.lod = lod + v.lod;
		fov_launch_lod(stream, q);
		fov_launch_chain(stream, v.a, st, nullptr, 1);
		// match_level's two scalars (:97-103) of each of the level's bands
		const int nblk = (int)((n + 1023) / 1024);
		double *sc = scal + 2 * met_band(p, l, 0);
		for (int centred = 0; centred < 2; centred++)
		{
			MetSumArgs s;
			s.maps = sn + p.n_maps[l]; s.n = n; s.centred = centred; s.scal = sc; s.part = part;
			hipLaunchKernelGGL(k_met_sum, dim3(nblk, v.nm), dim3(256), 0, stream, s);
			hipLaunchKernelGGL(k_met_finish, dim3(v.nm), dim3(1024), 0, stream, nblk, n, centred, (const double *)part, sc);
		}
		MetMatchArgs m;
		m.a = v.a; m.wst = st; m.band = sn + p.n_maps[l]; m.lod = lod + v.lod; m.scal = sc;
		hipLaunchKernelGGL(k_met_match, dim3((unsigned)((plane + 255) / 256), v.a.nmc), dim3(256), 0, stream, m);
	}
	// the last lowpass is the target's own (:116); the matched pyramid's synthesis, YCrCb -> RGB
	met_synthesise(stream, p, sn, p.n_maps, st + p.f.lv[p.f.L - 2].low_out, run, 1, filters, out);
	return check_launch(who, stream, false);
}

extern "C" int fr_hvs_metamer_roundtrip(int32_t H, int32_t W, int32_t n_levels, int32_t n_orientations, int32_t rgb, const float *filters,
	const float *image, float *workspace, float *out, void *stream_)
{
	static const char *who = "hvs_metamer_roundtrip";
	MetPlan p;
	int rc = met_plan(H, W, n_levels, n_orientations, true, &p);
	if (rc != FR_OK) return rc;
	if ((rc = met_flag(who, "rgb", rgb)) != FR_OK) return rc;
	if ((rc = met_pointer(who, "filters", filters, false)) != FR_OK || (rc = met_pointer(who, "image", image, false)) != FR_OK
		|| (rc = met_pointer(who, "workspace", workspace, true)) != FR_OK || (rc = met_pointer(who, "out", out, false)) != FR_OK)
		return rc;
	hipStream_t stream = (hipStream_t)stream_;
	float *st = workspace + p.o_target, *run = workspace + p.o_run;
	long long maps[HVS_MAXL];
	for (int l = 0; l < p.f.L - 1; l++) maps[l] = p.f.lv[l].a.maps;
	met_analyse(stream, p, image, st, false, rgb, filters);
	met_synthesise(stream, p, st, maps, st + p.f.lv[p.f.L - 2].low_out, run, rgb, filters, out);
	return check_launch(who, stream, false);
}

extern "C" int64_t fr_hvs_metamer_loss_workspace_doubles(int64_t n)
{
	if (n <= 0) { set_error("hvs_metamer_loss: n must be positive"); return -1; }
	return met_loss_blocks(n) + 1;
}

extern "C" int fr_hvs_metamer_loss_forward(int64_t n, int32_t mse, const float *image, const float *metamer, double *workspace, float *out,
	void *stream_)
{
	static const char *who = "hvs_metamer_loss_forward";
	int rc;
	if (n <= 0) { set_error("%s: n must be positive", who); return FR_ERR_INVALID; }
	if ((rc = met_flag(who, "mse", mse)) != FR_OK) return rc;
	if ((rc = met_pointer(who, "image", image, false)) != FR_OK || (rc = met_pointer(who, "metamer", metamer, false)) != FR_OK
		|| (rc = met_pointer(who, "workspace", workspace, true)) != FR_OK || (rc = met_pointer(who, "out", out, false)) != FR_OK)
		return rc;
	hipStream_t stream = (hipStream_t)stream_;
	hipLaunchKernelGGL(k_met_loss, dim3(met_loss_blocks(n)), dim3(256), 0, stream, (long long)n, mse, image, metamer, workspace, out);
	return check_launch(who, stream, false);
}

extern "C" int fr_hvs_metamer_loss_backward(int64_t n, int32_t mse, const float *image, const float *metamer, const float *grad_scale,
	float *dL_dimage, void *stream_)
{
	static const char *who = "hvs_metamer_loss_backward";
	int rc;
	if (n <= 0 || n > (1ll << 39)) { set_error("%s: n must be positive (and below 2^39)", who); return FR_ERR_INVALID; }
	if ((rc = met_flag(who, "mse", mse)) != FR_OK) return rc;
	if ((rc = met_pointer(who, "image", image, false)) != FR_OK || (rc = met_pointer(who, "metamer", metamer, false)) != FR_OK
		|| (rc = met_pointer(who, "dL_dimage", dL_dimage, false)) != FR_OK)
		return rc;
	hipStream_t stream = (hipStream_t)stream_;
	hipLaunchKernelGGL(k_met_loss_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (long long)n, mse, image, metamer, grad_scale, dL_dimage);
	return check_launch(who, stream, false);
}
