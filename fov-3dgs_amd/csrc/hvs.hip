// fovraster -- the uniform metameric (HVS) loss, fused: MetamericLossUniform with bilinear_downsampling=True and the cropped
// 5x5 filters, the loss of metric_mask_learn.py:227 and eff_finetune.py:122 (include/fovraster.h: fr_hvs_*).
//
// Reference behaviour:
//   metamer/odak_perception/color_conversion.py:400-403         Y = .299 R + .587 G + .114 B, Cr = .5 + .713 (R - Y), Cb = .5 + .564 (B - Y)
//   metamer/odak_perception/spatial_steerable_pyramid.py:136-145 level 0: h = conv(reflect-pad 2, h0), low = conv(reflect-pad 2, l0),
//                                                                 bands = conv(reflect-pad 2 of LOW, b_o)
//                                                      :148-178 levels 1..n-2: low = 2x2 mean of low, bands of that; the last 2x2 mean is a statistic
//   metamer/odak_perception/metameric_loss_uniform.py:8-12       blur = bilinear-up(area-down(x, 1/p)): adaptive-average windows
//                                                                 [floor(j n / n'), ceil((j+1) n / n')), n' = floor(n (1/p)); align_corners=False
//                                                      :57-69    mean = blur(x), var = blur(x^2) - mean^2, below 1e-7 -> 1e-7, std = sqrt(var)
//                                                      :75-87    statistics: (mean, std) of h, of every band (p halves per level), the last low
//                                                      :90-100   loss = mean over the statistics of their L1 / MSE mean
// The filter coefficients are an input: a device buffer [(2 + nb) * 25] = l0, h0, b_0 .. b_{nb-1}, read into LDS by every
// workgroup that filters. No table of them is compiled in.
//
// Forward, per pyramid level one launch of each of
//   k_hvs_level     a 16x16 tile of the level's lowpass with its 2-pixel halo in LDS (reflection resolved at the load; at level
//                   0 the colour-converted image with a 4-pixel halo, from which the lowpass tile AND h are made): all bands,
//                   each channel on its own, and the next level's lowpass (2x2 mean) from the one staged tile.
//   k_hvs_pool      the adaptive windows' mean and mean-square of every map of the level: the pooled maps are the state kept.
//   k_hvs_cmp_*     bilinear samples of both pictures' pooled maps -> mean, std -> |d| or d^2, summed per workgroup. No
//                   full-resolution statistic is written. A level whose 1/p is an integer has blur = identity exactly (every
//                   window is one pixel and a bilinear sample falls on or between copies of one value: .5 x + .5 x = x in every
//                   precision), so var = 0, std is the constant sqrt(1e-7) on both sides and the mean is the band: that level
//                   compares the bands directly (k_hvs_cmp_direct) and is not pooled.
// and k_hvs_finish adds the per-workgroup sums in double in a fixed order (no atomics anywhere: the same bits on every run).
// Image and target go through k_hvs_level / k_hvs_pool in the SAME launches (grid z / y), the target only when its state is
// not reused. Backward, all gathers:
//   k_hvs_bwd_up    per pooled cell: the adjoint of the bilinear up-sampling over the cell's footprint, the statistics'
//                   derivatives recomputed from the pooled maps at each pixel of the footprint.
//   k_hvs_bwd_level per level, coarsest first: per band the adjoint of the windows gathered at the load into an LDS tile with a
//                   2-pixel halo, the transposed 5x5 with the reflected halo folded back, summed over the bands, plus a quarter
//                   of the coarser level's lowpass gradient.
//   k_hvs_bwd_image l0^T of the level-0 lowpass gradient + h0^T of h's gradient, the colour transpose, times the upstream
//                   gradient (a device scalar).
// Resized (fr_hvs_*_resized): the scripts resize both pictures bilinearly to the next multiple of 2^levels in front of the loss
// (metric_mask_learn.py:221-227, eff_finetune.py:116-122, prune.py:128-134: F.interpolate(.., mode='bilinear',
// align_corners=False); 1080 is no multiple of 32). Here the pictures stay [3,Hs,Ws] and
//   k_hvs_level<true> samples them in the level-0 load: the staged value at the tile's reflected position (y, x) of the H x W
//                   grid is the two-tap lerp per axis (hvs_lerp, scale Hs / H, Ws / W) of R, G and B, the colour converted
//                   afterwards; everything behind the load is the H x W call. k_hvs_level<false> is the kernel as it was.
//   k_hvs_bwd_resize the transposed resize as a gather per SOURCE pixel over the resized pixels whose own hvs_lerp names it, in
//                   a fixed order, from k_hvs_bwd_image's H x W gradient in the workspace: no atomics, no zero fill.
// Hs <= H and Ws <= W only (an axis of equal size is the identity exactly).
// The foveated loss (csrc/hvs_fov.hip) launches k_hvs_level, k_hvs_bwd_level<FOV>, k_hvs_bwd_image<FOV>, k_hvs_bwd_resize,
// k_hvs_cmp_direct and k_hvs_finish through the launchers at the end of the namespace; hvs_common.h holds what both files share.
#include "hvs_common.h"

namespace fr {

struct HvsLevel
{
	int h, w, ph, pw, identity, nm;              // nm maps: the bands, at level 0 h in front of them
	long long maps, pool, low_in, low_out;       // offsets (floats) in a side's forward state
	long long gpool, glow;                       // ... in the backward workspace
	long long part; int part_n;                  // this level's slice of the partial sums
	double sy, sx;                               // bilinear source scale ph / h, pw / w
};

struct HvsPlan
{
	int L, nb, H, W, lh, lw, nstats;
	HvsLevel lv[HVS_MAXL];
	long long res_part; int res_part_n;
	long long ws_floats, bwd_floats, n_partials;
};

static int hvs_plan(int H, int W, double pooling, int L, int nb, HvsPlan *p)
{
	if (L < 2 || L > HVS_MAXL) { set_error("hvs: n_pyramid_levels %d outside 2..%d", L, HVS_MAXL); return FR_ERR_INVALID; }
	if (nb < 1 || nb > HVS_MAXB) { set_error("hvs: %d orientations outside 1..%d", nb, HVS_MAXB); return FR_ERR_INVALID; }
	if (H <= 0 || W <= 0 || H % (1 << L) || W % (1 << L)) { set_error("hvs: size %dx%d is not a multiple of 2^%d", H, W, L); return FR_ERR_INVALID; }
	if (H > 16384 || W > 16384) { set_error("hvs: size %dx%d too large (max 16384)", H, W); return FR_ERR_INVALID; }
	if (!(pooling > 0.0) || !(pooling < 1e6)) { set_error("hvs: pooling_size must be positive and finite"); return FR_ERR_INVALID; }
	p->L = L; p->nb = nb; p->H = H; p->W = W; p->nstats = 2 * (1 + (L - 1) * nb) + 1;
	long long ws = 0, bw = 0, np = 0;
	double pl = pooling;
	for (int l = 0; l < L - 1; l++, pl /= 2)
	{
		HvsLevel &v = p->lv[l];
		v.h = H >> l; v.w = W >> l; v.nm = nb + (l == 0 ? 1 : 0);
		const double k = 1.0 / pl;
		v.identity = (k >= 1.0 && k == floor(k)) ? 1 : 0;
		const long long plane = (long long)v.h * v.w;
		v.maps = ws; ws += (long long)v.nm * 3 * plane;
		v.ph = (int)floor((double)v.h * k); v.pw = (int)floor((double)v.w * k);
		v.pool = v.gpool = 0;
		if (!v.identity)
		{
			if (v.ph < 1 || v.pw < 1) { set_error("hvs: pooling %g leaves level %d (%dx%d) without a pooled pixel", pl, l, v.h, v.w); return FR_ERR_INVALID; }
			if ((long long)v.ph * v.pw > (1ll << 28)) { set_error("hvs: pooled level too large"); return FR_ERR_INVALID; }
			const long long cells = (long long)v.nm * 3 * v.ph * v.pw;
			v.pool = ws; ws += 2 * cells;
			v.gpool = bw; bw += 2 * cells;
			v.part_n = (int)((plane + 255) / 256) * v.nm * 3;
		}
		else
			v.part_n = (int)(((long long)v.nm * 3 * plane + 1023) / 1024);
		v.sy = (double)v.ph / (double)v.h; v.sx = (double)v.pw / (double)v.w;
		v.part = np; np += v.part_n;
		v.glow = bw; bw += 3 * plane;
		v.low_in = l == 0 ? 0 : p->lv[l - 1].low_out;
		v.low_out = ws; ws += 3 * (plane / 4);
	}
	p->lh = H >> (L - 1); p->lw = W >> (L - 1);
	p->res_part = np; p->res_part_n = (int)((3ll * p->lh * p->lw + 1023) / 1024); np += p->res_part_n;
	p->ws_floats = ws; p->bwd_floats = bw; p->n_partials = np;
	return FR_OK;
}

// ---------------------------------------------------------------- forward
// RESIZED (level 0 only): the staged value at (y, x) of the h x w grid is the bilinear sample (upsample_bilinear2d,
// align_corners=False: hvs_lerp) of the [3,hs,wsrc] picture, R, G and B interpolated first (in double, kept in fp32) and the
// colour converted afterwards, as a script that resizes and then calls the loss does. Reflection acts on (y, x). The plain
// instantiation is the kernel as it was.
template <bool RESIZED>
__global__ void __launch_bounds__(256) k_hvs_level(HvsLevelArgs a)
{
	__shared__ float S[HVS_IM][HVS_IM + 1], LP[HVS_LP][HVS_LP + 1], F[(2 + HVS_MAXB) * 25];
	const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
	const int side = blockIdx.z / 3, ch = blockIdx.z - 3 * side;
	const int bx = blockIdx.x * HVS_T, by = blockIdx.y * HVS_T, h = a.h, w = a.w;
	const size_t plane = (size_t)h * w;
	float *ws = a.ws[side];
	for (int i = tid; i < (2 + a.nb) * 25; i += 256) F[i] = a.filt[i];
	if (a.level0)
	{
		const float *src = a.src[side];
		for (int i = tid; i < HVS_IM * HVS_IM; i += 256)
		{
			const int r = i / HVS_IM, c = i - r * HVS_IM;
			float v;
			if (RESIZED)
			{
				const HvsLerp ly = hvs_lerp(hvs_reflect(by + r - 4, h), a.ry, a.hs), lx = hvs_lerp(hvs_reflect(bx + c - 4, w), a.rx, a.wsrc);
				const size_t splane = (size_t)a.hs * a.wsrc;
				if (a.rgb)
				{
					const float R = (float)hvs_bilerp(src, a.wsrc, ly, lx), G = (float)hvs_bilerp(src + splane, a.wsrc, ly, lx),
						B = (float)hvs_bilerp(src + 2 * splane, a.wsrc, ly, lx);
					const float Y = 0.299f * R + 0.587f * G + 0.114f * B;
					v = ch == 0 ? Y : (ch == 1 ? 0.5f + 0.713f * (R - Y) : 0.5f + 0.564f * (B - Y));
				}
				else
					v = (float)hvs_bilerp(src + ch * splane, a.wsrc, ly, lx);
				S[r][c] = v;
				continue;
			}
			const size_t o = (size_t)hvs_reflect(by + r - 4, h) * w + hvs_reflect(bx + c - 4, w);
			if (a.rgb)
			{
				const float R = src[o], G = src[plane + o], B = src[2 * plane + o];
				const float Y = 0.299f * R + 0.587f * G + 0.114f * B;
				v = ch == 0 ? Y : (ch == 1 ? 0.5f + 0.713f * (R - Y) : 0.5f + 0.564f * (B - Y));
			}
			else
				v = src[ch * plane + o];
			S[r][c] = v;
		}
		__syncthreads();
		// the lowpass at the tile and its halo: at a reflected position it is the lowpass of the reflected pixel, whose own
		// 5x5 neighbourhood lies inside the staged image (the reflected pixel is at most 3 from the edge, inside this tile)
		for (int i = tid; i < HVS_LP * HVS_LP; i += 256)
		{
			const int r = i / HVS_LP, c = i - r * HVS_LP;
			const int r2 = min(max(hvs_reflect(by + r - 2, h) - by + 4, 2), HVS_IM - 3);
			const int c2 = min(max(hvs_reflect(bx + c - 2, w) - bx + 4, 2), HVS_IM - 3);
			double t = 0.0; // (sums in double, kept in fp32: see HvsStat)
#pragma unroll
			for (int ky = 0; ky < 5; ky++)
#pragma unroll
				for (int kx = 0; kx < 5; kx++) t += (double)F[ky * 5 + kx] * (double)S[r2 + ky - 2][c2 + kx - 2];
			LP[r][c] = (float)t;
		}
	}
	else
	{
		const float *low = ws + a.low_in + ch * plane;
		for (int i = tid; i < HVS_LP * HVS_LP; i += 256)
		{
			const int r = i / HVS_LP, c = i - r * HVS_LP;
			LP[r][c] = low[(size_t)hvs_reflect(by + r - 2, h) * w + hvs_reflect(bx + c - 2, w)];
		}
	}
	__syncthreads();
	const int py = by + ty, px = bx + tx;
	if (py < h && px < w)
	{
		const size_t o = (size_t)py * w + px;
		int m = 0;
		if (a.level0)
		{
			double t = 0.0;
#pragma unroll
			for (int ky = 0; ky < 5; ky++)
#pragma unroll
				for (int kx = 0; kx < 5; kx++) t += (double)F[25 + ky * 5 + kx] * (double)S[ty + 2 + ky][tx + 2 + kx];
			ws[a.maps + (size_t)ch * plane + o] = (float)t;
			m = 1;
		}
		double v[25]; // the pixel's neighbourhood, converted once for all bands
#pragma unroll
		for (int ky = 0; ky < 5; ky++)
#pragma unroll
			for (int kx = 0; kx < 5; kx++) v[ky * 5 + kx] = (double)LP[ty + ky][tx + kx];
		for (int b = 0; b < a.nb; b++)
		{
			const float *f = F + 50 + b * 25;
			double t = 0.0;
#pragma unroll
			for (int k = 0; k < 25; k++) t += (double)f[k] * v[k];
			ws[a.maps + ((size_t)(m + b) * 3 + ch) * plane + o] = (float)t;
		}
	}
	if (tid < 64)
	{
		const int j = tid >> 3, i = tid & 7, oy = (by >> 1) + j, ox = (bx >> 1) + i, h2 = h >> 1, w2 = w >> 1;
		if (oy < h2 && ox < w2)
			ws[a.low_out + (size_t)ch * h2 * w2 + (size_t)oy * w2 + ox] =
				(float)((((double)LP[2 * j + 2][2 * i + 2] + (double)LP[2 * j + 2][2 * i + 3]) + ((double)LP[2 * j + 3][2 * i + 2] + (double)LP[2 * j + 3][2 * i + 3])) * 0.25);
	}
}

struct HvsPoolArgs { int h, w, ph, pw, nmc, G; float *ws[2]; long long maps, pool; };

// G lanes (1, 8 or 64) share one pooled cell: lane i adds elements i, i + G, .. of the window, the G sums are added by xor-shuffles
__global__ void __launch_bounds__(256) k_hvs_pool(HvsPoolArgs a)
{
	const int G = a.G, lane = threadIdx.x & (G - 1);
	const long long cell = ((long long)blockIdx.x * 256 + threadIdx.x) / G, ncell = (long long)a.nmc * a.ph * a.pw;
	const bool valid = cell < ncell;
	float *ws = a.ws[blockIdx.y];
	double s = 0.0, q = 0.0;
	int cnt = 1;
	if (valid)
	{
		const int mc = (int)(cell / (a.ph * a.pw)), rem = (int)(cell - (long long)mc * (a.ph * a.pw)), jy = rem / a.pw, jx = rem - jy * a.pw;
		const int ys = (int)(((long long)jy * a.h) / a.ph), ye = (int)(((long long)(jy + 1) * a.h + a.ph - 1) / a.ph);
		const int xs = (int)(((long long)jx * a.w) / a.pw), xe = (int)(((long long)(jx + 1) * a.w + a.pw - 1) / a.pw);
		const int ww = xe - xs;
		cnt = (ye - ys) * ww;
		const float *map = ws + a.maps + (size_t)mc * a.h * a.w;
		for (int e = lane; e < cnt; e += G)
		{
			const int y = ys + e / ww, x = xs + e % ww;
			const double v = (double)map[(size_t)y * a.w + x];
			s += v; q += v * v;
		}
	}
	for (int off = G >> 1; off > 0; off >>= 1) { s += __shfl_xor(s, off); q += __shfl_xor(q, off); }
	if (valid && lane == 0) { ws[a.pool + cell] = (float)(s / (double)cnt); ws[a.pool + ncell + cell] = (float)(q / (double)cnt); }
}

struct HvsCmpArgs { int h, w, ph, pw, nmc, mse; double sy, sx; float wgt; const float *wsi, *wst; long long pool; float *partials; };

__global__ void __launch_bounds__(256) k_hvs_cmp_pooled(HvsCmpArgs a)
{
	__shared__ double s_red[4];
	const int pix = blockIdx.x * 256 + threadIdx.x, mc = blockIdx.y;
	double acc = 0.0;
	if (pix < a.h * a.w)
	{
		const int y = pix / a.w, x = pix - y * a.w;
		const HvsLerp ly = hvs_lerp(y, a.sy, a.ph), lx = hvs_lerp(x, a.sx, a.pw);
		const size_t cells = (size_t)a.ph * a.pw;
		const HvsStat A = hvs_stat(a.wsi + a.pool + mc * cells, a.wsi + a.pool + (a.nmc + mc) * cells, a.pw, ly, lx);
		const HvsStat B = hvs_stat(a.wst + a.pool + mc * cells, a.wst + a.pool + (a.nmc + mc) * cells, a.pw, ly, lx);
		const double dm = A.mean - B.mean, ds = A.std - B.std;
		acc = a.mse ? dm * dm + ds * ds : fabs(dm) + fabs(ds);
	}
	const double t = hvs_block_sum(acc, s_red);
	if (threadIdx.x == 0) a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (float)(t * (double)a.wgt);
}

__global__ void __launch_bounds__(256) k_hvs_cmp_direct(const float *__restrict__ x, const float *__restrict__ y, long long n, int mse, float wgt,
	float *__restrict__ partials)
{
	__shared__ double s_red[4];
	double acc = 0.0;
#pragma unroll
	for (int k = 0; k < 4; k++)
	{
		const long long i = (long long)blockIdx.x * 1024 + k * 256 + threadIdx.x;
		if (i < n) { const double d = (double)x[i] - (double)y[i]; acc += mse ? d * d : fabs(d); }
	}
	const double t = hvs_block_sum(acc, s_red);
	if (threadIdx.x == 0) partials[blockIdx.x] = (float)(t * (double)wgt);
}

__global__ void __launch_bounds__(1024) k_hvs_finish(int n, const float *__restrict__ partials, float *__restrict__ out)
{
	__shared__ double s0[1024];
	double a = 0.0;
	for (int i = threadIdx.x; i < n; i += 1024) a += (double)partials[i];
	s0[threadIdx.x] = a;
	__syncthreads();
	for (int off = 512; off > 0; off >>= 1)
	{
		if ((int)threadIdx.x < off) s0[threadIdx.x] += s0[threadIdx.x + off];
		__syncthreads();
	}
	if (threadIdx.x == 0) out[0] = (float)s0[0];
}

// ---------------------------------------------------------------- backward
struct HvsUpArgs { int h, w, ph, pw, nmc, mse, G; double sy, sx; float wgt; const float *wsi, *wst; long long pool; float *gpool; };

__global__ void __launch_bounds__(256) k_hvs_bwd_up(HvsUpArgs a)
{
	const int G = a.G, lane = threadIdx.x & (G - 1);
	const long long cell = ((long long)blockIdx.x * 256 + threadIdx.x) / G, ncell = (long long)a.nmc * a.ph * a.pw;
	const bool valid = cell < ncell;
	float gm = 0.0f, gq = 0.0f;
	if (valid)
	{
		const size_t cells = (size_t)a.ph * a.pw;
		const int mc = (int)(cell / (long long)cells), rem = (int)(cell - (long long)mc * cells), jy = rem / a.pw, jx = rem - jy * a.pw;
		// the pixels whose two source rows can include jy: src in [jy - 1, jy + 1), one more on each side against rounding; each
		// pixel's own weights (computed as the forward does) decide
		int ylo = max(0, (int)floor(((double)jy - 0.5) / a.sy - 0.5) - 1), yhi = min(a.h - 1, (int)ceil(((double)jy + 1.5) / a.sy - 0.5) + 1);
		int xlo = max(0, (int)floor(((double)jx - 0.5) / a.sx - 0.5) - 1), xhi = min(a.w - 1, (int)ceil(((double)jx + 1.5) / a.sx - 0.5) + 1);
		if (jy == 0) ylo = 0;
		if (jx == 0) xlo = 0;
		if (jy == a.ph - 1) yhi = a.h - 1;
		if (jx == a.pw - 1) xhi = a.w - 1;
		const int nw = xhi - xlo + 1, cnt = (nw > 0 && yhi >= ylo) ? (yhi - ylo + 1) * nw : 0;
		const float *im = a.wsi + a.pool + mc * cells, *iq = a.wsi + a.pool + (a.nmc + mc) * cells;
		const float *tm = a.wst + a.pool + mc * cells, *tq = a.wst + a.pool + (a.nmc + mc) * cells;
		for (int e = lane; e < cnt; e += G)
		{
			const int y = ylo + e / nw, x = xlo + e % nw;
			const HvsLerp ly = hvs_lerp(y, a.sy, a.ph), lx = hvs_lerp(x, a.sx, a.pw);
			const double wy = (ly.i0 == jy ? ly.l0 : 0.0) + (ly.i1 == jy ? ly.l1 : 0.0);
			const double wx = (lx.i0 == jx ? lx.l0 : 0.0) + (lx.i1 == jx ? lx.l1 : 0.0);
			const float wt = (float)(wy * wx);
			if (wt != 0.0f)
			{
				float dmean, dmsq;
				hvs_pix_grad(hvs_stat(im, iq, a.pw, ly, lx), hvs_stat(tm, tq, a.pw, ly, lx), a.mse, a.wgt, dmean, dmsq);
				gm += wt * dmean; gq += wt * dmsq;
			}
		}
	}
	for (int off = G >> 1; off > 0; off >>= 1) { gm += __shfl_xor(gm, off); gq += __shfl_xor(gq, off); }
	if (valid && lane == 0) { a.gpool[cell] = gm; a.gpool[ncell + cell] = gq; }
}

// d loss / d map[mc](y, x): the adjoint of the adaptive windows (a gather over the cells whose window holds the pixel), or the
// direct comparison's derivative on an identity level; 0 outside the map. FOV (the foveated loss, csrc/hvs_fov.hip): the map's
// finished gradient, read from the workspace [nmc,h,w]. The plain instantiation is the function as it was.
template <bool FOV>
__device__ __forceinline__ float hvs_g_at(const HvsGArgs &a, int mc, int y, int x)
{
	if (y < 0 || y >= a.h || x < 0 || x >= a.w) return 0.0f;
	if (FOV) return a.gpool[(size_t)mc * a.h * a.w + (size_t)y * a.w + x];
	const size_t o = a.maps + (size_t)mc * a.h * a.w + (size_t)y * a.w + x;
	const float xv = a.wsi[o];
	if (a.identity) return a.wgt * hvs_dabs((double)xv - (double)a.wst[o], a.mse);
	const size_t cells = (size_t)a.ph * a.pw;
	const float *gm = a.gpool + mc * cells, *gq = a.gpool + (a.nmc + mc) * cells;
	const int jylo = max(0, (int)(((long long)y * a.ph) / a.h) - 1), jyhi = min(a.ph - 1, (int)(((long long)(y + 1) * a.ph + a.h - 1) / a.h) + 1);
	const int jxlo = max(0, (int)(((long long)x * a.pw) / a.w) - 1), jxhi = min(a.pw - 1, (int)(((long long)(x + 1) * a.pw + a.w - 1) / a.w) + 1);
	float acc = 0.0f;
	for (int jy = jylo; jy <= jyhi; jy++)
	{
		const int ys = (int)(((long long)jy * a.h) / a.ph), ye = (int)(((long long)(jy + 1) * a.h + a.ph - 1) / a.ph);
		if (y < ys || y >= ye) continue;
		for (int jx = jxlo; jx <= jxhi; jx++)
		{
			const int xs = (int)(((long long)jx * a.w) / a.pw), xe = (int)(((long long)(jx + 1) * a.w + a.pw - 1) / a.pw);
			if (x < xs || x >= xe) continue;
			acc += (gm[jy * a.pw + jx] + 2.0f * xv * gq[jy * a.pw + jx]) / (float)((ye - ys) * (xe - xs));
		}
	}
	return acc;
}

// The transposed 5x5 at (qy, qx) = (by + ty, bx + tx) from a gradient tile G (2-pixel halo, 0 outside the map), reflection
// folded back: with T[u] = sum_k f[k] g[u - k + 2] on the padded grid u in [-2, n + 2), the pixel collects T at itself and at
// the padded positions that reflect onto it (-q for q in {1, 2}; 2 (n - 1) - q for q in {n - 2, n - 3}). Every in-map g such a
// term reads lies within 2 of q, i.e. inside the tile's halo.
__device__ __forceinline__ float hvs_convT(const float (*G)[HVS_LP + 1], const float *f, int ty, int tx, int qy, int qx, int h, int w, int by, int bx)
{
	float acc = 0.0f;
#pragma unroll
	for (int ky = 0; ky < 5; ky++)
#pragma unroll
		for (int kx = 0; kx < 5; kx++) acc += f[ky * 5 + kx] * G[ty + 4 - ky][tx + 4 - kx];
	int uy[3], ux[3], ny = 1, nx = 1;
	uy[0] = qy; ux[0] = qx;
	if (qy == 1 || qy == 2) uy[ny++] = -qy;
	if (qy == h - 2 || qy == h - 3) uy[ny++] = 2 * (h - 1) - qy;
	if (qx == 1 || qx == 2) ux[nx++] = -qx;
	if (qx == w - 2 || qx == w - 3) ux[nx++] = 2 * (w - 1) - qx;
	if (ny > 1 || nx > 1)
		for (int i = 0; i < ny; i++)
			for (int j = 0; j < nx; j++)
			{
				if (i == 0 && j == 0) continue;
				for (int ky = 0; ky < 5; ky++)
				{
					const int gy = uy[i] - ky + 2, ry = gy - by + 2;
					if (gy < 0 || gy >= h || ry < 0 || ry >= HVS_LP) continue;
					for (int kx = 0; kx < 5; kx++)
					{
						const int gx = ux[j] - kx + 2, rx = gx - bx + 2;
						if (gx < 0 || gx >= w || rx < 0 || rx >= HVS_LP) continue;
						acc += f[ky * 5 + kx] * G[ry][rx];
					}
				}
			}
	return acc;
}

template <bool FOV>
__global__ void __launch_bounds__(256) k_hvs_bwd_level(HvsBwdLevelArgs a)
{
	__shared__ float G[HVS_LP][HVS_LP + 1], F[(2 + HVS_MAXB) * 25];
	const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, ch = blockIdx.z;
	const int bx = blockIdx.x * HVS_T, by = blockIdx.y * HVS_T, h = a.g.h, w = a.g.w;
	const int qy = by + ty, qx = bx + tx;
	const bool in = qy < h && qx < w;
	for (int i = tid; i < (2 + a.nb) * 25; i += 256) F[i] = a.filt[i];
	float acc = 0.0f;
	for (int b = 0; b < a.nb; b++)
	{
		__syncthreads();
		for (int i = tid; i < HVS_LP * HVS_LP; i += 256)
		{
			const int r = i / HVS_LP, c = i - r * HVS_LP;
			G[r][c] = hvs_g_at<FOV>(a.g, (a.m0 + b) * 3 + ch, by + r - 2, bx + c - 2);
		}
		__syncthreads();
		if (in) acc += hvs_convT(G, F + 50 + b * 25, ty, tx, qy, qx, h, w, by, bx);
	}
	if (in)
	{
		const int h2 = h >> 1, w2 = w >> 1;
		const size_t o2 = (size_t)ch * h2 * w2 + (size_t)(qy >> 1) * w2 + (qx >> 1);
		const float up = a.last ? a.wres * hvs_dabs((double)a.low_i[o2] - (double)a.low_t[o2], a.g.mse) : a.glow_next[o2];
		a.glow[(size_t)ch * h * w + (size_t)qy * w + qx] = acc + 0.25f * up;
	}
}

template <bool FOV>
__global__ void __launch_bounds__(256) k_hvs_bwd_image(HvsBwdImageArgs a)
{
	__shared__ float G[HVS_LP][HVS_LP + 1], F[50];
	const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
	const int bx = blockIdx.x * HVS_T, by = blockIdx.y * HVS_T, h = a.g.h, w = a.g.w;
	const int qy = by + ty, qx = bx + tx;
	const bool in = qy < h && qx < w;
	const size_t plane = (size_t)h * w;
	if (tid < 50) F[tid] = a.filt[tid];
	float gc[3];
#pragma unroll
	for (int ch = 0; ch < 3; ch++)
	{
		__syncthreads();
		for (int i = tid; i < HVS_LP * HVS_LP; i += 256)
		{
			const int r = i / HVS_LP, c = i - r * HVS_LP, y = by + r - 2, x = bx + c - 2;
			G[r][c] = (y >= 0 && y < h && x >= 0 && x < w) ? a.glow0[ch * plane + (size_t)y * w + x] : 0.0f;
		}
		__syncthreads();
		float t = in ? hvs_convT(G, F, ty, tx, qy, qx, h, w, by, bx) : 0.0f;
		__syncthreads();
		for (int i = tid; i < HVS_LP * HVS_LP; i += 256)
		{
			const int r = i / HVS_LP, c = i - r * HVS_LP;
			G[r][c] = hvs_g_at<FOV>(a.g, ch, by + r - 2, bx + c - 2);
		}
		__syncthreads();
		if (in) t += hvs_convT(G, F + 25, ty, tx, qy, qx, h, w, by, bx);
		gc[ch] = t;
	}
	if (!in) return;
	const float s = a.gscale ? *a.gscale : 1.0f;
	const size_t o = (size_t)qy * w + qx;
	if (a.rgb)
	{
		// the transpose of Y = .299 R + .587 G + .114 B, Cr = .5 + .713 (R - Y), Cb = .5 + .564 (B - Y)
		const float gy = gc[0] - 0.713f * gc[1] - 0.564f * gc[2];
		a.dimg[o] = s * (0.299f * gy + 0.713f * gc[1]);
		a.dimg[plane + o] = s * (0.587f * gy);
		a.dimg[2 * plane + o] = s * (0.114f * gy + 0.564f * gc[2]);
	}
	else
	{
		a.dimg[o] = s * gc[0]; a.dimg[plane + o] = s * gc[1]; a.dimg[2 * plane + o] = s * gc[2];
	}
}

// The adjoint of the resized load: dL/d(source) [3,hs,wsrc] from dL/d(resized) g [3,h,w] (k_hvs_bwd_image's output, written
// WITHOUT the upstream scalar, which multiplies each finished sum here: one rounding per element, so that an upstream gradient
// scales every element exactly, as in the plain call), a gather: one thread per source pixel, all three channels. The resized
// rows whose taps can be source row j have src in (j - 1, j + 1), i.e. d in ((j - .5) / ry - .5, (j + 1.5) / ry - .5); one more
// on each side against rounding, and each candidate's own hvs_lerp (the forward's) decides whether and with what weight it reads
// row j. Rows, then columns, in ascending order; sums in double, kept in fp32.
__global__ void __launch_bounds__(256) k_hvs_bwd_resize(HvsBwdResizeArgs a)
{
	const int sx = blockIdx.x * 64 + (threadIdx.x & 63), sy = blockIdx.y * 4 + (threadIdx.x >> 6);
	if (sx >= a.wsrc || sy >= a.hs) return;
	int ylo = max(0, (int)floor(((double)sy - 0.5) / a.ry - 0.5) - 1), yhi = min(a.h - 1, (int)ceil(((double)sy + 1.5) / a.ry - 0.5) + 1);
	int xlo = max(0, (int)floor(((double)sx - 0.5) / a.rx - 0.5) - 1), xhi = min(a.w - 1, (int)ceil(((double)sx + 1.5) / a.rx - 0.5) + 1);
	if (sy == 0) ylo = 0;
	if (sx == 0) xlo = 0;
	if (sy == a.hs - 1) yhi = a.h - 1;
	if (sx == a.wsrc - 1) xhi = a.w - 1;
	const size_t plane = (size_t)a.h * a.w;
	double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
	for (int y = ylo; y <= yhi; y++)
	{
		const HvsLerp ly = hvs_lerp(y, a.ry, a.hs);
		const double wy = (ly.i0 == sy ? ly.l0 : 0.0) + (ly.i1 == sy ? ly.l1 : 0.0);
		if (wy == 0.0) continue;
		const float *row = a.g + (size_t)y * a.w;
		for (int x = xlo; x <= xhi; x++)
		{
			const HvsLerp lx = hvs_lerp(x, a.rx, a.wsrc);
			const double wx = (lx.i0 == sx ? lx.l0 : 0.0) + (lx.i1 == sx ? lx.l1 : 0.0);
			if (wx == 0.0) continue;
			const double wt = wy * wx;
			acc0 += wt * (double)row[x]; acc1 += wt * (double)row[plane + x]; acc2 += wt * (double)row[2 * plane + x];
		}
	}
	const size_t splane = (size_t)a.hs * a.wsrc, o = (size_t)sy * a.wsrc + sx;
	const float s = a.gscale ? *a.gscale : 1.0f;
	a.dimg[o] = s * (float)acc0; a.dimg[splane + o] = s * (float)acc1; a.dimg[2 * splane + o] = s * (float)acc2;
}

// a resize of [3,Hs,Ws] to H x W the kernels take: no shrinking on either axis (no script does it; it would need another filter)
int hvs_resize_check(int Hs, int Ws, int H, int W)
{
	if (Hs <= 0 || Ws <= 0) { set_error("hvs: source size %dx%d is not positive", Hs, Ws); return FR_ERR_INVALID; }
	if (H < Hs || W < Ws) { set_error("hvs: shrinking %dx%d to %dx%d is unsupported (the resize size must be at least the source size)", Hs, Ws, H, W); return FR_ERR_INVALID; }
	return FR_OK;
}

static int hvs_group(long long window_elems) { return window_elems <= 16 ? 1 : (window_elems <= 256 ? 8 : 64); }

// ---------------------------------------------------------------- the launchers csrc/hvs_fov.hip uses (hvs_common.h)
void hvs_launch_level(bool resized, dim3 grid, hipStream_t stream, const HvsLevelArgs &a)
{
	if (resized) hipLaunchKernelGGL(k_hvs_level<true>, grid, dim3(256), 0, stream, a);
	else hipLaunchKernelGGL(k_hvs_level<false>, grid, dim3(256), 0, stream, a);
}

void hvs_launch_bwd_level(bool fov, dim3 grid, hipStream_t stream, const HvsBwdLevelArgs &a)
{
	if (fov) hipLaunchKernelGGL(k_hvs_bwd_level<true>, grid, dim3(256), 0, stream, a);
	else hipLaunchKernelGGL(k_hvs_bwd_level<false>, grid, dim3(256), 0, stream, a);
}

void hvs_launch_bwd_image(bool fov, dim3 grid, hipStream_t stream, const HvsBwdImageArgs &a)
{
	if (fov) hipLaunchKernelGGL(k_hvs_bwd_image<true>, grid, dim3(256), 0, stream, a);
	else hipLaunchKernelGGL(k_hvs_bwd_image<false>, grid, dim3(256), 0, stream, a);
}

void hvs_launch_bwd_resize(hipStream_t stream, const HvsBwdResizeArgs &a)
{
	hipLaunchKernelGGL(k_hvs_bwd_resize, dim3((a.wsrc + 63) / 64, (a.hs + 3) / 4), dim3(256), 0, stream, a);
}

void hvs_launch_cmp_direct(hipStream_t stream, const float *x, const float *y, long long n, int mse, float wgt, float *partials)
{
	hipLaunchKernelGGL(k_hvs_cmp_direct, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, stream, x, y, n, mse, wgt, partials);
}

void hvs_launch_finish(hipStream_t stream, int n, const float *partials, float *out)
{
	hipLaunchKernelGGL(k_hvs_finish, dim3(1), dim3(1024), 0, stream, n, partials, out);
}

} // namespace fr

using namespace fr;

extern "C" int64_t fr_hvs_workspace_floats(int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations, int32_t which)
{
	HvsPlan p;
	if (hvs_plan(H, W, pooling_size, n_levels, n_orientations, &p) != FR_OK) return -1;
	if (which == 0) return p.ws_floats;
	if (which == 1) return p.bwd_floats;
	if (which == 2) return p.n_partials;
	set_error("hvs: which must be 0 (forward state), 1 (backward workspace) or 2 (partial sums)");
	return -1;
}

// Hs = 0: img / target are [3,H,W]; else [3,Hs,Ws], resized to H x W in the level-0 load
static int hvs_forward(int Hs, int Ws, int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations, int32_t mse, int32_t rgb,
	const float *filters, const float *img, const float *target, float *state_img, float *state_target, float *partials, float *out, void *stream_)
{
	HvsPlan p;
	int rc = hvs_plan(H, W, pooling_size, n_levels, n_orientations, &p);
	if (rc != FR_OK) return rc;
	if (!filters || !img || !state_img || !state_target || !partials || !out) { set_error("hvs_forward: a required pointer is null"); return FR_ERR_INVALID; }
	hipStream_t stream = (hipStream_t)stream_;
	const int nside = target ? 2 : 1; // target == NULL: state_target already holds that target's state
	const float wstat = 1.0f / (float)p.nstats;
	for (int l = 0; l < p.L - 1; l++)
	{
		const HvsLevel &v = p.lv[l];
		HvsLevelArgs a;
		a.h = v.h; a.w = v.w; a.nb = p.nb; a.level0 = l == 0; a.rgb = rgb;
		a.src[0] = img; a.src[1] = target; a.ws[0] = state_img; a.ws[1] = state_target;
		a.low_in = v.low_in; a.maps = v.maps; a.low_out = v.low_out; a.filt = filters;
		a.hs = Hs; a.wsrc = Ws; a.ry = Hs ? (double)Hs / (double)H : 1.0; a.rx = Hs ? (double)Ws / (double)W : 1.0;
		const dim3 grid((v.w + HVS_T - 1) / HVS_T, (v.h + HVS_T - 1) / HVS_T, 3 * nside);
		if (l == 0 && Hs)
			hipLaunchKernelGGL(k_hvs_level<true>, grid, dim3(256), 0, stream, a);
		else
			hipLaunchKernelGGL(k_hvs_level<false>, grid, dim3(256), 0, stream, a);
		const size_t plane = (size_t)v.h * v.w;
		const float wgt = wstat / (float)(3 * plane);
		if (!v.identity)
		{
			HvsPoolArgs q;
			q.h = v.h; q.w = v.w; q.ph = v.ph; q.pw = v.pw; q.nmc = v.nm * 3;
			q.G = hvs_group((long long)((v.h + v.ph - 1) / v.ph + 1) * ((v.w + v.pw - 1) / v.pw + 1));
			q.ws[0] = state_img; q.ws[1] = state_target; q.maps = v.maps; q.pool = v.pool;
			const long long threads = (long long)q.nmc * v.ph * v.pw * q.G;
			hipLaunchKernelGGL(k_hvs_pool, dim3((unsigned)((threads + 255) / 256), nside), dim3(256), 0, stream, q);
			HvsCmpArgs c;
			c.h = v.h; c.w = v.w; c.ph = v.ph; c.pw = v.pw; c.nmc = v.nm * 3; c.mse = mse; c.sy = v.sy; c.sx = v.sx; c.wgt = wgt;
			c.wsi = state_img; c.wst = state_target; c.pool = v.pool; c.partials = partials + v.part;
			hipLaunchKernelGGL(k_hvs_cmp_pooled, dim3((unsigned)((plane + 255) / 256), v.nm * 3), dim3(256), 0, stream, c);
		}
		else
			hipLaunchKernelGGL(k_hvs_cmp_direct, dim3(v.part_n), dim3(256), 0, stream, state_img + v.maps, state_target + v.maps,
				(long long)v.nm * 3 * plane, mse, wgt, partials + v.part);
	}
	const long long last = p.lv[p.L - 2].low_out, nres = 3ll * p.lh * p.lw;
	hipLaunchKernelGGL(k_hvs_cmp_direct, dim3(p.res_part_n), dim3(256), 0, stream, state_img + last, state_target + last, nres, mse,
		wstat / (float)nres, partials + p.res_part);
	hipLaunchKernelGGL(k_hvs_finish, dim3(1), dim3(1024), 0, stream, (int)p.n_partials, partials, out);
	return check_launch("hvs_forward", stream, false);
}

extern "C" int fr_hvs_forward(int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations, int32_t mse, int32_t rgb,
	const float *filters, const float *img, const float *target, float *state_img, float *state_target, float *partials, float *out, void *stream_)
{
	return hvs_forward(0, 0, H, W, pooling_size, n_levels, n_orientations, mse, rgb, filters, img, target, state_img, state_target, partials, out, stream_);
}

extern "C" int fr_hvs_forward_resized(int32_t Hs, int32_t Ws, int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations,
	int32_t mse, int32_t rgb, const float *filters, const float *img, const float *target, float *state_img, float *state_target, float *partials,
	float *out, void *stream_)
{
	int rc = hvs_resize_check(Hs, Ws, H, W);
	if (rc != FR_OK) return rc;
	const bool same = Hs == H && Ws == W; // nothing to resize: the plain call
	return hvs_forward(same ? 0 : Hs, same ? 0 : Ws, H, W, pooling_size, n_levels, n_orientations, mse, rgb, filters, img, target, state_img, state_target,
		partials, out, stream_);
}

extern "C" int64_t fr_hvs_resized_backward_floats(int32_t Hs, int32_t Ws, int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations)
{
	HvsPlan p;
	if (hvs_resize_check(Hs, Ws, H, W) != FR_OK || hvs_plan(H, W, pooling_size, n_levels, n_orientations, &p) != FR_OK) return -1;
	return p.bwd_floats + ((Hs == H && Ws == W) ? 0 : 3ll * H * W); // the gradient before the resize's adjoint
}

// Hs = 0: dL_dimg is [3,H,W]; else [3,Hs,Ws], and the workspace holds 3 H W floats more, behind the plain one
static int hvs_backward(int Hs, int Ws, int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations, int32_t mse, int32_t rgb,
	const float *filters, const float *state_img, const float *state_target, float *workspace, const float *grad_scale, float *dL_dimg, void *stream_)
{
	HvsPlan p;
	int rc = hvs_plan(H, W, pooling_size, n_levels, n_orientations, &p);
	if (rc != FR_OK) return rc;
	if (!filters || !state_img || !state_target || !workspace || !dL_dimg) { set_error("hvs_backward: a required pointer is null"); return FR_ERR_INVALID; }
	hipStream_t stream = (hipStream_t)stream_;
	const float wstat = 1.0f / (float)p.nstats;
	const long long last = p.lv[p.L - 2].low_out;
	HvsGArgs g0 = {};
	for (int l = p.L - 2; l >= 0; l--)
	{
		const HvsLevel &v = p.lv[l];
		const size_t plane = (size_t)v.h * v.w;
		const float wgt = wstat / (float)(3 * plane);
		if (!v.identity)
		{
			HvsUpArgs u;
			u.h = v.h; u.w = v.w; u.ph = v.ph; u.pw = v.pw; u.nmc = v.nm * 3; u.mse = mse; u.sy = v.sy; u.sx = v.sx; u.wgt = wgt;
			u.G = hvs_group((long long)(2.0 / v.sy + 4.0) * (long long)(2.0 / v.sx + 4.0));
			u.wsi = state_img; u.wst = state_target; u.pool = v.pool; u.gpool = workspace + v.gpool;
			const long long threads = (long long)u.nmc * v.ph * v.pw * u.G;
			hipLaunchKernelGGL(k_hvs_bwd_up, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, u);
		}
		HvsBwdLevelArgs a = {};
		a.g.h = v.h; a.g.w = v.w; a.g.ph = v.ph; a.g.pw = v.pw; a.g.nmc = v.nm * 3; a.g.mse = mse; a.g.identity = v.identity; a.g.wgt = wgt;
		a.g.wsi = state_img; a.g.wst = state_target; a.g.maps = v.maps; a.g.gpool = workspace + v.gpool;
		a.nb = p.nb; a.m0 = l == 0 ? 1 : 0; a.last = l == p.L - 2;
		a.wres = wstat / (float)(3ll * p.lh * p.lw);
		a.filt = filters; a.glow_next = a.last ? nullptr : workspace + p.lv[l + 1].glow;
		a.low_i = state_img + last; a.low_t = state_target + last; a.glow = workspace + v.glow;
		hipLaunchKernelGGL(k_hvs_bwd_level<false>, dim3((v.w + HVS_T - 1) / HVS_T, (v.h + HVS_T - 1) / HVS_T, 3), dim3(256), 0, stream, a);
		if (l == 0) g0 = a.g;
	}
	HvsBwdImageArgs b = {};
	b.g = g0; b.rgb = rgb; b.filt = filters; b.glow0 = workspace + p.lv[0].glow;
	b.gscale = Hs ? nullptr : grad_scale; // (resized: k_hvs_bwd_resize applies it)
	b.dimg = Hs ? workspace + p.bwd_floats : dL_dimg;
	hipLaunchKernelGGL(k_hvs_bwd_image<false>, dim3((W + HVS_T - 1) / HVS_T, (H + HVS_T - 1) / HVS_T, 1), dim3(256), 0, stream, b);
	if (Hs)
	{
		HvsBwdResizeArgs r;
		r.h = H; r.w = W; r.hs = Hs; r.wsrc = Ws; r.ry = (double)Hs / (double)H; r.rx = (double)Ws / (double)W;
		r.g = workspace + p.bwd_floats; r.gscale = grad_scale; r.dimg = dL_dimg;
		hipLaunchKernelGGL(k_hvs_bwd_resize, dim3((Ws + 63) / 64, (Hs + 3) / 4), dim3(256), 0, stream, r);
	}
	return check_launch("hvs_backward", stream, false);
}

extern "C" int fr_hvs_backward(int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations, int32_t mse, int32_t rgb,
	const float *filters, const float *state_img, const float *state_target, float *workspace, const float *grad_scale, float *dL_dimg, void *stream_)
{
	return hvs_backward(0, 0, H, W, pooling_size, n_levels, n_orientations, mse, rgb, filters, state_img, state_target, workspace, grad_scale, dL_dimg, stream_);
}

extern "C" int fr_hvs_backward_resized(int32_t Hs, int32_t Ws, int32_t H, int32_t W, double pooling_size, int32_t n_levels, int32_t n_orientations,
	int32_t mse, int32_t rgb, const float *filters, const float *state_img, const float *state_target, float *workspace, const float *grad_scale,
	float *dL_dimg, void *stream_)
{
	int rc = hvs_resize_check(Hs, Ws, H, W);
	if (rc != FR_OK) return rc;
	const bool same = Hs == H && Ws == W;
	return hvs_backward(same ? 0 : Hs, same ? 0 : Ws, H, W, pooling_size, n_levels, n_orientations, mse, rgb, filters, state_img, state_target, workspace,
		grad_scale, dL_dimg, stream_);
}
