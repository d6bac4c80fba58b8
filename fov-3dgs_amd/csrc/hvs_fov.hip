// fovraster -- the foveated (gaze-dependent) metameric loss, fused: MetamericLoss with use_bilinear_downup=True,
// use_l2_foveal_loss=False and the cropped 5x5 filters, the "HVS FOV" figure of hvs_loss_calc.py:21-75 (include/fovraster.h:
// fr_hvs_fov_*). It is the uniform loss (csrc/hvs.hip) with another blur stage: the pyramid, the colour conversion, the
// in-kernel resize, the pyramid's backward pass and the final sum are hvs.hip's kernels (hvs_common.h), launched from here.
//
// Reference behaviour:
//   metamer/odak_perception/foveation.py:6-91      pixel positions linspace(-.5, .5, n) times the displayed size, viewing distance
//                                                   as z; eccentricity = acos of the clamped dot product with the gaze direction
//                               :123-146            pooling = alpha ecc (times ecc: "quadratic"); an ellipse whose major axis is
//                                                   (tan(c + p/2) - tan(c - p/2)) d, c the eccentricity from the picture's CENTRE,
//                                                   minor axis 2 dist tan(p/2); side of the square of its area, in pixels
//                               :174-179            lod = max(0, log2(1e-6 + pooling))
//   metamer/odak_perception/radially_varying_blur.py:100-109 the mip chain: m_0 = x, m_{k+1} = area-halved m_k (size floor(n/2),
//                                                   adaptive windows [floor(j n / n'), ceil((j+1) n / n'))) while both sides
//                                                   exceed 1; a chain that stops at 1x2 gets the mean of the two as m_K
//                               :111-140            up_k = m_k bilinearly to full size (align_corners=False), up_K the constant;
//                                                   out = up_K where lod >= K, else (1 - f) up_l + f up_{l+1}, l = floor(lod)
//   metamer/odak_perception/metameric_loss.py:101-109 mean = blur(x), var = blur(x^2) - mean^2, below 1e-7 -> 1e-7, std
//                               :125-167            statistics: (mean, std) of h and of every band, a level's maps sharing the
//                                                   LOD map built at that level's size; the raw last lowpass
//                               :169-191            loss = mean over the statistics of their L1 / MSE mean
// A size on which the reference's own final broadcast fails (a level's chain ends at 1 x w', w' >= 3, or h' x 1, h' >= 2) is
// refused here too.
//
// Forward, per pyramid level:
//   k_fov_lod       the level's LOD map in double from gaze, size and the four parameters; kept by the caller (lod_valid).
//   k_fov_lodmax    the map's largest value, kept behind the maps: the backward pass skips the chain levels no pixel blends.
//   k_hvs_level     (hvs.hip) the bands and the next lowpass.
//   k_fov_mip       one launch per chain step, image and target in one launch: m_{k+1} and the chain of the SQUARE q_{k+1}
//                   (q_0 = x x is never stored: the first step squares in its load, sums in double).
//   k_fov_cmp       per pixel: the two bilinear samples of both chains of both pictures, the blend, mean and std in double (as
//                   hvs_stat and for its reason), |d| or d^2 summed per workgroup. x x is formed in double where level 0 is
//                   sampled, so where lod = 0 the variance is 0 exactly and the clamp never hangs on a stored square's rounding.
// Backward, all gathers (no atomics, no zero fills: the same bits on every run), per level, coarsest first:
//   k_fov_bwd_up    per mip texel of level k = K .. 1: over the texel's bilinear footprint, the pixels whose floor(lod) is k or
//                   k - 1 (or lod >= K for k = K), the blend weight times the bilinear weight times the pixel's derivative with
//                   respect to the blended mean and mean-square (recomputed). G lanes share a texel; a large footprint is cut
//                   into row slices whose sums are added, in slice order, by
//   k_fov_bwd_down  ... which also walks the adjoint of the area windows down the chain: level k collects from level k + 1.
//   k_fov_bwd_map   per pixel of every map: its own term (floor(lod) = 0) plus level 1's windows, g_x = g_mean + 2 x g_square,
//                   written to the workspace, from where k_hvs_bwd_level<FOV> / k_hvs_bwd_image<FOV> (hvs.hip) read it.
#include "hvs_fov_common.h"

namespace fr {

static int fov_group(long long elems) { return elems <= 16 ? 1 : (elems <= 256 ? 8 : 64); }

// (the layout structures, fov_sample and fov_stat: hvs_fov_common.h, shared with csrc/metamer.hip)
int fov_plan(const char *who, int H, int W, int L, int nb, FovPlan *p)
{
	if (L < 2 || L > HVS_MAXL) { set_error("%s: n_pyramid_levels %d outside 2..%d", who, L, HVS_MAXL); return FR_ERR_INVALID; }
	if (nb < 1 || nb > HVS_MAXB) { set_error("%s: %d orientations outside 1..%d", who, nb, HVS_MAXB); return FR_ERR_INVALID; }
	if (H <= 0 || W <= 0 || H % (1 << L) || W % (1 << L)) { set_error("%s: size %dx%d is not a multiple of 2^%d", who, H, W, L); return FR_ERR_INVALID; }
	if (H > 16384 || W > 16384) { set_error("%s: size %dx%d too large (max 16384)", who, H, W); return FR_ERR_INVALID; }
	p->L = L; p->nb = nb; p->H = H; p->W = W; p->nstats = 2 * (1 + (L - 1) * nb) + 1;
	long long ws = 0, bw = 0, np = 0, nl = 0;
	p->gmap = 0; bw += (long long)(nb + 1) * 3 * H * W; // the maps' gradients of one level at a time; level 0 is the largest
	for (int l = 0; l < L - 1; l++)
	{
		FovLevel &v = p->lv[l];
		const int h = H >> l, w = W >> l;
		v.nm = nb + (l == 0 ? 1 : 0);
		v.a.h = h; v.a.w = w; v.a.nmc = v.nm * 3;
		const long long plane = (long long)h * w;
		v.a.maps = ws; ws += (long long)v.a.nmc * plane;
		FovChain &c = v.a.c;
		int K = 0;
		c.h[0] = h; c.w[0] = w; c.m[0] = c.q[0] = 0;
		while (c.h[K] > 1 && c.w[K] > 1 && K < FOV_MAXK) { c.h[K + 1] = c.h[K] / 2; c.w[K + 1] = c.w[K] / 2; K++; }
		if (c.h[K] == 1 && c.w[K] == 2 && K < FOV_MAXK) { c.h[K + 1] = 1; c.w[K + 1] = 1; K++; }
		if (c.h[K] != 1 || c.w[K] != 1)
		{
			set_error("%s: pyramid level %d (%dx%d): its mip chain ends at %dx%d, not at 1x1 or 1x2; the reference's MetamericLoss "
				"fails on this size too (its final broadcast)", who, l, h, w, c.h[K], c.w[K]);
			return FR_ERR_INVALID;
		}
		c.K = K;
		v.lod = nl; nl += plane;
		v.glow = bw; bw += 3 * plane;
		for (int k = 1; k <= K; k++)
		{
			const long long cells = (long long)v.a.nmc * c.h[k] * c.w[k];
			c.m[k] = ws; ws += cells;
			c.q[k] = ws; ws += cells;
			// the footprint of a texel: the pixels whose two bilinear taps can name it (k_fov_bwd_up), all of them for the 1x1 level
			const int rows = k == K ? h : min(h, (int)(2.0 * h / c.h[k]) + 6), cols = k == K ? w : min(w, (int)(2.0 * w / c.w[k]) + 6);
			v.rows[k] = rows; v.cols[k] = cols;
			v.G[k] = fov_group((long long)rows * cols);
			int S = (int)min((long long)rows, ((long long)rows * cols + (long long)v.G[k] * 512 - 1) / ((long long)v.G[k] * 512));
			v.R[k] = (rows + S - 1) / S;
			v.S[k] = (rows + v.R[k] - 1) / v.R[k];
			v.g[k] = bw; bw += 2 * cells;
			v.gpart[k] = bw; bw += (long long)v.S[k] * 2 * cells;
		}
		v.part_n = (int)((plane + 255) / 256) * v.a.nmc;
		v.part = np; np += v.part_n;
		v.low_in = l == 0 ? 0 : p->lv[l - 1].low_out;
		v.low_out = ws; ws += 3 * (plane / 4);
	}
	p->lh = H >> (L - 1); p->lw = W >> (L - 1);
	p->res_part = np; p->res_part_n = (int)((3ll * p->lh * p->lw + 1023) / 1024); np += p->res_part_n;
	p->lodmax = nl; nl += HVS_MAXL; // every level's largest LOD, behind the maps
	p->ws_floats = ws; p->bwd_floats = bw; p->n_partials = np; p->lod_doubles = nl;
	return FR_OK;
}

// ---------------------------------------------------------------- the LOD map
// linspace(-.5, .5, n)[i], from the nearer end as torch steps it
__device__ __forceinline__ double fov_lin(int i, int n)
{
	if (n == 1) return -0.5;
	const double step = 1.0 / (double)(n - 1);
	return i < n / 2 ? -0.5 + step * (double)i : 0.5 - step * (double)(n - 1 - i);
}

__global__ void __launch_bounds__(256) k_fov_lod(FovLodArgs a)
{
	const int pix = blockIdx.x * 256 + threadIdx.x;
	if (pix >= a.h * a.w) return;
	const int y = pix / a.w, x = pix - y * a.w;
	const double height = (a.width / (double)a.w) * (double)a.h;
	const double px = fov_lin(x, a.w) * a.width, py = fov_lin(y, a.h) * height, pz = a.distance;
	const double dist = sqrt(px * px + py * py + pz * pz);
	double gx = (a.gx * 2.0 - 1.0) * a.width * 0.5, gy = (a.gy * 2.0 - 1.0) * height * 0.5, gz = a.distance;
	const double gn = sqrt(gx * gx + gy * gy + gz * gz);
	gx /= gn; gy /= gn; gz /= gn;
	double dot = gx * (px / dist) + gy * (py / dist) + gz * (pz / dist);
	dot = fmin(fmax(dot, -1.0), 1.0);
	const double ecc = acos(dot);
	const double centre = acos(fmin(fmax(pz / dist, -1.0), 1.0)); // the gaze (.5, .5): direction (0, 0, 1)
	double rad = a.alpha * ecc;
	if (a.quadratic) rad *= ecc;
	const double major = (tan(centre + rad * 0.5) - tan(centre - rad * 0.5)) * a.distance;
	const double minor = 2.0 * dist * tan(rad * 0.5);
	const double area = fabs(3.14159265358979323846 * major * minor * 0.25);
	const double pooling = (sqrt(area) / a.width) * (double)a.w;
	const double lod = log2(1e-6 + pooling);
	a.lod[pix] = lod < 0.0 ? 0.0 : lod; // (a NaN stays a NaN, as in the reference)
}

// the largest value of a level's map (a NaN counts as +inf: such a pixel reads the last chain level), one workgroup
__global__ void __launch_bounds__(1024) k_fov_lodmax(const double *__restrict__ lod, int n, double *__restrict__ out)
{
	__shared__ double s0[1024];
	double m = 0.0;
	for (int i = threadIdx.x; i < n; i += 1024)
	{
		const double v = lod[i];
		m = fmax(m, v != v ? (double)INFINITY : v);
	}
	s0[threadIdx.x] = m;
	__syncthreads();
	for (int off = 512; off > 0; off >>= 1)
	{
		if ((int)threadIdx.x < off) s0[threadIdx.x] = fmax(s0[threadIdx.x], s0[threadIdx.x + off]);
		__syncthreads();
	}
	if (threadIdx.x == 0) out[0] = s0[0];
}

// ---------------------------------------------------------------- the mip chains
// one chain step of every map: destination cell (jy, jx) = the mean over its adaptive window of the source level; first: the
// source is the map itself and the square's source is x x, formed here in double
__global__ void __launch_bounds__(256) k_fov_mip(FovMipArgs a)
{
	const int cell = blockIdx.x * 256 + threadIdx.x, mc = blockIdx.y;
	if (cell >= a.hd * a.wd) return;
	float *st = a.st[blockIdx.z];
	const int jy = cell / a.wd, jx = cell - jy * a.wd;
	const int ys = (int)(((long long)jy * a.hs) / a.hd), ye = (int)(((long long)(jy + 1) * a.hs + a.hd - 1) / a.hd);
	const int xs = (int)(((long long)jx * a.ws) / a.wd), xe = (int)(((long long)(jx + 1) * a.ws + a.wd - 1) / a.wd);
	const size_t so = (size_t)mc * a.hs * a.ws;
	const float *pm = st + a.ms + so, *pq = st + a.qs + so;
	double s = 0.0, q = 0.0;
	for (int y = ys; y < ye; y++)
		for (int x = xs; x < xe; x++)
		{
			const double v = (double)pm[(size_t)y * a.ws + x];
			s += v;
			q += a.first ? v * v : (double)pq[(size_t)y * a.ws + x];
		}
	const double cnt = (double)((ye - ys) * (xe - xs));
	const size_t o = (size_t)mc * a.hd * a.wd + cell;
	st[a.md + o] = (float)(s / cnt);
	st[a.qd + o] = (float)(q / cnt);
}

// ---------------------------------------------------------------- the launchers csrc/metamer.hip uses (hvs_fov_common.h)
void fov_launch_lod(hipStream_t stream, const FovLodArgs &a)
{
	hipLaunchKernelGGL(k_fov_lod, dim3((unsigned)(((long long)a.h * a.w + 255) / 256)), dim3(256), 0, stream, a);
}

void fov_launch_chain(hipStream_t stream, const FovMaps &a, float *st0, float *st1, int nside)
{
	const FovChain &c = a.c;
	for (int k = 0; k < c.K; k++)
	{
		FovMipArgs m;
		m.nmc = a.nmc; m.hs = c.h[k]; m.ws = c.w[k]; m.hd = c.h[k + 1]; m.wd = c.w[k + 1]; m.first = k == 0;
		m.st[0] = st0; m.st[1] = st1;
		m.ms = k == 0 ? a.maps : c.m[k]; m.qs = k == 0 ? a.maps : c.q[k]; m.md = c.m[k + 1]; m.qd = c.q[k + 1];
		hipLaunchKernelGGL(k_fov_mip, dim3((unsigned)(((long long)m.hd * m.wd + 255) / 256), a.nmc, nside), dim3(256), 0, stream, m);
	}
}

// ---------------------------------------------------------------- the blended statistics at one pixel: fov_stat (hvs_fov_common.h)
struct FovCmpArgs { FovMaps a; int mse; float wgt; const float *wsi, *wst; const double *lod; float *partials; };

__global__ void __launch_bounds__(256) k_fov_cmp(FovCmpArgs a)
{
	__shared__ double s_red[4];
	const int pix = blockIdx.x * 256 + threadIdx.x, mc = blockIdx.y;
	double acc = 0.0;
	if (pix < a.a.h * a.a.w)
	{
		const int y = pix / a.a.w, x = pix - y * a.a.w;
		const double lod = fov_lod_of(a.lod, pix);
		const HvsStat A = fov_stat(a.wsi, a.a, mc, y, x, lod), B = fov_stat(a.wst, a.a, mc, y, x, lod);
		const double dm = A.mean - B.mean, ds = A.std - B.std;
		acc = a.mse ? dm * dm + ds * ds : fabs(dm) + fabs(ds);
	}
	const double t = hvs_block_sum(acc, s_red);
	if (threadIdx.x == 0) a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (float)(t * (double)a.wgt);
}

// ---------------------------------------------------------------- backward
struct FovUpArgs { FovMaps a; int k, G, S, R, mse; float wgt; const float *wsi, *wst; const double *lod, *lodmax; float *part; };

// G lanes (1, 8 or 64) share one texel of level k and one row slice (blockIdx.y) of its footprint: part[slice][mean | square][texel].
// Level k is blended only by pixels with floor(lod) = k - 1 or k (or lod >= K = k): above floor(largest LOD) + 1 it gets zeros.
__global__ void __launch_bounds__(256) k_fov_bwd_up(FovUpArgs a)
{
	const int G = a.G, lane = threadIdx.x & (G - 1), k = a.k, K = a.a.c.K, h = a.a.h, w = a.a.w;
	const int hk = a.a.c.h[k], wk = a.a.c.w[k];
	const long long cell = ((long long)blockIdx.x * 256 + threadIdx.x) / G, cells = (long long)hk * wk, ncell = (long long)a.a.nmc * cells;
	const bool valid = cell < ncell;
	const double sy = (double)hk / (double)h, sx = (double)wk / (double)w;
	float gm = 0.0f, gq = 0.0f;
	if (valid)
	{
		const int mc = (int)(cell / cells), rem = (int)(cell - (long long)mc * cells), jy = rem / wk, jx = rem - jy * wk;
		int ylo = 0, yhi = h - 1, xlo = 0, xhi = w - 1;
		if (k != K)
		{
			// the pixels whose two source rows can include jy: src in [jy - 1, jy + 1), one more on each side against rounding; each
			// pixel's own weights (computed as the forward does) decide
			ylo = max(0, (int)floor(((double)jy - 0.5) / sy - 0.5) - 1); yhi = min(h - 1, (int)ceil(((double)jy + 1.5) / sy - 0.5) + 1);
			xlo = max(0, (int)floor(((double)jx - 0.5) / sx - 0.5) - 1); xhi = min(w - 1, (int)ceil(((double)jx + 1.5) / sx - 0.5) + 1);
			if (jy == 0) ylo = 0;
			if (jx == 0) xlo = 0;
			if (jy == hk - 1) yhi = h - 1;
			if (jx == wk - 1) xhi = w - 1;
		}
		const int slice = blockIdx.y;
		const int ys = ylo + slice * a.R, ye = slice == a.S - 1 ? yhi : min(yhi, ys + a.R - 1);
		const bool unused = (double)k > floor(*a.lodmax) + 1.0;
		const int nw = xhi - xlo + 1, cnt = (!unused && nw > 0 && ye >= ys) ? (ye - ys + 1) * nw : 0;
		for (int e = lane; e < cnt; e += G)
		{
			const int y = ys + e / nw, x = xlo + e % nw;
			const double lod = fov_lod_of(a.lod, (size_t)y * w + x);
			double c;
			if (!(lod < (double)K))
			{
				if (k != K) continue;
				c = 1.0;
			}
			else
			{
				const int l = (int)lod;
				const double f = lod - (double)l;
				if (l == k) c = 1.0 - f;
				else if (l + 1 == k) c = f;
				else continue;
				if (c == 0.0) continue;
				if (k != K)
				{
					const HvsLerp ly = hvs_lerp(y, sy, hk), lx = hvs_lerp(x, sx, wk);
					const double wy = (ly.i0 == jy ? ly.l0 : 0.0) + (ly.i1 == jy ? ly.l1 : 0.0);
					const double wx = (lx.i0 == jx ? lx.l0 : 0.0) + (lx.i1 == jx ? lx.l1 : 0.0);
					c *= wy * wx;
				}
			}
			const float wt = (float)c;
			if (wt != 0.0f)
			{
				float dmean, dmsq;
				hvs_pix_grad(fov_stat(a.wsi, a.a, mc, y, x, lod), fov_stat(a.wst, a.a, mc, y, x, lod), a.mse, a.wgt, dmean, dmsq);
				gm += wt * dmean; gq += wt * dmsq;
			}
		}
	}
	for (int off = G >> 1; off > 0; off >>= 1) { gm += __shfl_xor(gm, off); gq += __shfl_xor(gq, off); }
	if (valid && lane == 0)
	{
		float *part = a.part + (size_t)blockIdx.y * 2 * ncell;
		part[cell] = gm; part[ncell + cell] = gq;
	}
}

struct FovDownArgs { int nmc, hk, wk, hp, wp, S, top; const float *part, *gparent; float *g; };

// g[mean | square][texel] of level k = the slices' sums in slice order, plus (unless level k is the top) the adjoint of the area
// windows of level k + 1: every parent cell whose window holds the texel gives its gradient over its window's size
__global__ void __launch_bounds__(256) k_fov_bwd_down(FovDownArgs a)
{
	const long long cells = (long long)a.hk * a.wk, ncell = (long long)a.nmc * cells;
	const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
	if (idx >= 2 * ncell) return;
	const int which = (int)(idx / ncell);
	const long long r = idx - (long long)which * ncell;
	float acc = 0.0f;
	for (int s = 0; s < a.S; s++) acc += a.part[((size_t)s * 2 + which) * ncell + r];
	if (!a.top)
	{
		const int mc = (int)(r / cells), rem = (int)(r - (long long)mc * cells), y = rem / a.wk, x = rem - y * a.wk;
		const float *gp = a.gparent + ((size_t)which * a.nmc + mc) * a.hp * a.wp;
		const int jylo = max(0, (int)(((long long)y * a.hp) / a.hk) - 1), jyhi = min(a.hp - 1, (int)(((long long)(y + 1) * a.hp + a.hk - 1) / a.hk) + 1);
		const int jxlo = max(0, (int)(((long long)x * a.wp) / a.wk) - 1), jxhi = min(a.wp - 1, (int)(((long long)(x + 1) * a.wp + a.wk - 1) / a.wk) + 1);
		for (int jy = jylo; jy <= jyhi; jy++)
		{
			const int ys = (int)(((long long)jy * a.hk) / a.hp), ye = (int)(((long long)(jy + 1) * a.hk + a.hp - 1) / a.hp);
			if (y < ys || y >= ye) continue;
			for (int jx = jxlo; jx <= jxhi; jx++)
			{
				const int xs = (int)(((long long)jx * a.wk) / a.wp), xe = (int)(((long long)(jx + 1) * a.wk + a.wp - 1) / a.wp);
				if (x < xs || x >= xe) continue;
				acc += gp[jy * a.wp + jx] / (float)((ye - ys) * (xe - xs));
			}
		}
	}
	a.g[idx] = acc;
}

struct FovMapArgs { FovMaps a; int mse; float wgt; const float *wsi, *wst, *g1; const double *lod; float *gmap; };

// d loss / d map[mc](y, x): the pixel's own term where floor(lod) = 0 (weight 1 - f on level 0) plus level 1's windows that
// hold it, combined as g_mean + 2 x g_square
__global__ void __launch_bounds__(256) k_fov_bwd_map(FovMapArgs a)
{
	const int pix = blockIdx.x * 256 + threadIdx.x, mc = blockIdx.y, h = a.a.h, w = a.a.w;
	if (pix >= h * w) return;
	const int y = pix / w, x = pix - y * w;
	const double lod = fov_lod_of(a.lod, pix);
	const float xv = a.wsi[a.a.maps + (size_t)mc * h * w + pix];
	float acc = 0.0f;
	if (lod < 1.0) // (K >= 1 always)
	{
		float dmean, dmsq;
		hvs_pix_grad(fov_stat(a.wsi, a.a, mc, y, x, lod), fov_stat(a.wst, a.a, mc, y, x, lod), a.mse, a.wgt, dmean, dmsq);
		const float c = (float)(1.0 - lod);
		acc = c * dmean + 2.0f * xv * (c * dmsq);
	}
	const int h1 = a.a.c.h[1], w1 = a.a.c.w[1];
	const size_t cells = (size_t)h1 * w1;
	const float *gm = a.g1 + mc * cells, *gq = a.g1 + ((size_t)a.a.nmc + mc) * cells;
	const int jylo = max(0, (int)(((long long)y * h1) / h) - 1), jyhi = min(h1 - 1, (int)(((long long)(y + 1) * h1 + h - 1) / h) + 1);
	const int jxlo = max(0, (int)(((long long)x * w1) / w) - 1), jxhi = min(w1 - 1, (int)(((long long)(x + 1) * w1 + w - 1) / w) + 1);
	for (int jy = jylo; jy <= jyhi; jy++)
	{
		const int ys = (int)(((long long)jy * h) / h1), ye = (int)(((long long)(jy + 1) * h + h1 - 1) / h1);
		if (y < ys || y >= ye) continue;
		for (int jx = jxlo; jx <= jxhi; jx++)
		{
			const int xs = (int)(((long long)jx * w) / w1), xe = (int)(((long long)(jx + 1) * w + w1 - 1) / w1);
			if (x < xs || x >= xe) continue;
			acc += (gm[jy * w1 + jx] + 2.0f * xv * gq[jy * w1 + jx]) / (float)((ye - ys) * (xe - xs));
		}
	}
	a.gmap[(size_t)mc * h * w + pix] = acc;
}

static int fov_check(int Hs, int Ws, int H, int W, double alpha, double width, double distance, double gx, double gy)
{
	if (Hs || Ws)
	{
		int rc = hvs_resize_check(Hs, Ws, H, W);
		if (rc != FR_OK) return rc;
	}
	return fov_check_view("hvs_fov", alpha, width, distance, gx, gy);
}

int fov_check_view(const char *who, double alpha, double width, double distance, double gx, double gy)
{
	if (!(alpha >= 0.0) || !(alpha < 1e6)) { set_error("%s: alpha must be finite and not negative", who); return FR_ERR_INVALID; }
	if (!(width > 0.0) || !(width < 1e9) || !(distance > 0.0) || !(distance < 1e9))
	{
		set_error("%s: real_image_width and real_viewing_distance must be positive and finite", who);
		return FR_ERR_INVALID;
	}
	if (!(fabs(gx) < 1e6) || !(fabs(gy) < 1e6)) { set_error("%s: the gaze must be finite", who); return FR_ERR_INVALID; }
	return FR_OK;
}

} // namespace fr

using namespace fr;

extern "C" int64_t fr_hvs_fov_workspace_floats(int32_t Hs, int32_t Ws, int32_t H, int32_t W, int32_t n_levels, int32_t n_orientations, int32_t which)
{
	FovPlan p;
	if ((Hs || Ws) && hvs_resize_check(Hs, Ws, H, W) != FR_OK) return -1;
	if (fov_plan("hvs_fov", H, W, n_levels, n_orientations, &p) != FR_OK) return -1;
	const bool resized = (Hs || Ws) && !(Hs == H && Ws == W);
	if (which == 0) return p.ws_floats;
	if (which == 1) return p.bwd_floats + (resized ? 3ll * H * W : 0);
	if (which == 2) return p.n_partials;
	if (which == 3) return 2 * p.lod_doubles;
	set_error("hvs_fov: which must be 0 (forward state), 1 (backward workspace), 2 (partial sums) or 3 (LOD maps)");
	return -1;
}

extern "C" int fr_hvs_fov_backward_plan(int32_t H, int32_t W, int32_t n_levels, int32_t n_orientations, int32_t level, int32_t k, int64_t *out)
{
	FovPlan p;
	if (fov_plan("hvs_fov", H, W, n_levels, n_orientations, &p) != FR_OK) return FR_ERR_INVALID;
	if (level < 0 || level > p.L - 2) { set_error("hvs_fov_backward_plan: pyramid level %d outside 0..%d", level, p.L - 2); return FR_ERR_INVALID; }
	const FovLevel &v = p.lv[level];
	if (k < 1 || k > v.a.c.K) { set_error("hvs_fov_backward_plan: chain level %d outside 1..%d (pyramid level %d)", k, v.a.c.K, level); return FR_ERR_INVALID; }
	if (!out) { set_error("hvs_fov_backward_plan: out is null"); return FR_ERR_INVALID; }
	out[0] = v.a.c.K; out[1] = v.a.c.h[k]; out[2] = v.a.c.w[k]; out[3] = v.rows[k]; out[4] = v.cols[k];
	out[5] = v.G[k]; out[6] = v.S[k]; out[7] = v.R[k]; out[8] = v.g[k]; out[9] = v.gpart[k];
	return FR_OK;
}

extern "C" int fr_hvs_fov_forward(int32_t Hs, int32_t Ws, int32_t H, int32_t W, double alpha, double real_image_width, double real_viewing_distance,
	int32_t mode, double gaze_x, double gaze_y, int32_t n_levels, int32_t n_orientations, int32_t mse, int32_t rgb, const float *filters,
	const float *img, const float *target, float *state_img, float *state_target, float *lod, int32_t lod_valid, float *partials, float *out,
	void *stream_)
{
	FovPlan p;
	int rc = fov_check(Hs, Ws, H, W, alpha, real_image_width, real_viewing_distance, gaze_x, gaze_y);
	if (rc != FR_OK) return rc;
	if ((rc = fov_plan("hvs_fov", H, W, n_levels, n_orientations, &p)) != FR_OK) return rc;
	if (mode != 0 && mode != 1) { set_error("hvs_fov: mode must be 0 (linear) or 1 (quadratic)"); return FR_ERR_INVALID; }
	if (!filters || !img || !state_img || !state_target || !lod || !partials || !out) { set_error("hvs_fov_forward: a required pointer is null"); return FR_ERR_INVALID; }
	if ((uintptr_t)lod & 7) { set_error("hvs_fov_forward: lod must be 8-byte aligned (it holds doubles)"); return FR_ERR_INVALID; }
	if (Hs == H && Ws == W) Hs = Ws = 0; // nothing to resize: the plain call
	hipStream_t stream = (hipStream_t)stream_;
	const int nside = target ? 2 : 1; // target == NULL: state_target already holds that target's state
	const float wstat = 1.0f / (float)p.nstats;
	double *lodd = (double *)lod;
	for (int l = 0; l < p.L - 1; l++)
	{
		const FovLevel &v = p.lv[l];
		const int h = v.a.h, w = v.a.w;
		const size_t plane = (size_t)h * w;
		if (!lod_valid)
		{
			FovLodArgs q;
			q.h = h; q.w = w; q.quadratic = mode; q.alpha = alpha; q.width = real_image_width; q.distance = real_viewing_distance;
			q.gx = gaze_x; q.gy = gaze_y; q.lod = lodd + v.lod;
			hipLaunchKernelGGL(k_fov_lod, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, stream, q);
			hipLaunchKernelGGL(k_fov_lodmax, dim3(1), dim3(1024), 0, stream, (const double *)q.lod, (int)plane, lodd + p.lodmax + l);
		}
		HvsLevelArgs a;
		a.h = h; a.w = w; a.nb = p.nb; a.level0 = l == 0; a.rgb = rgb;
		a.src[0] = img; a.src[1] = target; a.ws[0] = state_img; a.ws[1] = state_target;
		a.low_in = v.low_in; a.maps = v.a.maps; a.low_out = v.low_out; a.filt = filters;
		a.hs = Hs; a.wsrc = Ws; a.ry = Hs ? (double)Hs / (double)H : 1.0; a.rx = Hs ? (double)Ws / (double)W : 1.0;
		hvs_launch_level(l == 0 && Hs, dim3((w + HVS_T - 1) / HVS_T, (h + HVS_T - 1) / HVS_T, 3 * nside), stream, a);
		fov_launch_chain(stream, v.a, state_img, state_target, nside);
		FovCmpArgs q;
		q.a = v.a; q.mse = mse; q.wgt = wstat / (float)(3 * plane); q.wsi = state_img; q.wst = state_target; q.lod = lodd + v.lod;
		q.partials = partials + v.part;
		hipLaunchKernelGGL(k_fov_cmp, dim3((unsigned)((plane + 255) / 256), v.a.nmc), dim3(256), 0, stream, q);
	}
	const long long last = p.lv[p.L - 2].low_out, nres = 3ll * p.lh * p.lw;
	hvs_launch_cmp_direct(stream, state_img + last, state_target + last, nres, mse, wstat / (float)nres, partials + p.res_part);
	hvs_launch_finish(stream, (int)p.n_partials, partials, out);
	return check_launch("hvs_fov_forward", stream, false);
}

extern "C" int fr_hvs_fov_backward(int32_t Hs, int32_t Ws, int32_t H, int32_t W, double alpha, double real_image_width, double real_viewing_distance,
	int32_t mode, double gaze_x, double gaze_y, int32_t n_levels, int32_t n_orientations, int32_t mse, int32_t rgb, const float *filters,
	const float *state_img, const float *state_target, const float *lod, float *workspace, const float *grad_scale, float *dL_dimg, void *stream_)
{
	FovPlan p;
	int rc = fov_check(Hs, Ws, H, W, alpha, real_image_width, real_viewing_distance, gaze_x, gaze_y);
	if (rc != FR_OK) return rc;
	if ((rc = fov_plan("hvs_fov", H, W, n_levels, n_orientations, &p)) != FR_OK) return rc;
	if (!filters || !state_img || !state_target || !lod || !workspace || !dL_dimg) { set_error("hvs_fov_backward: a required pointer is null"); return FR_ERR_INVALID; }
	if ((uintptr_t)lod & 7) { set_error("hvs_fov_backward: lod must be 8-byte aligned (it holds doubles)"); return FR_ERR_INVALID; }
	if (Hs == H && Ws == W) Hs = Ws = 0;
	hipStream_t stream = (hipStream_t)stream_;
	const float wstat = 1.0f / (float)p.nstats;
	const long long last = p.lv[p.L - 2].low_out;
	const double *lodd = (const double *)lod;
	float *gmap = workspace + p.gmap;
	HvsGArgs g0 = {};
	for (int l = p.L - 2; l >= 0; l--)
	{
		const FovLevel &v = p.lv[l];
		const int h = v.a.h, w = v.a.w;
		const size_t plane = (size_t)h * w;
		const float wgt = wstat / (float)(3 * plane);
		const FovChain &c = v.a.c;
		for (int k = c.K; k >= 1; k--)
		{
			const long long ncell = (long long)v.a.nmc * c.h[k] * c.w[k];
			FovUpArgs u;
			u.a = v.a; u.k = k; u.G = v.G[k]; u.S = v.S[k]; u.R = v.R[k]; u.mse = mse; u.wgt = wgt; u.wsi = state_img; u.wst = state_target;
			u.lod = lodd + v.lod; u.lodmax = lodd + p.lodmax + l; u.part = workspace + v.gpart[k];
			hipLaunchKernelGGL(k_fov_bwd_up, dim3((unsigned)((ncell * u.G + 255) / 256), v.S[k]), dim3(256), 0, stream, u);
			FovDownArgs d;
			d.nmc = v.a.nmc; d.hk = c.h[k]; d.wk = c.w[k]; d.top = k == c.K; d.hp = d.top ? 1 : c.h[k + 1]; d.wp = d.top ? 1 : c.w[k + 1];
			d.S = v.S[k]; d.part = workspace + v.gpart[k]; d.gparent = d.top ? nullptr : workspace + v.g[k + 1]; d.g = workspace + v.g[k];
			hipLaunchKernelGGL(k_fov_bwd_down, dim3((unsigned)((2 * ncell + 255) / 256)), dim3(256), 0, stream, d);
		}
		FovMapArgs m;
		m.a = v.a; m.mse = mse; m.wgt = wgt; m.wsi = state_img; m.wst = state_target; m.g1 = workspace + v.g[1]; m.lod = lodd + v.lod; m.gmap = gmap;
		hipLaunchKernelGGL(k_fov_bwd_map, dim3((unsigned)((plane + 255) / 256), v.a.nmc), dim3(256), 0, stream, m);
		HvsBwdLevelArgs a = {};
		a.g.h = h; a.g.w = w; a.g.nmc = v.a.nmc; a.g.mse = mse; a.g.wgt = wgt;
		a.g.wsi = state_img; a.g.wst = state_target; a.g.maps = v.a.maps; a.g.gpool = gmap;
		a.nb = p.nb; a.m0 = l == 0 ? 1 : 0; a.last = l == p.L - 2;
		a.wres = wstat / (float)(3ll * p.lh * p.lw);
		a.filt = filters; a.glow_next = a.last ? nullptr : workspace + p.lv[l + 1].glow;
		a.low_i = state_img + last; a.low_t = state_target + last; a.glow = workspace + v.glow;
		hvs_launch_bwd_level(true, dim3((w + HVS_T - 1) / HVS_T, (h + HVS_T - 1) / HVS_T, 3), stream, a);
		if (l == 0) g0 = a.g;
	}
	HvsBwdImageArgs b = {};
	b.g = g0; b.rgb = rgb; b.filt = filters; b.glow0 = workspace + p.lv[0].glow;
	b.gscale = Hs ? nullptr : grad_scale; // (resized: k_hvs_bwd_resize applies it)
	b.dimg = Hs ? workspace + p.bwd_floats : dL_dimg;
	hvs_launch_bwd_image(true, dim3((W + HVS_T - 1) / HVS_T, (H + HVS_T - 1) / HVS_T, 1), stream, b);
	if (Hs)
	{
		HvsBwdResizeArgs r;
		r.h = H; r.w = W; r.hs = Hs; r.wsrc = Ws; r.ry = (double)Hs / (double)H; r.rx = (double)Ws / (double)W;
		r.g = workspace + p.bwd_floats; r.gscale = grad_scale; r.dimg = dL_dimg;
		hvs_launch_bwd_resize(stream, r);
	}
	return check_launch("hvs_fov_backward", stream, false);
}
