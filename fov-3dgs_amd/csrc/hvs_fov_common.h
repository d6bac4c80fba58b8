// fovraster -- what the foveated metameric loss (csrc/hvs_fov.hip) shares with the metamer's synthesis (csrc/metamer.hip): the
// layout of one picture's forward state (bands, both mip chains, lowpasses), the blended statistics at one pixel as device
// functions, and host launchers of the two kernels that fill the LOD maps and the mip chains. The kernels themselves are
// compiled once, in hvs_fov.hip.
#pragma once
#include "hvs_common.h"

namespace fr {

#define FOV_MAXK 16

struct FovChain
{
	int K;                                        // the last level: always 1x1
	int h[FOV_MAXK + 1], w[FOV_MAXK + 1];
	long long m[FOV_MAXK + 1], q[FOV_MAXK + 1];   // offsets (floats) of [nmc,h_k,w_k] in a side's forward state, k >= 1
};

struct FovMaps { int h, w, nmc; long long maps; FovChain c; };

struct FovLevel
{
	int nm;
	FovMaps a;
	long long low_in, low_out, lod;               // lod: offset in doubles
	long long part; int part_n;
	long long glow, g[FOV_MAXK + 1], gpart[FOV_MAXK + 1]; // backward workspace: [2,nmc,cells_k] and [S_k,2,nmc,cells_k]
	int G[FOV_MAXK + 1], S[FOV_MAXK + 1], R[FOV_MAXK + 1];
	int rows[FOV_MAXK + 1], cols[FOV_MAXK + 1];   // the footprint bound G, S and R were sized for (fr_hvs_fov_backward_plan reports it)
};

struct FovPlan
{
	int L, nb, H, W, lh, lw, nstats;
	FovLevel lv[HVS_MAXL];
	long long res_part; int res_part_n;
	long long ws_floats, bwd_floats, n_partials, lod_doubles, lodmax, gmap;
};

// the layout of an H x W call; `who` starts the error message of a refused size ("hvs_fov", "hvs_metamer")
int fov_plan(const char *who, int H, int W, int L, int nb, FovPlan *p);
// alpha, the display geometry and the gaze: finite, in range
int fov_check_view(const char *who, double alpha, double width, double distance, double gx, double gy);

struct FovLodArgs { int h, w, quadratic; double alpha, width, distance, gx, gy; double *lod; };

struct FovMipArgs { int nmc, hs, ws, hd, wd, first; float *st[2]; long long ms, qs, md, qd; };

// the level's LOD map [h,w] in double
void fov_launch_lod(hipStream_t stream, const FovLodArgs &a);
// every chain step of a level's maps, of nside pictures' states in the same launches
void fov_launch_chain(hipStream_t stream, const FovMaps &a, float *st0, float *st1, int nside);

// ---------------------------------------------------------------- the blended statistics at one pixel
// level k of map mc sampled at pixel (y, x): (mean, mean-square). Level 0 is the map (the bilinear sample at equal size is the
// pixel itself) and its square is formed in double; level K is the constant.
__device__ __forceinline__ void fov_sample(const float *__restrict__ st, const FovMaps &a, int mc, int k, int y, int x, double &M, double &Q)
{
	if (k == 0)
	{
		const double v = (double)st[a.maps + (size_t)mc * a.h * a.w + (size_t)y * a.w + x];
		M = v; Q = v * v;
		return;
	}
	const int hk = a.c.h[k], wk = a.c.w[k];
	const size_t o = (size_t)mc * hk * wk;
	const float *pm = st + a.c.m[k] + o, *pq = st + a.c.q[k] + o;
	if (k == a.c.K) { M = (double)pm[0]; Q = (double)pq[0]; return; }
	const HvsLerp ly = hvs_lerp(y, (double)hk / (double)a.h, hk), lx = hvs_lerp(x, (double)wk / (double)a.w, wk);
	M = hvs_bilerp(pm, wk, ly, lx); Q = hvs_bilerp(pq, wk, ly, lx);
}

// (the maps hold no negative LOD; fov_lod_of keeps an index in range whatever the buffer holds)
__device__ __forceinline__ double fov_lod_of(const double *__restrict__ lod, size_t i) { const double v = lod[i]; return v < 0.0 ? 0.0 : v; }

__device__ __forceinline__ HvsStat fov_stat(const float *__restrict__ st, const FovMaps &a, int mc, int y, int x, double lod)
{
	double M, Q;
	if (!(lod < (double)a.c.K))
		fov_sample(st, a, mc, a.c.K, y, x, M, Q);
	else
	{
		const int l = (int)lod;
		const double f = lod - (double)l;
		fov_sample(st, a, mc, l, y, x, M, Q);
		if (f != 0.0) // (f = 0: (1 - 0) a + 0 b = a in every precision)
		{
			double M1, Q1;
			fov_sample(st, a, mc, l + 1, y, x, M1, Q1);
			M = (1.0 - f) * M + f * M1; Q = (1.0 - f) * Q + f * Q1;
		}
	}
	HvsStat s;
	s.mean = M;
	s.var = Q - M * M;
	s.std = sqrt(s.var < HVS_VAR_FLOOR ? HVS_VAR_FLOOR : s.var);
	return s;
}

} // namespace fr
