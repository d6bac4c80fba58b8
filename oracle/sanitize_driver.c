/*
 * sanitize_driver.c -- the CPU oracle's foveated forward under AddressSanitizer / UBSan, as a stand-alone program.
 * TEST INFRASTRUCTURE ONLY (tests/test_oracle_sanitized_cpu.py builds and runs it).
 *
 * Build and run (from the repository root):
 *   gcc -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan -fno-sanitize-recover=all -fopenmp -ffp-contract=off -o /tmp/orc_san oracle/sanitize_driver.c -lm && /tmp/orc_san
 *
 * One and 64 Gaussians in front of an identity camera, frames 1x1, 2x2, 3x40 (every tile centre lies outside the frame:
 * the tile level is NaN), 17x15 (a tile with tile_min <= -1) and 16x16, 200x120, 15x1, 8x8, every foveated variant. Every output array is a malloc of exactly the
 * size oracle/oracle.py allocates, so a write past its end is a heap-buffer-overflow. Prints one line per frame and exits
 * with 0 when nothing was reported.
 */
#include <stdio.h>
#include "fovraster_oracle.c"

static real *reals(size_t n, real v)
{
	real *p = (real *)malloc(sizeof(real) * (n ? n : 1));
	for (size_t i = 0; i < n; i++) p[i] = v;
	return p;
}

static unsigned rng_state = 12345u;
static real rnd(void) /* [0, 1) */
{
	rng_state = rng_state * 1664525u + 1013904223u;
	return (real)(rng_state >> 8) / (real)16777216.0f;
}

static int64_t run(int variant, int P, int W, int H, int *nan_tiles, int *visible)
{
	const int T = ((W + 15) / 16) * ((H + 15) / 16), M = variant == ORC_RF ? 15 : 16;
	const real fovx = (real)1.2f;
	const real tfx = r_tan(fovx / 2), tfy = tfx * (real)H / (real)W;
	const real zn = (real)0.01f, zf = (real)100.0f;
	/* row-vector convention (as the reference's transposed matrices): identity view, perspective projection */
	real view[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
	real proj[16] = { 1 / tfx, 0, 0, 0, 0, 1 / tfy, 0, 0, 0, 0, zf / (zf - zn), 1, 0, 0, -(zf * zn) / (zf - zn), 0 };
	real campos[3] = { 0, 0, 0 }, bg[3] = { (real)0.3f, (real)0.1f, (real)0.25f };
	orc_in in;
	memset(&in, 0, sizeof in);
	in.variant = variant; in.P = P; in.D = 3; in.M = M; in.W = W; in.H = H;
	in.tanfovx = tfx; in.tanfovy = tfy; in.scale_modifier = 1;
	in.gaze_x = (real)0.4f; in.gaze_y = (real)0.55f; in.alpha = (real)0.6f;
	in.bg = bg; in.viewmatrix = view; in.projmatrix = proj; in.campos = campos;
	real *means = reals((size_t)3 * P, 0), *scales = reals((size_t)3 * P, 0), *rots = reals((size_t)4 * P, 0);
	const int fov_rows = variant == ORC_RF;
	real *opac = reals((size_t)P * (fov_rows ? FOV_NUM : 1), 0), *shs = reals((size_t)P * M * 3, 0);
	real *dcs = reals((size_t)P * FOV_NUM * 3, 0), *hl = reals((size_t)P, 0);
	for (int i = 0; i < P; i++)
	{
		means[3 * i] = (rnd() - (real)0.5f) * (real)1.5f; means[3 * i + 1] = (rnd() - (real)0.5f) * (real)1.5f;
		means[3 * i + 2] = (real)2 + (real)3 * rnd();
		for (int k = 0; k < 3; k++) scales[3 * i + k] = (real)0.02f + (real)0.6f * rnd() * rnd();
		rots[4 * i] = 1; rots[4 * i + 1] = rnd() - (real)0.5f; rots[4 * i + 2] = rnd() - (real)0.5f; rots[4 * i + 3] = rnd() - (real)0.5f;
		real nq = r_sqrt(rots[4 * i] * rots[4 * i] + rots[4 * i + 1] * rots[4 * i + 1] + rots[4 * i + 2] * rots[4 * i + 2] + rots[4 * i + 3] * rots[4 * i + 3]);
		for (int k = 0; k < 4; k++) rots[4 * i + k] /= nq;
		for (int k = 0; k < (fov_rows ? FOV_NUM : 1); k++) opac[(size_t)i * (fov_rows ? FOV_NUM : 1) + k] = (real)0.05f + (real)0.9f * rnd();
		for (int k = 0; k < M * 3; k++) shs[(size_t)i * M * 3 + k] = (rnd() - (real)0.5f) * (real)0.3f;
		for (int k = 0; k < FOV_NUM * 3; k++) dcs[(size_t)i * FOV_NUM * 3 + k] = rnd() * (real)2;
		hl[i] = (real)(i % FOV_NUM);
	}
	in.means3D = means; in.scales = scales; in.rotations = rots; in.opacities = opac; in.shs = shs; in.shs_dcs = dcs; in.highest_levels = hl;
	in.cur_level = 1;
	int64_t n = 0, capacity = 0;
	for (int pass = 0; pass < 2; pass++)
	{
		orc_out o;
		memset(&o, 0, sizeof o);
		o.depths = reals(P, 0); o.radii = (int32_t *)calloc(P, 4); o.means2D = reals((size_t)2 * P, 0); o.cov3D = reals((size_t)6 * P, 0);
		o.conic = reals((size_t)3 * P, 0); o.rgb = reals((size_t)3 * P, 0); o.clamped = (uint8_t *)calloc((size_t)3 * P, 1);
		o.tiles_rect = (uint32_t *)calloc(P, 4); o.tiles_touched = (uint32_t *)calloc(P, 4);
		o.eigen_len = reals((size_t)2 * P, 0); o.eigen_vec = reals((size_t)4 * P, 0);
		o.level_ranges = (int32_t *)calloc((size_t)2 * P, 4); o.fov_colors = reals((size_t)P * FOV_NUM * 3, (real)NAN);
		o.tile_levels = reals(T, 0); o.tile_gx = reals(T, 0); o.tile_gy = reals(T, 0); o.tile_min = reals(T, 0);
		o.tile_blend = (uint8_t *)calloc(T, 1); o.ranges = (uint32_t *)calloc((size_t)2 * T, 4);
		o.capacity = capacity;
		o.point_list = (uint32_t *)calloc(capacity > 0 ? capacity : 1, 4); o.keys = (uint64_t *)calloc(capacity > 0 ? capacity : 1, 8);
		o.color = reals((size_t)3 * H * W, 0); o.final_T = reals((size_t)H * W, 0); o.n_contrib = (uint32_t *)calloc((size_t)H * W, 4);
		o.gaussians_count = (int32_t *)calloc(P, 4); o.contributions = reals(P, 0);
		n = orc_forward(&in, &o);
		*nan_tiles = 0; *visible = 0;
		for (int t = 0; t < T; t++) *nan_tiles += o.tile_levels[t] != o.tile_levels[t];
		for (int i = 0; i < P; i++) *visible += o.radii[i] > 0;
		void *all[] = { o.depths, o.radii, o.means2D, o.cov3D, o.conic, o.rgb, o.clamped, o.tiles_rect, o.tiles_touched, o.eigen_len, o.eigen_vec,
			o.level_ranges, o.fov_colors, o.tile_levels, o.tile_gx, o.tile_gy, o.tile_min, o.tile_blend, o.ranges, o.point_list, o.keys, o.color,
			o.final_T, o.n_contrib, o.gaussians_count, o.contributions };
		for (size_t k = 0; k < sizeof all / sizeof all[0]; k++) free(all[k]);
		if (n <= capacity) break;
		capacity = n;
	}
	free(means); free(scales); free(rots); free(opac); free(shs); free(dcs); free(hl);
	return n;
}

int main(void)
{
	static const int frames[][2] = { { 16, 16 }, { 17, 15 }, { 1, 1 }, { 2, 2 }, { 3, 40 }, { 16, 16 }, { 200, 120 }, { 15, 1 }, { 8, 8 } };
	static const int variants[] = { ORC_RF, ORC_SMFR, ORC_MMFR };
	static const int counts[] = { 1, 64 };
	for (size_t v = 0; v < sizeof variants / sizeof variants[0]; v++)
		for (size_t c = 0; c < sizeof counts / sizeof counts[0]; c++)
			for (size_t f = 0; f < sizeof frames / sizeof frames[0]; f++)
			{
				int nan_tiles = 0, visible = 0;
				int64_t n = run(variants[v], counts[c], frames[f][0], frames[f][1], &nan_tiles, &visible);
				printf("variant %d P %d frame %dx%d: instances %lld, visible %d, tiles with a NaN level %d\n", variants[v], counts[c],
					frames[f][0], frames[f][1], (long long)n, visible, nan_tiles);
				fflush(stdout);
			}
	printf("sanitize_driver: done\n");
	return 0;
}
