/* Exact 3-nearest-neighbour mean squared distance (the contract of fr_knn_mean_dist2, include/fovraster.h), by k-d tree.
 * Test infrastructure: compiled by tests/knn_ref.py with gcc -O2 -fopenmp -ffp-contract=off.
 *
 *   knn_exact IN OUT     IN: int32 P, then P x 3 float32; OUT: P float32
 *
 * out[i] = ((b0 + b1) + b2) / 3.0f, b0 <= b1 <= b2 the three smallest d(i,j) = (dx*dx + dy*dy) + dz*dz over j != i,
 * dx = p_j.x - p_i.x, seeded with FLT_MAX. A node is skipped when the bound of its box, computed in the same order with
 * per-axis gap max(0, lo - q, q - hi), is >= b2: rounding is monotone, so the bound is <= the distance of every point in
 * the box, and a distance >= b2 cannot change the three values. Finite coordinates only. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#define LEAF 8

typedef struct { float lo[3], hi[3]; int begin, end, left, right; } Node;

static const float *g_pts;
static int *g_idx;
static Node *g_nodes;
static int g_nnodes;

static float coord(int k, int axis) { return g_pts[3 * (size_t)g_idx[k] + axis]; }

/* Hoare quickselect on g_idx[lo..hi] by coordinate `axis`: afterwards position k holds its order statistic
 * (balanced splits also when many coordinates are equal) */
static void select_k(int lo, int hi, int k, int axis)
{
	while (lo < hi)
	{
		const float pivot = coord((lo + hi) / 2, axis);
		int i = lo, j = hi;
		while (i <= j)
		{
			while (coord(i, axis) < pivot) i++;
			while (coord(j, axis) > pivot) j--;
			if (i <= j) { int t = g_idx[i]; g_idx[i] = g_idx[j]; g_idx[j] = t; i++; j--; }
		}
		if (k <= j) hi = j;
		else if (k >= i) lo = i;
		else break;
	}
}

static int build(int begin, int end)
{
	const int ni = g_nnodes++;
	Node *n = &g_nodes[ni];
	for (int a = 0; a < 3; a++) { n->lo[a] = FLT_MAX; n->hi[a] = -FLT_MAX; }
	for (int k = begin; k < end; k++)
		for (int a = 0; a < 3; a++)
		{
			const float c = coord(k, a);
			if (c < n->lo[a]) n->lo[a] = c;
			if (c > n->hi[a]) n->hi[a] = c;
		}
	n->begin = begin; n->end = end; n->left = n->right = -1;
	if (end - begin <= LEAF) return ni;
	int axis = 0;
	for (int a = 1; a < 3; a++) if (n->hi[a] - n->lo[a] > n->hi[axis] - n->lo[axis]) axis = a;
	const int mid = begin + (end - begin) / 2;
	select_k(begin, end - 1, mid, axis);
	const int l = build(begin, mid);
	const int r = build(mid, end);
	g_nodes[ni].left = l;
	g_nodes[ni].right = r;
	return ni;
}

static float gap(float lo, float hi, float q) { return fmaxf(0.0f, fmaxf(lo - q, q - hi)); }

static float bound(const Node *n, const float *q)
{
	const float gx = gap(n->lo[0], n->hi[0], q[0]), gy = gap(n->lo[1], n->hi[1], q[1]), gz = gap(n->lo[2], n->hi[2], q[2]);
	return (gx * gx + gy * gy) + gz * gz;
}

static void search(int ni, int self, const float *q, float *b)
{
	const Node *n = &g_nodes[ni];
	if (!(bound(n, q) < b[2])) return;
	if (n->left < 0)
	{
		for (int k = n->begin; k < n->end; k++)
		{
			const int j = g_idx[k];
			if (j == self) continue;
			const float *p = g_pts + 3 * (size_t)j;
			const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
			const float d = (dx * dx + dy * dy) + dz * dz;
			b[2] = fminf(b[2], fmaxf(b[1], d));
			b[1] = fminf(b[1], fmaxf(b[0], d));
			b[0] = fminf(b[0], d);
		}
		return;
	}
	const float bl = bound(&g_nodes[n->left], q), br = bound(&g_nodes[n->right], q);
	if (bl <= br) { search(n->left, self, q, b); search(n->right, self, q, b); }
	else { search(n->right, self, q, b); search(n->left, self, q, b); }
}

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	int32_t P = 0;
	if (!f || fread(&P, 4, 1, f) != 1 || P < 0) { fprintf(stderr, "bad input\n"); return 2; }
	float *pts = malloc((size_t)(P ? P : 1) * 12), *out = malloc((size_t)(P ? P : 1) * 4);
	g_idx = malloc((size_t)(P ? P : 1) * sizeof(int));
	g_nodes = malloc(((size_t)P / 2 + 16) * sizeof(Node)); /* leaves hold >= LEAF / 2 points */
	if (!pts || !out || !g_idx || !g_nodes) { fprintf(stderr, "out of memory\n"); return 2; }
	if (fread(pts, 12, (size_t)P, f) != (size_t)P) { fprintf(stderr, "short input\n"); return 2; }
	fclose(f);
	g_pts = pts;
	for (int i = 0; i < P; i++) g_idx[i] = i;
	if (P > 0) build(0, P);
#pragma omp parallel for schedule(dynamic, 1024)
	for (int i = 0; i < P; i++)
	{
		float b[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
		search(0, i, pts + 3 * (size_t)i, b);
		out[i] = ((b[0] + b[1]) + b[2]) / 3.0f;
	}
	f = fopen(argv[2], "wb");
	if (!f || fwrite(out, 4, (size_t)P, f) != (size_t)P) { fprintf(stderr, "cannot write output\n"); return 2; }
	fclose(f);
	return 0;
}
