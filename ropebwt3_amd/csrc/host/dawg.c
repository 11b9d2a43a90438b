/*
 * dawg.c -- the directed acyclic word graph of a query, the rows of `sw --local` (rb3_bwtl_gen and rb3_dawg_gen of the reference, dawg.c:28-76
 * and 115-228, restated by behaviour).
 *
 * A node is an interval [lo, hi) of the query's own suffix array that a backward search from the whole array [0, len + 1) can reach; an
 * edge W -> cW is one backward extension.  The query is indexed with every symbol above 4 counted as A (dawg.c:44-45), so a node reached
 * over an N carries symbol 1: N against an indexed A then scores a match.  The suffix array comes from the SA-IS of sais.c (row 0 is the
 * sentinel's, sa[0] = len); a rank is a count over rows, and the `$` row holds none of the four symbols, which is what skipping it amounts to.
 *
 * What nothing but the reference's traversal gives is the NUMBER of a node, and the numbers decide the order in which candidates meet:
 *   1. in-degrees: from the root, pop an interval, visit its children c = 3..0, push a child the first time it is seen;
 *   2. numbers: the same walk, but a child is pushed -- and gets the next number -- the moment its LAST incoming edge is seen.  The
 *      predecessor lists are laid out in that order, in-degree many places each (an in-degree is not bounded by 4);
 *   3. predecessors: nodes by ascending number, children c = 0..3, each child gets the node appended to its list.
 * Per node on the host: qoff0 = sa[lo], where the node's string starts in the query (the first of its n_qoff = hi - lo places).
 */
#include <stdlib.h>
#include <string.h>
#include "rb3host.h"

int rb3h_sais_i32(const int32_t *T, int32_t *SA, int32_t n, int32_t K); /* sais.c */

typedef struct { uint64_t key; int32_t deg, cnt, id; } dg_ent_t;

static inline uint64_t dg_hash(uint64_t x)
{
	x ^= x >> 33, x *= 0xff51afd7ed558ccdULL;
	x ^= x >> 33, x *= 0xc4ceb9fe1a85ec53ULL;
	return x ^ x >> 33;
}

static inline dg_ent_t *dg_find(dg_ent_t *h, uint64_t mask, uint64_t key) /* the entry of key, or the empty one where it belongs (no key is 0) */
{
	uint64_t i = dg_hash(key) & mask;
	while (h[i].key != 0 && h[i].key != key) i = (i + 1) & mask;
	return h + i;
}

void rb3h_dawg_free(rb3h_dawg_t *g)
{
	if (g == 0) return;
	free(g->sym); free(g->pre_off); free(g->pre); free(g->qoff0); free(g->n_qoff);
	memset(g, 0, sizeof(*g));
}

int rb3h_dawg_build(int64_t len, const uint8_t *seq, rb3h_dawg_t *g)
{
	const int64_t n = len + 1; /* rows of the suffix array */
	int32_t *T = 0, *sa = 0, (*occ)[4] = 0, *nlo = 0, *nhi = 0, *fill = 0, acc[4], cnt[4] = { 0, 0, 0, 0 };
	uint64_t *stack = 0, mask, cap;
	dg_ent_t *h = 0, *e;
	int64_t i, n_stack, n_node = 0, n_pre = 0, m_node;
	int32_t id = 0;
	int ret = -1, c;
	memset(g, 0, sizeof(*g));
	if (len < 0 || len > 0x3ffffff0LL) return -3;
	m_node = 2 * n + 2; /* (a suffix automaton has at most 2 len - 1 states; its classes are these intervals) */
	for (cap = 16; cap < (uint64_t)m_node * 2; cap <<= 1) {}
	mask = cap - 1;
	T = (int32_t*)malloc((size_t)n * 4), sa = (int32_t*)malloc((size_t)n * 4);
	occ = (int32_t(*)[4])malloc((size_t)(n + 1) * 16);
	h = (dg_ent_t*)calloc((size_t)cap, sizeof(dg_ent_t));
	stack = (uint64_t*)malloc((size_t)m_node * 8);
	nlo = (int32_t*)malloc((size_t)m_node * 4), nhi = (int32_t*)malloc((size_t)m_node * 4);
	if (!T || !sa || !occ || !h || !stack || !nlo || !nhi) goto end;
	for (i = 0; i < len; ++i) T[i] = seq[i] >= 5 || seq[i] == 0 ? 1 : seq[i];
	T[len] = 0;
	if (rb3h_sais_i32(T, sa, (int32_t)n, 5) < 0) goto end;
	for (i = 0; i < n; ++i) { /* occ[k][c]: rows [0, k) whose symbol -- the one before the row's suffix -- is c + 1 */
		memcpy(occ[i], cnt, 16);
		if (sa[i] > 0) ++cnt[T[sa[i] - 1] - 1];
	}
	memcpy(occ[n], cnt, 16);
	acc[0] = 1;
	for (c = 1; c < 4; ++c) acc[c] = acc[c - 1] + cnt[c - 1];

#define DG_KEY(lo, hi) ((uint64_t)(uint32_t)(lo) << 32 | (uint32_t)(hi))
	/* 1. in-degrees */
	e = dg_find(h, mask, DG_KEY(0, n)), e->key = DG_KEY(0, n), n_node = 1;
	stack[0] = DG_KEY(0, n), n_stack = 1;
	while (n_stack > 0) {
		const uint64_t x = stack[--n_stack];
		const int32_t lo = (int32_t)(x >> 32), hi = (int32_t)x;
		for (c = 3; c >= 0; --c) {
			const int32_t l = acc[c] + occ[lo][c], u = acc[c] + occ[hi][c];
			if (l == u) continue;
			e = dg_find(h, mask, DG_KEY(l, u));
			if (e->key == 0) {
				if (n_node >= m_node) goto end; /* (cannot happen) */
				e->key = DG_KEY(l, u), stack[n_stack++] = e->key, ++n_node;
			}
			++e->deg, ++n_pre;
		}
	}
	g->sym = (uint8_t*)calloc((size_t)n_node, 1);
	g->pre_off = (int64_t*)calloc((size_t)n_node + 1, 8);
	g->pre = (int32_t*)malloc((size_t)(n_pre > 0 ? n_pre : 1) * 4);
	g->qoff0 = (int32_t*)malloc((size_t)n_node * 4), g->n_qoff = (int32_t*)malloc((size_t)n_node * 4);
	fill = (int32_t*)calloc((size_t)n_node, 4);
	if (!g->sym || !g->pre_off || !g->pre || !g->qoff0 || !g->n_qoff || !fill) goto end;
	/* 2. numbers */
	nlo[0] = 0, nhi[0] = (int32_t)n, id = 1;
	stack[0] = DG_KEY(0, n), n_stack = 1;
	while (n_stack > 0) {
		const uint64_t x = stack[--n_stack];
		const int32_t lo = (int32_t)(x >> 32), hi = (int32_t)x;
		for (c = 3; c >= 0; --c) {
			const int32_t l = acc[c] + occ[lo][c], u = acc[c] + occ[hi][c];
			if (l == u) continue;
			e = dg_find(h, mask, DG_KEY(l, u));
			if (e->key == 0 || id > n_node) goto end;
			if (++e->cnt == e->deg) {
				if (id >= n_node) goto end;
				e->id = id, nlo[id] = l, nhi[id] = u, g->sym[id] = (uint8_t)(c + 1);
				g->pre_off[id + 1] = g->pre_off[id] + e->deg;
				stack[n_stack++] = e->key, ++id;
			}
		}
	}
	if (id != n_node || g->pre_off[n_node] != n_pre) goto end;
	/* 3. predecessors */
	for (i = 0; i < n_node; ++i) {
		for (c = 0; c < 4; ++c) {
			const int32_t l = acc[c] + occ[nlo[i]][c], u = acc[c] + occ[nhi[i]][c];
			if (l == u) continue;
			e = dg_find(h, mask, DG_KEY(l, u));
			if (e->key == 0 || fill[e->id] >= e->deg) goto end;
			g->pre[g->pre_off[e->id] + fill[e->id]++] = (int32_t)i;
		}
		g->qoff0[i] = sa[nlo[i]], g->n_qoff[i] = nhi[i] - nlo[i];
	}
#undef DG_KEY
	g->n_node = n_node, g->n_pre = n_pre;
	ret = 0;
end:
	free(T); free(sa); free(occ); free(h); free(stack); free(nlo); free(nhi); free(fill);
	if (ret < 0) rb3h_dawg_free(g);
	return ret;
}

/* the graphs of a batch, one after another: query q owns the nodes [node_off[q], node_off[q + 1]); pre_off[] runs over all nodes of the batch
 * (one more entry than nodes) and names places of pre[], whose entries are node numbers WITHIN the query */
int rb3h_dawg_batch(int64_t n_query, const int64_t *offsets, const uint8_t *symbols, rb3h_dawg_t *out, int64_t *node_off)
{
	rb3h_dawg_t *g;
	int64_t q, tn = 0, tp = 0;
	int err = 0;
	memset(out, 0, sizeof(*out));
	if (n_query < 0) return -3;
	g = (rb3h_dawg_t*)calloc((size_t)(n_query > 0 ? n_query : 1), sizeof(*g));
	if (g == 0) return -1;
#pragma omp parallel for schedule(dynamic, 16)
	for (q = 0; q < n_query; ++q) {
		const int r = rb3h_dawg_build(offsets[q + 1] - offsets[q], symbols + offsets[q], &g[q]);
		if (r < 0) {
#pragma omp critical
			err = r;
		}
	}
	node_off[0] = 0;
	for (q = 0; q < n_query && !err; ++q) tn += g[q].n_node, tp += g[q].n_pre, node_off[q + 1] = tn;
	if (!err) {
		out->sym = (uint8_t*)malloc((size_t)tn + 1), out->pre_off = (int64_t*)malloc((size_t)(tn + 1) * 8), out->pre = (int32_t*)malloc((size_t)(tp + 1) * 4);
		out->qoff0 = (int32_t*)malloc((size_t)(tn + 1) * 4), out->n_qoff = (int32_t*)malloc((size_t)(tn + 1) * 4);
		if (!out->sym || !out->pre_off || !out->pre || !out->qoff0 || !out->n_qoff) err = -1;
	}
	if (!err) {
		int64_t an = 0, ap = 0, i;
		for (q = 0; q < n_query; ++q) {
			const rb3h_dawg_t *x = g + q;
			memcpy(out->sym + an, x->sym, (size_t)x->n_node);
			memcpy(out->qoff0 + an, x->qoff0, (size_t)x->n_node * 4);
			memcpy(out->n_qoff + an, x->n_qoff, (size_t)x->n_node * 4);
			if (x->n_pre > 0) memcpy(out->pre + ap, x->pre, (size_t)x->n_pre * 4);
			for (i = 0; i < x->n_node; ++i) out->pre_off[an + i] = ap + x->pre_off[i];
			an += x->n_node, ap += x->n_pre;
		}
		out->pre_off[an] = ap, out->n_node = an, out->n_pre = ap;
	}
	for (q = 0; q < n_query; ++q) rb3h_dawg_free(g + q);
	free(g);
	if (err) rb3h_dawg_free(out);
	return err;
}
