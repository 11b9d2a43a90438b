/*
 * rb3gpu_kount.h -- k-mer counting over one or more indexes (`kount`, the reference's main_kount, main.c:333-423) as a
 * level-synchronous walk of the k-mer trie.
 *
 * The reference walks the trie depth first with one stack per index: a node is a string of d symbols with its interval
 * [lo, hi) in every index, its child for a = A C G T (1..4) prepends a: [C[a] + rank(a, lo), C[a] + rank(a, hi)).  A
 * child is kept if hi - lo >= m in ANY index (all children for m <= 0).  Here every node of one depth is expanded at
 * once: a FRONTIER holds the nodes of a depth in the order the reference visits them -- parents in order, each parent's
 * children T, G, C, A (the stack pops the last child pushed) -- and the last level is written in A, C, G, T order, as
 * the reference prints it.  No sort anywhere.
 *
 * A frontier node: the symbols chosen so far, 2 bits each (symbol a - 1 of depth t at bit 2 (t - 1) of the W-word
 * code), and (lo, hi) per index.  Per level: k_kount_expand (one octet per (node, index): two oct_rank_issue and
 * oct_rank_finish for a = 1..4 -- the merge's rank decode, all slot layouts and the beyond-2^32 modes included),
 * k_kount_keep (several indexes: the keep mask from the maximum count), an exclusive scan of the kept-children counts
 * (rocPRIM, rb3gpu_kount.hip) and k_kount_emit (the next frontier, or output records at the last level).  The number of
 * nodes of a frontier lives on the device (a count pointer) and bounds the grids from above, so a level needs no host
 * synchronisation unless its children might not fit the level cap (rb3gpu_kount in rb3gpu.hip slices it then).
 */
#ifndef RB3GPU_KOUNT_H
#define RB3GPU_KOUNT_H

#include "rb3gpu_kernels.h"

/* the four children of node q (bit a - 1 for symbol a): kept if some index counts at least m, all for m <= 0.
 * ci: (lo, hi) of the children per node, index and symbol: ci[((q * ni + i) * 4 + a - 1) * 2 + {0, 1}] */
__device__ __forceinline__ uint32_t kount_mask(const int64_t *ci, int64_t q, int ni, int64_t m)
{
	if (m <= 0) return 15u;
	uint32_t mask = 0;
	for (int i = 0; i < ni; ++i) {
		const int64_t *c = ci + (q * ni + i) * 8;
#pragma unroll
		for (int a = 0; a < 4; ++a)
			if (c[a * 2 + 1] - c[a * 2] >= m) mask |= 1u << a;
	}
	return mask;
}

/* the root: the string of no symbols, [0, n) in every index, and the frontier's count (1) */
__global__ void __launch_bounds__(64) k_kount_root(const IdxView *tab, int ni, int W, uint64_t *code, int64_t *iv, int64_t *pn)
{
	const int t = threadIdx.x;
	for (int i = t; i < ni; i += blockDim.x) iv[i * 2] = 0, iv[i * 2 + 1] = tab[i].n;
	for (int w = t; w < W; w += blockDim.x) code[w] = 0;
	if (t == 0) *pn = 1;
}

/* child intervals of the nodes [0, *pn) of a frontier, one octet per (node, index); nub >= *pn bounds the frontier from above.
 * cnt[q] = 0 for q in [*pn, nub] (the scan runs over nub + 1 entries); one index: cnt[q] = kept children, else k_kount_keep does that.
 * nodes += *pn (the nodes expanded, for the statistics) */
__global__ void __launch_bounds__(256) k_kount_expand(const IdxView *tab, int ni, const int64_t *pn, int64_t nub, const int64_t *iv, int64_t *ci,
		uint32_t *cnt, int64_t m, unsigned long long *nodes)
{
	const int lane = threadIdx.x & 63, j = lane & 7;
	int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
	const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 3, n = *pn, np = (nub + 1) * ni;
	if (p == 0 && j == 0) atomicAdd(nodes, (unsigned long long)n);
	for (; p < np; p += stride) {
		const int64_t q = p / ni;
		const int i = (int)(p - q * ni);
		if (q >= n) { if (i == 0 && j == 0) cnt[q] = 0; continue; }
		const int64_t lo = iv[p * 2], hi = iv[p * 2 + 1];
		int64_t *c = ci + p * 8;
		uint32_t mask = 0;
		if (lo >= hi) { // absent from this index: so are its children (their place in the BWT does not matter, only their count)
			if (j < 4) c[j * 2] = 0, c[j * 2 + 1] = 0;
		} else {
			const IdxView ix = tab[i];
			RankLoad rl, ru;
			oct_rank_issue(ix, lo, j, rl);
			oct_rank_issue(ix, hi, j, ru);
#pragma unroll
			for (int a = 1; a <= 4; ++a) {
				const int64_t x = oct_rank_finish(rl, a, j, ix.abs), y = oct_rank_finish(ru, a, j, ix.abs);
				if (j == a - 1) c[j * 2] = x, c[j * 2 + 1] = y;
				if (m <= 0 || y - x >= m) mask |= 1u << (a - 1);
			}
		}
		if (ni == 1 && j == 0) cnt[q] = __popc(m <= 0 ? 15u : mask);
	}
}

/* several indexes: the kept children of every node from the maximum count over the indexes */
__global__ void __launch_bounds__(256) k_kount_keep(const int64_t *ci, int ni, const int64_t *pn, int64_t nub, int64_t m, uint32_t *cnt)
{
	const int64_t n = *pn;
	for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= nub; q += (int64_t)gridDim.x * blockDim.x)
		cnt[q] = q < n ? __popc(kount_mask(ci, q, ni, m)) : 0u;
}

/* the parent q in [i0, j) of which the exclusive scan `off` holds the most children within lim: j (> i0: a parent has at most
 * 4 children and lim >= 4) and off[j] - off[i0] into sc[0], sc[1].  One thread. */
__global__ void k_kount_split(const int64_t *off, int64_t i0, int64_t n, int64_t lim, int64_t *sc)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	const int64_t base = off[i0];
	int64_t lo = i0 + 1, hi = n; // the answer lies in [lo, hi]
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo + 1) / 2;
		if (off[mid] - base <= lim) lo = mid;
		else hi = mid - 1;
	}
	sc[0] = lo, sc[1] = off[lo] - base;
}

/* the children of the parents [i0, j) (j = *pj if pj is given) of depth d: child r = off[q] - off[i0] + (its place among the kept
 * children of q).  leaf = 0: the frontier of depth d + 1 (code2, iv2), children T, G, C, A.  leaf = 1 (d = k - 1): output records in
 * A, C, G, T order, the k-mer as symbols 1..4 (kmers[r * k + p]; the symbol of depth t is character k - t, the last level's comes first) and the count per index */
__global__ void __launch_bounds__(256) k_kount_emit(const uint64_t *code, const int64_t *ci, const int64_t *off, int W, int ni, int d, int k, int64_t m,
		int64_t i0, int64_t j, const int64_t *pj, int leaf, uint64_t *code2, int64_t *iv2, uint8_t *kmers, int64_t *counts)
{
	if (pj) j = *pj;
	const int64_t base = off[i0];
	for (int64_t q = i0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < j; q += (int64_t)gridDim.x * blockDim.x) {
		const uint32_t mask = kount_mask(ci, q, ni, m);
		if (mask == 0) continue;
		int64_t r = off[q] - base;
		const uint64_t *pc = code + q * W;
		if (!leaf) {
			for (int a = 4; a >= 1; --a) {
				if (!(mask >> (a - 1) & 1u)) continue;
				uint64_t *cc = code2 + r * W;
				for (int w = 0; w < W; ++w) cc[w] = pc[w] | (w == (d >> 5) ? (uint64_t)(a - 1) << (2 * (d & 31)) : 0ull);
				for (int i = 0; i < ni; ++i) {
					const int64_t *c = ci + ((q * ni + i) * 4 + a - 1) * 2;
					iv2[(r * ni + i) * 2] = c[0], iv2[(r * ni + i) * 2 + 1] = c[1];
				}
				++r;
			}
		} else {
			for (int a = 1; a <= 4; ++a) {
				if (!(mask >> (a - 1) & 1u)) continue;
				uint8_t *s = kmers + r * k;
				s[0] = (uint8_t)a; // (the symbol of depth k)
				for (int p = 1; p < k; ++p) {
					const int t = k - 1 - p; // the symbol of depth k - p sits at code position k - p - 1
					s[p] = (uint8_t)((pc[t >> 5] >> (2 * (t & 31)) & 3u) + 1u);
				}
				for (int i = 0; i < ni; ++i) {
					const int64_t *c = ci + ((q * ni + i) * 4 + a - 1) * 2;
					counts[r * ni + i] = c[1] - c[0];
				}
				++r;
			}
		}
	}
}

#endif
