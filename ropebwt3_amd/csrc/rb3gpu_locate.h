/*
 * rb3gpu_locate.h -- where the rows of an interval lie in the indexed sequences (`mem -p`: rb3_ssa_multi, ssa.c:114-192 of the
 * reference), for a batch of intervals: up to min(P, hi - lo) pairs (sid, pos) per interval, the SAME pairs in the SAME order as
 * the reference.  The order is the reference's traversal and nothing else fixes it: with P < hi - lo it decides which occurrences
 * are reported.
 *
 *   split    an interval is cut at its sampled rows (rows r >= acc[1] with (r - acc[1]) % 2^ss == 0): a sampled row is answered at once
 *            from ssa[], the pieces between go onto a binary heap ordered by size (ssa_add_intv; the piece after the last sampled row is
 *            pushed even when it is empty, and so it is here: it takes a place in the heap and decides ties);
 *   pop      the largest piece leaves the heap (ks_heapdown of ksort.h after the last element moved to the top; ties fall as that
 *            heap leaves them), ONE pair of all-symbol ranks at its two ends: the rows whose symbol is the sentinel are answered from
 *            r2i[], the children for the symbols 1..5 are split and pushed with offset + 1;
 *   stop     the moment min(P, hi - lo) pairs are out, in the middle of a split or of the sentinel rows as well.
 *
 * One octet per interval, as in k_mem_walk: the rank pair (two oct_rank_issue, six oct_rank_finish each) runs converged over the eight
 * octets of a wave -- the decode moves data between lanes and must see all of them --, the heap is kept by lane 0 of the octet
 * between two ranks, and an octet that has finished takes the next interval from a counter.
 *
 * The heap of an octet is `cap` entries of LDS (tier 1).  An interval that needs more is flagged and given up; the flagged ones are
 * run again by the same kernel with heaps in global memory, sized by the host from a bound on what a heap can hold (tier 2;
 * DESIGN.md 7d has the bound).  Every interval knows its place in the output before the launch (an exclusive scan of min(P, size)),
 * so there are no atomics on the output and no sort; the traversal ends with exactly that many pairs or the call fails.
 */
#ifndef RB3GPU_LOCATE_H
#define RB3GPU_LOCATE_H

#include "rb3gpu_kernels.h"

struct LocEnt { int64_t lo, hi, off; };     // a piece on the heap (ssa_intv_t)
struct LocPair { int64_t sid, pos; };       // rb3gpu_pos_t

enum { LOC_CTR_NEXT = 0, LOC_CTR_POPS, LOC_CTR_MAXHEAP, LOC_CTR_OVF, LOC_CTR_ERR, LOC_CTR_WORDS = 8 };

/* the traversal of one interval as lane 0 of its octet sees it */
struct LocState {
	LocEnt *a;             // the heap: LDS (tier 1) or global memory (tier 2)
	int64_t cap, n_a;      // its room, its entries
	int64_t n_sa, max_sa;  // pairs written, pairs wanted
	LocPair *out;
	bool ovf, bad;
	int64_t top;           // most entries the heap held
};

/* the interval source: lo = src[i * stride], then its end (is_size == 0) or its size.  iv[2i], iv[2i + 1] = lo, hi; cnt[i] = min(P, hi - lo); cnt[n] = 0 */
__global__ void __launch_bounds__(256) k_locate_prep(const int64_t *src, int stride, int is_size, int64_t n, int64_t max_pos, int64_t *iv, uint32_t *cnt)
{
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) {
		if (i == n) { cnt[i] = 0; continue; }
		const int64_t lo = src[i * stride], x = src[i * stride + 1], hi = is_size ? lo + x : x;
		const int64_t sz = hi > lo ? hi - lo : 0;
		iv[2 * i] = lo, iv[2 * i + 1] = hi;
		cnt[i] = (uint32_t)(sz < max_pos ? sz : max_pos);
	}
}

/* ssa_add_intv1 with ks_heapup: the new piece rises past every parent that is not larger */
__device__ __forceinline__ void loc_push(LocState &s, int64_t lo, int64_t hi, int64_t off)
{
	if (s.n_a >= s.cap) { s.ovf = true; return; }
	int64_t k = s.n_a++;
	const int64_t sz = hi - lo;
	while (k) {
		const int64_t i = (k - 1) >> 1;
		const LocEnt p = s.a[i];
		if (sz < p.hi - p.lo) break;
		s.a[k] = p, k = i;
	}
	LocEnt e;
	e.lo = lo, e.hi = hi, e.off = off;
	s.a[k] = e;
	if (s.n_a > s.top) s.top = s.n_a;
}

/* the top of the heap; the last element takes its place and sinks (ks_heapdown from 0) */
__device__ __forceinline__ LocEnt loc_pop(LocState &s)
{
	const LocEnt x = s.a[0];
	const int64_t n = --s.n_a;
	if (n > 0) {
		const LocEnt t = s.a[n];
		const int64_t ts = t.hi - t.lo;
		int64_t i = 0, k = 0;
		while ((k = (k << 1) + 1) < n) {
			LocEnt c = s.a[k];
			if (k != n - 1) {
				const LocEnt d = s.a[k + 1];
				if (c.hi - c.lo < d.hi - d.lo) c = d, ++k;
			}
			if (c.hi - c.lo < ts) break;
			s.a[i] = c, i = k;
		}
		s.a[i] = t;
	}
	return x;
}

/* ssa_add_intv: the sampled rows of [lo, hi) answered, the pieces between them pushed */
__device__ __forceinline__ void loc_add(LocState &s, const uint64_t *ssa, int64_t n_ssa, int64_t m, int ss, int ms, int64_t lo, int64_t hi, int64_t off)
{
	if (s.n_sa == s.max_sa || s.ovf) return;
	const uint64_t mask = ((uint64_t)1 << ms) - 1;
	for (int64_t k = (((lo - m) >> ss) << ss) + m; k < hi; k += (int64_t)1 << ss) {
		if (k < lo) continue;
		const int64_t l = (k - m) >> ss;
		if (l < 0 || l >= n_ssa) { s.bad = true; return; }
		const uint64_t v = ssa[l];
		LocPair p;
		p.sid = (int64_t)(v & mask), p.pos = off + (int64_t)(v >> ms);
		s.out[s.n_sa++] = p;
		if (s.n_sa == s.max_sa) return;
		if (lo < k) loc_push(s, lo, k, off);
		if (s.ovf) return;
		lo = k + 1;
	}
	loc_push(s, lo, hi, off);
}

/* The intervals idx[t] (idx == NULL: t itself) for t in [0, n): iv their bounds, cnt their pair counts, ooff their places in `out`
 * less obase.  hoff == NULL: tier 1, a heap of `cap` entries of dynamic LDS per octet, an interval that overflows it gets flag[i] = 1;
 * else tier 2, interval t owns gheap[hoff[t], hoff[t + 1]) and an overflow is an error.  ctr: LOC_CTR_* (NEXT zero at launch) */
__global__ void __launch_bounds__(256) k_locate(IdxView ix, Acc7 acc, int ss, int ms, const uint64_t *ssa, int64_t n_ssa, const uint64_t *r2i, int64_t n, const int64_t *idx,
		const int64_t *iv, const uint32_t *cnt, const int64_t *ooff, int64_t obase, LocPair *out, int64_t cap, const int64_t *hoff, LocEnt *gheap, uint32_t *flag, unsigned long long *ctr)
{
	extern __shared__ LocEnt loc_lds[];
	const int j = threadIdx.x & 7;
	const int64_t m = acc.a[1];
	LocState s;
	s.a = nullptr, s.cap = s.n_a = s.n_sa = s.max_sa = 0, s.out = nullptr, s.ovf = s.bad = false, s.top = 0;
	bool have = false, done = false;
	int64_t cur = 0, xoff = 0;
	unsigned long long pops = 0, n_ovf = 0, n_err = 0;
	for (;;) {
		int64_t plo = 0, phi = 0;
		uint32_t act = 0;
		if (j == 0) { // everything between two rank pairs
			while (!done) {
				if (!have) {
					const unsigned long long t = atomicAdd(ctr + LOC_CTR_NEXT, 1ull);
					if ((int64_t)t >= n) { done = true; break; }
					cur = idx ? idx[t] : (int64_t)t;
					if (hoff) s.a = gheap + hoff[t], s.cap = hoff[t + 1] - hoff[t];
					else s.a = loc_lds + (int64_t)(threadIdx.x >> 3) * cap, s.cap = cap;
					s.n_a = s.n_sa = 0, s.max_sa = cnt[cur], s.out = out + (ooff[cur] - obase), s.ovf = s.bad = false;
					have = true;
					if (s.max_sa > 0) loc_add(s, ssa, n_ssa, m, ss, ms, iv[2 * cur], iv[2 * cur + 1], 0);
				}
				if (s.bad) { ++n_err, have = false; continue; }
				if (s.ovf) { // not with this heap
					if (hoff) ++n_err;
					else flag[cur] = 1u, ++n_ovf;
					have = false;
					continue;
				}
				if (s.n_a > 0 && s.n_sa < s.max_sa) {
					const LocEnt x = loc_pop(s);
					plo = x.lo, phi = x.hi, xoff = x.off, act = 1;
					break;
				}
				if (s.n_sa != s.max_sa) ++n_err; // (the children of a rank pair add up to the piece: cannot happen on a sound index)
				have = false;
			}
		}
		act = oct_bcast0(act, j);
		if (__ballot(act != 0u) == 0ull) break;
		{
			const uint32_t a0 = oct_bcast0((uint32_t)plo, j), a1 = oct_bcast0((uint32_t)((uint64_t)plo >> 32), j);
			const uint32_t b0 = oct_bcast0((uint32_t)phi, j), b1 = oct_bcast0((uint32_t)((uint64_t)phi >> 32), j);
			plo = (int64_t)((uint64_t)a1 << 32 | a0), phi = (int64_t)((uint64_t)b1 << 32 | b0);
		}
		RankLoad rl, ru;
		oct_rank_issue(ix, act ? plo : 0, j, rl); // (an idle octet: a valid address, the result unused)
		oct_rank_issue(ix, act ? phi : 0, j, ru);
		int64_t ok[6], ol[6];
#pragma unroll
		for (int c = 0; c < 6; ++c) ok[c] = oct_rank_finish(rl, c, j, ix.abs), ol[c] = oct_rank_finish(ru, c, j, ix.abs); // (acc[c] + rank: the child's rows)
		if (j == 0 && act) {
			++pops;
			for (int64_t l = ok[0]; l < ol[0] && s.n_sa < s.max_sa; ++l) { // rows that reach a sentinel: the string starts here
				if (l < 0 || l >= m) { s.bad = true; break; }
				LocPair p;
				p.sid = (int64_t)r2i[l], p.pos = xoff;
				s.out[s.n_sa++] = p;
			}
#pragma unroll
			for (int c = 1; c < 6; ++c)
				if (ok[c] < ol[c]) loc_add(s, ssa, n_ssa, m, ss, ms, ok[c], ol[c], xoff + 1);
		}
	}
	if (j == 0) {
		if (pops) atomicAdd(ctr + LOC_CTR_POPS, pops);
		if (s.top) atomicMax(ctr + LOC_CTR_MAXHEAP, (unsigned long long)s.top);
		if (n_ovf) atomicAdd(ctr + LOC_CTR_OVF, n_ovf);
		if (n_err) atomicAdd(ctr + LOC_CTR_ERR, n_err);
	}
}

#endif
