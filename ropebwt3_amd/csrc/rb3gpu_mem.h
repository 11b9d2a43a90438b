/*
 * rb3gpu_mem.h -- super-maximal exact matches of queries (`mem`, the reference's default algorithm rb3_fmd_smem_TG,
 * fm-index.c:483-528, on the bidirectional extension rb3_fmd_extend, fm-index.c:384-400).
 *
 * A match is a bidirectional interval (x0, x1, size): x0 the first row of the match, x1 the first row of its reverse
 * complement.  Extending it by one symbol on either side is ONE pair of all-symbol ranks at lo and lo + size of the side
 * being extended (two oct_rank_issue, oct_rank_finish of the six symbols) and a few additions.
 *
 * One WALKER per chunk [a, b) of a query, an octet per walker.  A walker runs the reference's loop from x = a on the WHOLE
 * query and stops when its next start is >= b:
 *   phase 1  backward from x + min_len - 1 down to x; below min_occ at i: restart at x = i + 1;
 *   phase 2  forward from x + min_len to the first j that fails: the match (x, j);
 *   phase 3  backward from j down to x + 1: the first i that fails gives the next start i + 1.
 * The first match of a walker with a > 0 that starts AT a may be the tail of a match that starts further left: one more backward
 * extension by q[a - 1] decides, and the match is dropped if it stays at min_occ or above (the chunk to the left reports the whole of
 * it; DESIGN.md 7d has the argument).  Every other match of the walker is a match of the whole query.
 *
 * A match that starts at query position st is written to raw[global position of st - the slice's first position] and flagged there: a
 * query position starts at most one match, the chunks tile the symbols of the call, so the flagged entries in buffer order ARE the
 * reference's output order -- an exclusive scan of the flags and k_mem_gather compact them; no sort, no per-walker counts.
 * An octet that has finished its walker takes the next one from a counter, so the lanes of a wave stay busy whatever the walkers' lengths.
 */
#ifndef RB3GPU_MEM_H
#define RB3GPU_MEM_H

#include "rb3gpu_kernels.h"

struct MemRaw { int64_t x0, size; int32_t st, en; };                  // a match where it starts (24 bytes)
struct MemOut { int64_t query, x0, size; int32_t st, en; };           // rb3gpu_mem_rec_t

enum { MEM_IDLE = 0, MEM_START, MEM_ENTER2, MEM_FIN, MEM_EMIT, MEM_AFTER, /* no rank needed */
       MEM_P1, MEM_P2, MEM_P3, MEM_CHK, /* one extension each */ MEM_DONE };

__device__ __forceinline__ int mem_comp(int c) { return c >= 1 && c <= 4 ? 5 - c : c; }

/* acc[c] without indexing the kernel argument by a register */
__device__ __forceinline__ int64_t mem_acc(const Acc7 &acc, int c)
{
	int64_t v = acc.a[0];
#pragma unroll
	for (int a = 1; a < 7; ++a) v = c == a ? acc.a[a] : v;
	return v;
}

/* the place of symbol a in the order the other side's intervals are laid out in: $ T G C A N (fm-index.c:394-399) */
__device__ __forceinline__ int mem_ord(int a) { return a == 0 ? 0 : a == 5 ? 5 : 5 - a; }

/* the walkers [w0, w1) of a slice: walker w is chunk [wa[w], wa[w] + chunk) of query wq[w].  s0: the global position (qoff[query] + st) of the
 * slice's first symbol, cap: entries of raw / flag.  ctr[0]: the next walker to hand out (0 at launch), ctr[1] += extension steps */
__global__ void __launch_bounds__(256) k_mem_walk(IdxView ix, Acc7 acc, const uint8_t *sym, const int64_t *qoff, const int32_t *wq, const int32_t *wa,
		int64_t w0, int64_t w1, int64_t chunk, int64_t min_len, int64_t min_occ, int64_t s0, int64_t cap, MemRaw *raw, uint32_t *flag, unsigned long long *ctr)
{
	const int j = threadIdx.x & 7;
	int phase = MEM_IDLE;
	int64_t qb = 0, len = 0, a = 0, b = 0, x = 0, pos = 0, x0 = 0, x1 = 0, size = 0;
	unsigned long long steps = 0;
	for (;;) {
		while (phase <= MEM_AFTER) { // everything between two extensions (the same in the eight lanes of an octet)
			if (phase == MEM_IDLE) {
				unsigned long long t = 0;
				if (j == 0) t = atomicAdd(ctr, 1ull);
				const uint32_t tl = oct_bcast0((uint32_t)t, j), th = oct_bcast0((uint32_t)(t >> 32), j);
				const int64_t w = w0 + (int64_t)((unsigned long long)th << 32 | tl);
				if (w >= w1) { phase = MEM_DONE; break; }
				const int64_t q = wq[w];
				qb = qoff[q], len = qoff[q + 1] - qb, a = wa[w];
				b = a + chunk < len ? a + chunk : len; // (chunk <= 2^31 - 1: no overflow)
				x = a, phase = MEM_START;
			} else if (phase == MEM_START) { // rb3_fmd_smem1_TG from x
				if (x >= b || len - x < min_len) { phase = MEM_IDLE; continue; }
				const int c = min((int)sym[qb + x + min_len - 1], 5);
				x0 = mem_acc(acc, c), size = mem_acc(acc, c + 1) - x0, x1 = mem_acc(acc, mem_comp(c));
				pos = x + min_len - 2;
				phase = pos >= x ? MEM_P1 : MEM_ENTER2;
			} else if (phase == MEM_ENTER2) {
				pos = x + min_len;
				phase = pos < len ? MEM_P2 : MEM_FIN;
			} else if (phase == MEM_FIN) { // the match (x, pos)
				phase = x == a && a > 0 ? MEM_CHK : MEM_EMIT;
			} else if (phase == MEM_EMIT) {
				const int64_t g = qb + x - s0;
				if (j == 0 && g >= 0 && g < cap) {
					MemRaw r;
					r.x0 = x0, r.size = size, r.st = (int32_t)x, r.en = (int32_t)pos;
					raw[g] = r, flag[g] = 1u;
				}
				phase = MEM_AFTER;
			} else { // MEM_AFTER: the next start from the symbol that ended the match
				if (pos >= len) { phase = MEM_IDLE; continue; }
				const int c = min((int)sym[qb + pos], 5);
				x0 = mem_acc(acc, c), size = mem_acc(acc, c + 1) - x0, x1 = mem_acc(acc, mem_comp(c));
				--pos; // (pos = j - 1)
				if (pos > x) phase = MEM_P3;
				else x = pos + 1, phase = MEM_START;
			}
		}
		if (__ballot(phase != MEM_DONE) == 0ull) break;
		// one extension: backward by q[pos] (phases 1 and 3; the left check: q[a - 1]), forward by the complement of q[pos] (phase 2)
		const bool act = phase != MEM_DONE, back = phase != MEM_P2;
		int c = 0;
		if (act) {
			c = min((int)sym[qb + (phase == MEM_CHK ? a - 1 : pos)], 5);
			if (!back) c = mem_comp(c);
		}
		const int64_t p = back ? x0 : x1, o = back ? x1 : x0;
		RankLoad rl, ru;
		oct_rank_issue(ix, act ? p : 0, j, rl); // (a finished octet: a valid address, the result unused)
		oct_rank_issue(ix, act ? p + size : 0, j, ru);
		int64_t np = 0, ns = 0, cum = 0;
		const int oc = mem_ord(c);
#pragma unroll
		for (int s = 0; s < 6; ++s) {
			const int64_t lo = oct_rank_finish(rl, s, j, ix.abs), hi = oct_rank_finish(ru, s, j, ix.abs);
			if (s == c) np = lo, ns = hi - lo;
			if (mem_ord(s) < oc) cum += hi - lo;
		}
		if (act) {
			++steps;
			const bool ok = ns >= min_occ;
			if (ok && phase != MEM_CHK) {
				if (back) x0 = np, x1 = o + cum;
				else x1 = np, x0 = o + cum;
				size = ns;
			}
			if (phase == MEM_P1) {
				if (!ok) x = pos + 1, phase = MEM_START;
				else if (--pos < x) phase = MEM_ENTER2;
			} else if (phase == MEM_P2) {
				if (!ok || ++pos == len) phase = MEM_FIN;
			} else if (phase == MEM_P3) {
				if (!ok) x = pos + 1, phase = MEM_START;
				else if (--pos <= x) x = pos + 1, phase = MEM_START;
			} else phase = ok ? MEM_AFTER : MEM_EMIT; // MEM_CHK: extendable to the left: not a match of the whole query
		}
	}
	if (j == 0 && steps) atomicAdd(ctr + 1, steps);
}

/* the flagged entries of raw[0, ns) in order, with their query: out[off[g]] for flag[g] != 0 (off: the exclusive scan of flag).
 * The query of global position s0 + g: the last q of [0, nq) with qoff[q] <= s0 + g (queries of no symbols own no position) */
__global__ void __launch_bounds__(256) k_mem_gather(const MemRaw *raw, const uint32_t *flag, const int64_t *off, int64_t ns, int64_t s0, const int64_t *qoff, int64_t nq, MemOut *out)
{
	for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ns; g += (int64_t)gridDim.x * blockDim.x) {
		if (!flag[g]) continue;
		const int64_t at = s0 + g;
		int64_t lo = 0, hi = nq - 1; // the answer lies in [lo, hi]
		while (lo < hi) {
			const int64_t mid = lo + (hi - lo + 1) / 2;
			if (qoff[mid] <= at) lo = mid;
			else hi = mid - 1;
		}
		const MemRaw r = raw[g];
		MemOut t;
		t.query = lo, t.x0 = r.x0, t.size = r.size, t.st = r.st, t.en = r.en;
		out[off[g]] = t;
	}
}

#endif
