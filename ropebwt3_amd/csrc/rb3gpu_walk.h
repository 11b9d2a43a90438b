/*
 * rb3gpu_walk.h -- the plain walks over the index: `suffix`, the longest suffix of a query that occurs in the index
 * (main_suffix, main.c:167-217 of the reference, on the one-sided backward extension rb3_fmi_extend1, fm-index.h:140-147),
 * `get`, the i-th indexed string spelled out (rb3_fmi_retrieve, fm-index.c:552-567), as one chain per string or in pieces, and the seed test of `sw -j`: does
 * any stretch of min_len symbols of the query occur in the index (rb3_fmd_smem_present, fm-index.c:483-498 and 530-538).
 *
 * All are dependent chains of ranks: a step cannot start before the step in front of it has ended, so one chain runs at the
 * latency of a rank and the throughput comes from the chains in flight.  An octet of lanes per chain, as everywhere in the
 * engine; an octet that has finished its chain takes the next one from a counter, so the lanes of a wave stay busy whatever
 * the chains' lengths (k_mem_walk, k_ssa_walk).
 *
 *   k_suffix_walk  a step is ONE pair of ranks of ONE symbol, at the two ends of the interval: two oct_rank_issue and two
 *                  oct_rank_finish of the query's symbol -- a third of the decode of a step of k_mem_walk, which needs the
 *                  six symbols of both ends for the other strand's interval.
 *   k_get_walk     a step is oct_lf_self: the symbol at the row and its rank there.  Two modes of one template: COUNT
 *                  notes the length of the walk and the row it met the sentinel at, EMIT walks again and stores symbol t of
 *                  the walk at off + len - 1 - t, so the string lands in text order.  Between them lies an exclusive scan
 *                  of the lengths of a slice of rows (the driver).
 *   k_piece_walk   `get` in pieces: the step of k_get_walk, but a walker goes from a splitter's row (those of k_ssa_walk) to the next one only.
 *                  COUNT walks every piece of the index and the rows asked for down to their first splitter; k_ssa_jump joins the pieces, a sort
 *                  orders them by string and distance (k_piece_key, k_piece_inverse, k_piece_resolve), and EMIT walks the pieces of a slice of rows
 *                  again, all side by side, storing the symbol read at distance d from the start of the string at off + d - 2.
 *   k_seed_walk    the step of k_suffix_walk, in windows of min_len symbols: a window is walked from its last symbol to its
 *                  first; where the interval empties at symbol i, the next window starts at i + 1 (no window that holds
 *                  q[i .. x + min_len - 1] can occur), and a window that reaches its first symbol is a seed.  A query is cut
 *                  into walkers of `chunk` window starts each; the answer is the OR of the walkers' answers.
 */
#ifndef RB3GPU_WALK_H
#define RB3GPU_WALK_H

#include "rb3gpu_kernels.h"

struct SuffixOut { int64_t start, size; };                            // rb3gpu_suffix_rec_t

/* the next item of [0, n) from the counter, the same in the eight lanes of an octet */
__device__ __forceinline__ int64_t walk_take(unsigned long long *ctr, int j)
{
	unsigned long long t = 0;
	if (j == 0) t = atomicAdd(ctr, 1ull);
	const uint32_t tl = oct_bcast0((uint32_t)t, j), th = oct_bcast0((uint32_t)(t >> 32), j);
	return (int64_t)((unsigned long long)th << 32 | tl);
}

/* the queries [q0, q1): query q is sym[qoff[q], qoff[q + 1]) (fewer than 2^31 symbols: the driver refuses longer ones), its record out[q - q0].
 * ctr[0]: the next query to hand out (0 at launch), ctr[1] += extension steps */
__global__ void __launch_bounds__(256) k_suffix_walk(IdxView ix, Acc7 acc, const uint8_t *sym, const int64_t *qoff, int64_t q0, int64_t q1, SuffixOut *out, unsigned long long *ctr)
{
	const int j = threadIdx.x & 7;
	bool act = false, done = false;
	int64_t q = 0, qb = 0, k = 0, l = 0, last = 0;
	int32_t i = -1;
	unsigned long long steps = 0;
	for (;;) {
		while (!act && !done) { // (the same in the eight lanes of an octet)
			q = q0 + walk_take(ctr, j);
			if (q >= q1) { done = true; break; }
			qb = qoff[q];
			i = (int32_t)(qoff[q + 1] - qb) - 1;
			k = 0, l = acc.a[6], last = 0;
			if (i >= 0) act = true;
			else if (j == 0) { SuffixOut r; r.start = 0, r.size = 0; out[q - q0] = r; } // a query of no symbols
		}
		if (__ballot(act) == 0ull) break;
		// one extension by q[i]: the ranks of that symbol at both ends (main.c:199-206)
		const int c = act ? min((int)sym[qb + i], 5) : 0;
		RankLoad rl, ru;
		oct_rank_issue(ix, act ? k : 0, j, rl); // (a finished octet: a valid address, the result unused)
		oct_rank_issue(ix, act ? l : 0, j, ru);
		const int64_t nk = oct_rank_finish(rl, c, j, ix.abs), nl = oct_rank_finish(ru, c, j, ix.abs);
		if (act) {
			++steps;
			k = nk, l = nl;
			const bool hit = l - k != 0;
			if (hit) last = l - k, --i;
			if (!hit || i < 0) { // the symbol at i does not extend the match, or the query ran out
				if (j == 0) { SuffixOut r; r.start = (int64_t)i + 1, r.size = last; out[q - q0] = r; }
				act = false;
			}
		}
	}
	if (j == 0 && steps) atomicAdd(ctr + 1, steps);
}

/* the rows rows[r0, r1) (each inside [0, ix.n): the driver keeps the others away; one that is not is answered like them, never walked).
 * COUNT (EMIT = false): len[r] = the symbols in front of the sentinel, end[r] = the row whose symbol is the sentinel (what rb3_fmi_retrieve
 * returns), len32[r] the length once more for the scan.  EMIT: symbol t of the walk of row r to out[off[r - r0] + len[r] - 1 - t], inside
 * [0, cap).  ctr[0]: the next row to hand out (0 at launch), ctr[1] += LF steps, ctr[2] += walks that took more steps than the index has
 * rows (no index does that: the driver answers RB3GPU_EINTERNAL) */
template<bool EMIT> __global__ void __launch_bounds__(256) k_get_walk(IdxView ix, const int64_t *rows, int64_t r0, int64_t r1, int64_t *len, int64_t *end, uint32_t *len32,
		const int64_t *off, uint8_t *out, int64_t cap, unsigned long long *ctr)
{
	const int j = threadIdx.x & 7;
	bool act = false, done = false;
	int64_t r = 0, k = 0, t = 0, base = 0;
	unsigned long long steps = 0;
	for (;;) {
		while (!act && !done) {
			r = r0 + walk_take(ctr, j);
			if (r >= r1) { done = true; break; }
			k = rows[r], t = 0;
			if ((uint64_t)k < (uint64_t)ix.n) {
				if (EMIT) base = off[r - r0] + len[r] - 1, act = len[r] > 0; // (a string of no symbols: nothing to write)
				else act = true;
			} else if (!EMIT && j == 0) len[r] = 0, end[r] = -1, len32[r] = 0u;
		}
		if (__ballot(act) == 0ull) break;
		int c;
		const int64_t k2 = oct_lf_self(ix, act ? k : 0, j, &c);
		if (act) {
			++steps;
			if (c == 0 || t >= ix.n) { // the sentinel: the string starts here
				if (!EMIT && j == 0) len[r] = t, end[r] = k, len32[r] = (uint32_t)t;
				if (c != 0 && j == 0) atomicAdd(ctr + 2, 1ull);
				act = false;
			} else {
				if (EMIT) {
					const int64_t p = base - t;
					if (j == 0 && p >= 0 && p < cap) out[p] = (uint8_t)c;
				}
				++t, k = k2;
			}
		}
	}
	if (j == 0 && steps) atomicAdd(ctr + 1, steps);
}

/* `get` in pieces.  The rows are cut by the splitters of k_ssa_walk -- splitter p < m is sentinel row p, splitter p >= m is row m + ((p - m) << S),
 * nsp of them -- and a piece is the walk from a splitter's row to the next splitter's row or to the sentinel.  D(k): the LF steps from row k up to and including the
 * step that reads the sentinel; the symbol read at row k is symbol D(k) - 2 of its string.
 * COUNT (EMIT = false): the walkers are the nsp pieces and, behind them, the rows rows[0, nr) (each inside [0, ix.n): the driver keeps the others away).  A walker ends
 * where it reads the sentinel or lands on a splitter's row and leaves (next splitter, or RB3_SSA_END | string: the sentinel row LF leads to, below m; steps) in lnk[p]
 * or rq[v], one 16-byte store; the one that reads the sentinel of string s also notes the row it read it at in endrow[s].  A row asked for that is a splitter's row
 * is that splitter after no steps.  ctr[2] += walks of 2^24 - 1 steps without a splitter (the driver answers RB3GPU_EINTERNAL), ctr[3] = the longest piece.
 * EMIT: the items [0, ioff[nr]) of the rows rows[r0, r0 + nr): item ioff[v] is the walk of row v itself down to the splitter it met (rq[v].y steps, none for a
 * splitter's row), the items behind it are the pieces sorted[first[v]], sorted[first[v] + 1], ...: the pieces of the row's string from its end up to that splitter.
 * A symbol read at distance d goes to out[off[v] + d - 2], inside [0, cap).  ctr[2] += walks that ran past the start of their string (no index does that).
 * ctr[0]: the next walker to hand out (0 at launch), ctr[1] += LF steps */
struct PieceView {
	int S;
	int64_t nsp;
	ulonglong2 *lnk, *rq;          // (next, steps) per piece and per row asked for; after the join lnk[p] = (RB3_SSA_END | string, D)
	int64_t *endrow;               // per string: the row whose symbol is its sentinel
	const int64_t *rows, *ioff, *off;
	const uint32_t *first, *len32, *sorted;
};

template<bool EMIT> __global__ void __launch_bounds__(256) k_piece_walk(IdxView ix, PieceView pv, int64_t r0, int64_t nr, uint8_t *out, int64_t cap, unsigned long long *ctr)
{
	const int j = threadIdx.x & 7;
	const int64_t m = ix.m, maskS = ((int64_t)1 << pv.S) - 1, nw = EMIT ? pv.ioff[nr] : pv.nsp + nr;
	bool act = false, done = false, req = false;
	int64_t w = 0, k = 0, d = 0, base = 0;
	uint32_t l = 0, maxl = 0;
	unsigned long long steps = 0;
	for (;;) {
		while (!act && !done) { // (the same in the eight lanes of an octet)
			w = walk_take(ctr, j);
			if (w >= nw) { done = true; break; }
			if (!EMIT) {
				req = w >= pv.nsp, l = 0;
				if (!req) k = w < m ? w : m + ((w - m) << pv.S), act = true;
				else {
					k = pv.rows[w - pv.nsp];
					if ((uint64_t)k >= (uint64_t)ix.n) { if (j == 0) pv.rq[w - pv.nsp] = make_ulonglong2(RB3_SSA_END, 0ull); } // (never walked; the driver does not send one)
					else if (k < m || ((k - m) & maskS) == 0) { if (j == 0) pv.rq[w - pv.nsp] = make_ulonglong2((unsigned long long)(k < m ? k : m + ((k - m) >> pv.S)), 0ull); }
					else act = true;
				}
			} else {
				int64_t lo = 0, hi = nr; // the row of item w: the last v with ioff[v] <= w (w < ioff[nr])
				while (hi - lo > 1) {
					const int64_t mid = (lo + hi) >> 1;
					if (pv.ioff[mid] <= w) lo = mid; else hi = mid;
				}
				const int64_t v = r0 + lo, t = w - pv.ioff[lo];
				base = pv.off[lo] - 2;
				if (t == 0) k = pv.rows[v], d = (int64_t)pv.len32[v] + 1, act = pv.rq[v].y != 0ull && (uint64_t)k < (uint64_t)ix.n;
				else {
					const int64_t p = (int64_t)pv.sorted[(int64_t)pv.first[v] + t - 1];
					act = p < pv.nsp; // (it is: the sorted values are the piece ids)
					if (act) k = p < m ? p : m + ((p - m) << pv.S), d = (int64_t)pv.lnk[p].y;
				}
			}
		}
		if (__ballot(act) == 0ull) break;
		int c;
		const int64_t k2 = oct_lf_self(ix, act ? k : 0, j, &c);
		if (act) {
			++steps;
			const bool at_split = c != 0 && ((k2 - m) & maskS) == 0; // (k2 >= m whenever c != 0)
			if (!EMIT) {
				++l;
				const bool too_long = l >= (1u << RB3_SSA_LBITS) - 1u;
				if (c == 0 || at_split || too_long) {
					if (j == 0) {
						const ulonglong2 e = make_ulonglong2(c == 0 ? (RB3_SSA_END | (unsigned long long)k2) : (unsigned long long)(m + ((k2 - m) >> pv.S)), (unsigned long long)l);
						if (req) pv.rq[w - pv.nsp] = e; else pv.lnk[w] = e;
						if (c == 0 && (uint64_t)k2 < (uint64_t)m) pv.endrow[k2] = k;
						if (c != 0 && !at_split) atomicAdd(ctr + 2, 1ull);
					}
					if (!req && l > maxl) maxl = l;
					act = false;
				}
			} else {
				const int64_t p = base + d;
				if (c != 0 && j == 0 && p >= 0 && p < cap) out[p] = (uint8_t)c;
				--d;
				if (c == 0 || at_split) act = false;
				else if (d <= 0) { if (j == 0) atomicAdd(ctr + 2, 1ull); act = false; } // past the start of the string
			}
			k = k2;
		}
	}
	if (j == 0 && steps) atomicAdd(ctr + 1, steps);
	if (!EMIT && j == 0 && maxl) atomicMax(ctr + 3, (unsigned long long)maxl);
}

/* after the join: the sort key of piece p, (string << 32 | D - 1), and its value p.  err[0] += links that do not end in a string (cannot be after the jumping
 * rounds), err[1] += strings of 2^32 symbols or more */
__global__ void __launch_bounds__(256) k_piece_key(int64_t nsp, int64_t m, const ulonglong2 *lnk, uint64_t *key, uint32_t *val, unsigned long long *err)
{
	const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= nsp) return;
	const ulonglong2 e = lnk[p];
	const uint64_t s = e.x & ~RB3_SSA_END;
	if (!(e.x & RB3_SSA_END) || s >= (uint64_t)m || e.y == 0ull) atomicAdd(err, 1ull);
	else if (e.y - 1 > 0xFFFFFFFFull) atomicAdd(err + 1, 1ull);
	key[p] = s << 32 | ((e.y - 1) & 0xFFFFFFFFull), val[p] = (uint32_t)p;
}

/* pos[sorted[i]] = i: where every piece stands in the sorted order */
__global__ void __launch_bounds__(256) k_piece_inverse(int64_t nsp, const uint32_t *sorted, uint32_t *pos)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < nsp && sorted[i] < (uint64_t)nsp) pos[sorted[i]] = (uint32_t)i;
}

/* the rows asked for, one thread each: D = the row's own steps + D of the splitter it met, len = D - 1, the end row of its string, and its pieces in the sorted
 * order: [first, the place of that splitter], the first piece of string s being the lowest key of s << 32 and above; cnt = those pieces + 1 for the row's own
 * walk.  A row that read the sentinel before any splitter has no pieces.  err[0] += broken links, err[1] += strings of 2^32 symbols or more */
__global__ void __launch_bounds__(256) k_piece_resolve(int64_t nr, int64_t nsp, int64_t m, const ulonglong2 *lnk, const ulonglong2 *rq, const int64_t *endrow, const uint64_t *skey,
		const uint32_t *pos, int64_t *len, int64_t *end, uint32_t *len32, uint32_t *cnt32, uint32_t *first, unsigned long long *err)
{
	const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= nr) return;
	const ulonglong2 a = rq[v];
	uint64_t s, D = a.y, f = 0, c = 1;
	bool bad = false;
	if (a.x & RB3_SSA_END) s = a.x & ~RB3_SSA_END;
	else if (a.x >= (uint64_t)nsp) s = 0, bad = true;
	else {
		const ulonglong2 e = lnk[a.x];
		s = e.x & ~RB3_SSA_END, D += e.y;
		if (!(e.x & RB3_SSA_END) || s >= (uint64_t)m) bad = true;
		else {
			int64_t lo = 0, hi = nsp; // the first i with skey[i] >= s << 32
			while (lo < hi) {
				const int64_t mid = (lo + hi) >> 1;
				if (skey[mid] < (s << 32)) lo = mid + 1; else hi = mid;
			}
			f = (uint64_t)lo;
			if ((uint64_t)pos[a.x] < f) bad = true; else c = (uint64_t)pos[a.x] - f + 2;
		}
	}
	if (bad || s >= (uint64_t)m || D == 0) { atomicAdd(err, 1ull); len[v] = 0, end[v] = -1, len32[v] = 0u, cnt32[v] = 0u, first[v] = 0u; return; }
	if (D - 1 > 0xFFFFFFFFull) atomicAdd(err + 1, 1ull);
	len[v] = (int64_t)(D - 1), end[v] = endrow[s], len32[v] = (uint32_t)(D - 1), cnt32[v] = (uint32_t)c, first[v] = (uint32_t)f;
}

/* one walker of k_seed_walk: the window starts [a, b) of query q (the driver keeps b <= len - min_len + 1) */
struct SeedWalker { int64_t q; int32_t a, b; };

/* the walkers wk[0, nw) over windows of min_len >= 2 symbols (queries of fewer than 2^31 symbols: the driver refuses longer ones).  A walker that finds
 * a window whose min_len symbols occur sets present[q] = 1 (zeroed by the driver; every writer stores the same byte) and ends; it also ends without
 * looking further when another walker of its query has already done so.  ctr[0]: the next walker to hand out (0 at launch), ctr[1] += extension steps */
__global__ void __launch_bounds__(256) k_seed_walk(IdxView ix, Acc7 acc, const uint8_t *sym, const int64_t *qoff, const SeedWalker *wk, int64_t nw, int32_t min_len, uint8_t *present,
		unsigned long long *ctr)
{
	const int j = threadIdx.x & 7;
	bool act = false, done = false;
	int64_t q = 0, qb = 0, k = 0, l = 0;
	int32_t len = 0, x = 0, b = 0, i = -1;
	unsigned long long steps = 0;
	// the window that starts at x: false if there is none left for this walker; else the interval of its last symbol (no rank needed), the cursor in front of it
	auto window = [&]() -> bool {
		if (len - x < min_len || x >= b) return false; // (fm-index.c:489; the end of the walker's start range)
		if (*(const volatile uint8_t*)(present + q)) return false;
		const int c = min((int)sym[qb + x + min_len - 1], 5);
		k = acc.a[c], l = acc.a[c + 1], i = x + min_len - 2;
		return true;
	};
	for (;;) {
		while (!act && !done) { // (the same in the eight lanes of an octet)
			const int64_t w = walk_take(ctr, j);
			if (w >= nw) { done = true; break; }
			const SeedWalker s = wk[w];
			q = s.q, qb = qoff[q], len = (int32_t)(qoff[q + 1] - qb), x = s.a, b = s.b;
			act = window();
		}
		if (__ballot(act) == 0ull) break;
		// one extension by q[i] (fm-index.c:491-496): the ranks of that symbol at both ends
		const int c = act ? min((int)sym[qb + i], 5) : 0;
		RankLoad rl, ru;
		oct_rank_issue(ix, act ? k : 0, j, rl); // (a finished octet: a valid address, the result unused)
		oct_rank_issue(ix, act ? l : 0, j, ru);
		const int64_t nk = oct_rank_finish(rl, c, j, ix.abs), nl = oct_rank_finish(ru, c, j, ix.abs);
		if (act) {
			++steps;
			k = nk, l = nl;
			if (l - k <= 0) x = i + 1, act = window(); // q[i .. x + min_len - 1] does not occur: the next window starts behind i (fm-index.c:497)
			else if (--i < x) { // the whole window occurs: a seed
				if (j == 0) present[q] = 1;
				act = false;
			}
		}
	}
	if (j == 0 && steps) atomicAdd(ctr + 1, steps);
}

#endif
