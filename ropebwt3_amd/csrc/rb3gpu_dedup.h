/*
 * rb3gpu_dedup.h -- `dedup`: which strings of the index are copies of another one or lie inside a longer one (no counterpart in the reference).
 *
 * The LF walk of `get` from row r spells string r from its last symbol to its first; fed with those symbols the backward search of `suffix` finds every
 * place the string occurs at.  One chain per string does both, with two intervals: `any` from all the rows [0, n), `suf` from the sentinels' rows [0, m), which
 * holds the rows whose suffix is the string read so far followed by a sentinel.  At the sentinel
 *   occ    = |any|                     the string as a substring anywhere in the index, itself included;
 *   cls    = occ0(suf.lo)              the strings that sort in front of it: the same for all of its copies and for no other string;
 *   copies = occ0(suf.hi) - cls        the strings that ARE this string.
 * A string lies inside a longer one iff occ > copies.  `any` always holds the walk's own row: once |any| == 1 the string is unique, and the walk ends there.
 *
 *   k_dedup_walk    an octet of lanes per string.  A step is oct_lf_self at the row and the rank pairs of k_suffix_walk at the ends of both intervals, FIVE
 *                   loads issued before any of them is decoded -- the symbol is needed by oct_rank_finish only.  A load is the two dependent trips of every rank
 *                   (the directory's slot word, then the slot), so a step is those two trips with five requests in flight in each, not three times two.
 *   k_dedup_keeper  the smallest unit of every class of more than one string: atomicMin into a table of m entries, indexed by cls.
 *   k_dedup_kind    K, D or C and the keeper per unit (a row, or with pair the rows 2u and 2u + 1, judged on row 2u).
 */
#ifndef RB3GPU_DEDUP_H
#define RB3GPU_DEDUP_H

#include "rb3gpu_walk.h"

struct DedupRec { int64_t occ, copies, cls; };                       // rb3gpu_dedup_rec_t

#define RB3_DEDUP_NONE 0xFFFFFFFFu                                   // a class nobody has entered (units are below 2^31)

/* the strings [r0, r1) (each below ix.m: the driver's), the record of string r to out[r].  early != 0: a walk whose `any` has come down to one row ends there with
 * (1, 1, -1).  ctr[0]: the next string to hand out (0 at launch), ctr[1] += steps, ctr[2] += walks of more steps than the index has rows (no index does that),
 * ctr[3] += walks whose own last row is not among the copies counted (the sanity count), ctr[4] += early exits, ctr[5] += strings of 2^31 symbols or more */
__global__ void __launch_bounds__(256) k_dedup_walk(IdxView ix, int64_t r0, int64_t r1, int early, DedupRec *out, unsigned long long *ctr)
{
	const int j = threadIdx.x & 7;
	bool act = false, done = false;
	int64_t r = 0, k = 0, al = 0, ah = 0, sl = 0, sh = 0, t = 0;
	unsigned long long steps = 0, n_early = 0;
	for (;;) {
		while (!act && !done) { // (the same in the eight lanes of an octet)
			r = r0 + walk_take(ctr, j);
			if (r >= r1) { done = true; break; }
			k = r, al = 0, ah = ix.n, sl = 0, sh = ix.m, t = 0;
			act = (uint64_t)r < (uint64_t)ix.m;
		}
		if (__ballot(act) == 0ull) break;
		// the five loads of a step, then the symbol at the row (oct_lf_self), then the ranks of that symbol
		RankLoad rk, ral, rah, rsl, rsh;
		oct_rank_issue(ix, act ? k : 0, j, rk); // (a finished octet: a valid address, the result unused)
		oct_rank_issue(ix, act ? al : 0, j, ral);
		oct_rank_issue(ix, act ? ah : 0, j, rah);
		oct_rank_issue(ix, act ? sl : 0, j, rsl);
		oct_rank_issue(ix, act ? sh : 0, j, rsh);
		const uint32_t hdr0 = oct_bcast0(rk.sl.x, j);
		const int c = (int)(oct_sum(slice_sym(rk.sl, hdr0, rk.koff - (hdr0 & 0xFFFFu), j)) & 7u);
		const int cc = c <= 5 ? c : 5;
		const int64_t nk = oct_rank_finish(rk, cc, j, ix.abs), nal = oct_rank_finish(ral, cc, j, ix.abs), nah = oct_rank_finish(rah, cc, j, ix.abs);
		const int64_t nsl = oct_rank_finish(rsl, cc, j, ix.abs), nsh = oct_rank_finish(rsh, cc, j, ix.abs);
		if (act) {
			++steps;
			if (c == 0) { // the sentinel: the string starts here; nk, nsl, nsh are occ0 at the row and at the ends of suf
				if (j == 0) {
					DedupRec x;
					x.occ = ah - al, x.copies = nsh - nsl, x.cls = nsl;
					out[r] = x;
					if (nk < nsl || nk >= nsh) atomicAdd(ctr + 3, 1ull);
				}
				act = false;
			} else if (t >= ix.n || t >= 0x7fffffffLL || nah <= nal || nsh <= nsl) { // (no index: the intervals of a string that is there never empty)
				if (j == 0) {
					DedupRec x;
					x.occ = 0, x.copies = 0, x.cls = -1;
					out[r] = x;
					atomicAdd(ctr + (t < ix.n && t >= 0x7fffffffLL ? 5 : 2), 1ull);
				}
				act = false;
			} else {
				++t, k = nk, al = nal, ah = nah, sl = nsl, sh = nsh;
				if (early && ah - al == 1) { // nothing but the string itself
					if (j == 0) {
						DedupRec x;
						x.occ = 1, x.copies = 1, x.cls = -1;
						out[r] = x;
					}
					++n_early, act = false;
				}
			}
		}
	}
	if (j == 0 && steps) atomicAdd(ctr + 1, steps);
	if (j == 0 && n_early) atomicAdd(ctr + 4, n_early); // (one add per octet, as for the steps: the counters share a line with ctr[0], which every octet waits for)
}

/* one thread per row r < m: a row with copies > 1 enters its unit (r >> pair) into keep[cls] (RB3_DEDUP_NONE at launch; m entries).  err[0] += records whose class
 * is outside the table */
__global__ void __launch_bounds__(256) k_dedup_keeper(int64_t m, int pair, const DedupRec *rec, uint32_t *keep, unsigned long long *err)
{
	const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= m) return;
	const DedupRec x = rec[r];
	if (x.copies <= 1) return;
	if ((uint64_t)x.cls >= (uint64_t)m) { atomicAdd(err, 1ull); return; }
	atomicMin(keep + x.cls, (uint32_t)(r >> pair));
}

/* one thread per i < m.  i < nu: unit i, judged on row i << pair: 'C' where occ > copies (not with dup_only), else 'D' where copies > 1 and the keeper of its class
 * is another unit, else 'K'; keeper[i] = that keeper, i itself where copies == 1.  With pair, cnt[3] += units whose two rows disagree in occ or copies.
 * Every i: cnt[2] += classes entered.  cnt[0] += D, cnt[1] += C */
__global__ void __launch_bounds__(256) k_dedup_kind(int64_t m, int64_t nu, int pair, int dup_only, const DedupRec *rec, const uint32_t *keep, uint8_t *kind, int64_t *keeper, unsigned long long *cnt)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int lane = (int)(threadIdx.x & 63u);
	bool isd = false, isc = false, cls = false, bad = false;
	if (i < m) cls = keep[i] != RB3_DEDUP_NONE;
	if (i < nu) {
		const DedupRec x = rec[i << pair];
		if (pair) {
			const DedupRec y = rec[(i << 1) + 1];
			bad = x.occ != y.occ || x.copies != y.copies;
		}
		int64_t kp = i;
		if (x.copies > 1 && (uint64_t)x.cls < (uint64_t)m) kp = (int64_t)keep[x.cls];
		isc = !dup_only && x.occ > x.copies;
		isd = !isc && x.copies > 1 && kp != i;
		kind[i] = (uint8_t)(isc ? 'C' : isd ? 'D' : 'K');
		keeper[i] = kp;
	}
	const unsigned long long bd = __ballot(isd), bc = __ballot(isc), bl = __ballot(cls), bb = __ballot(bad);
	if (lane == 0) {
		if (bd) atomicAdd(cnt, (unsigned long long)__popcll(bd));
		if (bc) atomicAdd(cnt + 1, (unsigned long long)__popcll(bc));
		if (bl) atomicAdd(cnt + 2, (unsigned long long)__popcll(bl));
		if (bb) atomicAdd(cnt + 3, (unsigned long long)__popcll(bb));
	}
}

#endif
