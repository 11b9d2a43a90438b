/*
 * rb3gpu_overlap.h -- `overlap`: which strings of the index overlap, end to start, and by how much (no counterpart in the reference).
 *
 * The LF walk of `get` from row a spells string a from its last symbol to its first; fed with those symbols the backward search of `suffix`, started from all
 * the rows, holds after d symbols every row whose suffix starts with the last d symbols of a.  The rows of that interval whose BWT symbol is the sentinel are the
 * strings that START with those d symbols: occ0(hi) - occ0(lo) of them, and the sentinel ranks in between name them.  The pass that reads a's own sentinel is depth
 * len(a), the whole string: not an overlap.  The interval always holds the walk's own row; once it is that row alone nothing but the whole string is left.
 *
 *   k_ovl_walk<EMIT>  an octet of lanes per string.  A pass is the rank loads at the row and at both ends of the interval, THREE loads issued before any is decoded;
 *                     the two interval loads are finished a second time with symbol 0 where the depth has reached min_len: no further memory trip.  COUNT notes per
 *                     string the records and the largest depth with a kept group; EMIT walks the strings that have records again, down to that depth only, and
 *                     stores the group of depth p at off + cnt - (written so far) - z: longest overlap first, without a sort.
 *   k_ovl_iota        rows[r] = r: the rows k_get_walk<false> walks for the lengths and the end rows of all the strings.
 *   k_ovl_who         who[occ0(end[r])] = r: the string every sentinel rank belongs to, each entry written exactly once.
 */
#ifndef RB3GPU_OVERLAP_H
#define RB3GPU_OVERLAP_H

#include "rb3gpu_walk.h"

struct OvlRec { int32_t a, b, len, len_b; };                         // rb3gpu_overlap_rec_t

#define RB3_OVL_NONE 0xFFFFFFFFu                                     // a sentinel rank nobody has claimed (strings are below 2^31)

/* COUNT (EMIT = false): the strings [r0, r1) (each below ix.m: the driver's); cnt[r] = the records of string r, last[r] = the largest depth with a kept group (-1:
 * none).  A group is the z > 0 sentinels inside the interval at a depth p >= min_len in front of the string's first symbol; it is kept where max_hits == 0 or
 * z <= max_hits.  early != 0: a walk whose interval has come down to one row ends there.
 * EMIT: the strings em[r0, r1), each with cnt > 0: the passes 0 .. last[r], the group of depth p to out[off[r] - obase + cnt[r] - written - z ..], inside [0, cap), its
 * records in ascending sentinel rank e: (r, who[e], p, len32[who[e]]), the eight lanes striding over them.
 * ctr[0]: the next string to hand out (0 at launch), ctr[1] += passes, ctr[2] += walks of more passes than the index has rows or with an empty interval (no index
 * does that), ctr[3] += strings of 2^31 symbols or more, ctr[4] += early exits, ctr[5] += kept groups, ctr[6] += groups over the cap, ctr[7] += their sentinels,
 * ctr[8] += records (COUNT: counted, EMIT: stored), ctr[9] += strings of 2^31 records or more, ctr[10] += (EMIT) strings whose stored records are not cnt[r] */
template<bool EMIT> __global__ void __launch_bounds__(256) k_ovl_walk(IdxView ix, int64_t r0, int64_t r1, int32_t min_len, int64_t max_hits, int early, const uint32_t *em,
		uint32_t *cnt, int32_t *last, const int64_t *off, int64_t obase, const uint32_t *who, const uint32_t *len32, OvlRec *out, int64_t cap, unsigned long long *ctr)
{
	const int j = threadIdx.x & 7;
	bool act = false, done = false;
	int64_t r = 0, k = 0, lo = 0, hi = 0, p = 0, nrec = 0, base = 0;
	int32_t lastp = -1;
	unsigned long long steps = 0, n_early = 0, n_grp = 0, n_cgrp = 0, n_chit = 0, n_rec = 0;
	for (;;) {
		while (!act && !done) { // (the same in the eight lanes of an octet)
			r = r0 + walk_take(ctr, j);
			if (r >= r1) { done = true; break; }
			if (EMIT) r = (int64_t)em[r];
			k = r, lo = 0, hi = ix.n, p = 0, nrec = 0, lastp = -1;
			act = (uint64_t)r < (uint64_t)ix.m;
			if (EMIT && act) lastp = last[r], base = off[r] - obase + (int64_t)cnt[r], act = cnt[r] > 0u && lastp >= 0;
		}
		if (__ballot(act) == 0ull) break;
		// the three loads of a pass, then the symbol at the row (oct_lf_self), then the ranks of that symbol
		RankLoad rk, rl, rh;
		oct_rank_issue(ix, act ? k : 0, j, rk); // (a finished octet: a valid address, the result unused)
		oct_rank_issue(ix, act ? lo : 0, j, rl);
		oct_rank_issue(ix, act ? hi : 0, j, rh);
		const uint32_t hdr0 = oct_bcast0(rk.sl.x, j);
		const int c = (int)(oct_sum(slice_sym(rk.sl, hdr0, rk.koff - (hdr0 & 0xFFFFu), j)) & 7u);
		const int cc = c <= 5 ? c : 5;
		const int64_t nk = oct_rank_finish(rk, cc, j, ix.abs), nlo = oct_rank_finish(rl, cc, j, ix.abs), nhi = oct_rank_finish(rh, cc, j, ix.abs);
		const bool deep = act && c != 0 && p >= (int64_t)min_len;
		int64_t e0 = 0, e1 = 0;
		if (__ballot(deep) != 0ull) // (the whole wave or none of it: the shuffles inside see every lane) the sentinels in front of both ends
			e0 = oct_rank_finish(rl, 0, j, ix.abs), e1 = oct_rank_finish(rh, 0, j, ix.abs);
		if (act) {
			++steps;
			if (c == 0) act = false; // the sentinel: the string starts here; depth p is the whole string
			else if (p >= ix.n || p >= 0x7fffffffLL || nhi <= nlo) { // (no index: the interval of a string that is there never empties)
				if (j == 0) atomicAdd(ctr + (p < ix.n && p >= 0x7fffffffLL ? 3 : 2), 1ull);
				act = false;
			} else {
				const int64_t z = deep ? e1 - e0 : 0;
				if (z > 0) {
					if (max_hits == 0 || z <= max_hits) {
						++n_grp, n_rec += (unsigned long long)z;
						if (EMIT) {
							const int64_t dst = base - nrec - z; // in front of the shorter overlaps written so far
							for (int64_t i = j; i < z; i += 8) {
								const int64_t e = e0 + i, d = dst + i;
								if ((uint64_t)e < (uint64_t)ix.m && d >= 0 && d < cap) {
									const uint32_t b = who[e];
									reinterpret_cast<int4*>(out)[d] = make_int4((int)r, (int)b, (int)p, b < (uint32_t)ix.m ? (int)len32[b] : -1); // one 16-byte store
								}
							}
						} else lastp = (int32_t)p;
						nrec += z;
					} else ++n_cgrp, n_chit += (unsigned long long)z;
				}
				if (EMIT && p >= (int64_t)lastp) act = false; // nothing kept beyond this depth
				else {
					++p, k = nk, lo = nlo, hi = nhi;
					if (!EMIT && early && hi - lo == 1) ++n_early, act = false; // nothing but the string itself: only its whole length is left
				}
			}
			if (!act && j == 0) {
				if (!EMIT) {
					cnt[r] = (uint32_t)(nrec < 0x80000000LL ? nrec : 0), last[r] = lastp;
					if (nrec >= 0x80000000LL) atomicAdd(ctr + 9, 1ull);
				} else if (nrec != (int64_t)cnt[r]) atomicAdd(ctr + 10, 1ull);
			}
		}
	}
	if (j == 0) { // (one add per octet and counter: they share a line with ctr[0], which every octet waits for)
		if (steps) atomicAdd(ctr + 1, steps);
		if (n_early) atomicAdd(ctr + 4, n_early);
		if (n_grp) atomicAdd(ctr + 5, n_grp);
		if (n_cgrp) atomicAdd(ctr + 6, n_cgrp);
		if (n_chit) atomicAdd(ctr + 7, n_chit);
		if (n_rec) atomicAdd(ctr + 8, n_rec);
	}
}

__global__ void __launch_bounds__(256) k_ovl_iota(int64_t m, int64_t *rows)
{
	const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r < m) rows[r] = r;
}

/* an octet per string r < m: end[r] is the row whose symbol is r's sentinel (k_get_walk<false>), and the sentinels in front of it are its rank: who[that rank] = r
 * (RB3_OVL_NONE at launch; m entries).  err[0] += rows that hold no sentinel, ranks outside the table and entries claimed twice: with none of them every entry is
 * written exactly once */
__global__ void __launch_bounds__(256) k_ovl_who(IdxView ix, const int64_t *end, uint32_t *who, unsigned long long *err)
{
	const int j = threadIdx.x & 7;
	const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
	const bool act = r < ix.m; // (the same in the eight lanes of an octet)
	const int64_t k = act ? end[r] : 0;
	const bool ok = act && (uint64_t)k < (uint64_t)ix.n;
	int c;
	const int64_t e = oct_lf_self(ix, ok ? k : 0, j, &c); // (a row that is not there: a valid address, the result unused)
	if (act && j == 0) {
		if (!ok || c != 0 || (uint64_t)e >= (uint64_t)ix.m) atomicAdd(err, 1ull);
		else if (atomicExch(who + e, (uint32_t)r) != RB3_OVL_NONE) atomicAdd(err, 1ull);
	}
}

#endif
