/*
 * rb3gpu_fetch.h -- `fetch`: regions of the indexed strings through the sampled suffix array (no counterpart in the reference).
 *
 * Sample x of the sampled suffix array is row m + (x << ss) with ssa[x] = o << ms | s: that row is the suffix of string s (the `get` row s < m) that starts at
 * text offset o; sentinel row r is offset len(r) of string r.  One LF step from the row of offset o reads symbol o - 1 and leads to the row of offset o - 1.
 * Sorted by (s, o) -- the TABLE, a permutation of the samples made once per sampled suffix array (k_fetch_key and a radix sort) -- the samples are an index from
 * text coordinates to rows, and a region [beg, end) of string r is read by
 *   the ANCHOR       the sample of r with the smallest offset >= end, or sentinel row r at offset len(r) where there is none, and
 *   the INNER ones   every sample of r with beg < o < end,
 * each a walker of its own that goes down to beg or to the row of the next sample, whichever comes first.  The steps of a region sum to o_anchor - beg and no
 * walker goes further than one gap between samples.
 *
 *   k_fetch_key    the sort key of every sample: s << obits | o
 *   k_fetch_plan   a thread per region: the range test, two binary searches in the table, the anchor, the number of walkers; a region without an anchor goes
 *                  on a list
 *   k_fetch_len    the regions of that list, an octet each: the walk from row r to the first sample it lands on (len = its offset + the steps) or to the
 *                  sentinel (len = the steps - 1); the anchor is (r, len), and end > len is an invalid region
 *   k_fetch_walk   the walkers of a slice of regions, an octet each, in the shape of k_piece_walk<true>
 */
#ifndef RB3GPU_FETCH_H
#define RB3GPU_FETCH_H

#include "rb3gpu_walk.h"

struct FetchRegion { int64_t row, beg, end; };                        // rb3gpu_region_t

struct FetchView {
	int ss, ms;                    // sample spacing 2^ss, bits of the string in a sample
	int64_t n_ssa;
	const uint64_t *ssa;           // ssa[n_ssa]
	const uint32_t *tab;           // the samples by (string, offset)
	const FetchRegion *reg;
	int64_t *ak, *ao;              // per region: row and offset of its anchor
	uint32_t *first, *cnt32;       // per region: its first inner walker in tab, its walkers (inner + 1; 0 for an invalid region)
	int64_t *mlist;                // the regions without an anchor
	const int64_t *ioff, *off;     // per region of a slice: its first walker, its first symbol in out
};

__global__ void __launch_bounds__(256) k_fetch_key(int64_t n_ssa, int ms, int obits, const uint64_t *ssa, uint64_t *key, uint32_t *val)
{
	const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= n_ssa) return;
	const uint64_t t = ssa[x];
	key[x] = (t & ((1ull << ms) - 1)) << obits | ((t >> ms) & ((1ull << obits) - 1)), val[x] = (uint32_t)x;
}

/* the first i in [0, n_ssa] whose sample is not below (string r, offset o) */
__device__ __forceinline__ int64_t fetch_lower(const FetchView &fv, uint64_t r, uint64_t o)
{
	const uint64_t smask = (1ull << fv.ms) - 1;
	int64_t lo = 0, hi = fv.n_ssa;
	while (lo < hi) {
		const int64_t mid = (lo + hi) >> 1;
		const uint64_t t = fv.ssa[fv.tab[mid]], s = t & smask;
		if (s < r || (s == r && (t >> fv.ms) < o)) lo = mid + 1; else hi = mid;
	}
	return lo;
}

/* the regions [0, n).  ctr[4] += regions without an anchor (mlist), ctr[5] = the first region that fails the range test (min; ~0 at launch) */
__global__ void __launch_bounds__(256) k_fetch_plan(FetchView fv, int64_t n, int64_t m, unsigned long long *ctr)
{
	const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= n) return;
	const FetchRegion g = fv.reg[v];
	if (g.row < 0 || g.row >= m || g.beg < 0 || g.beg >= g.end) {
		fv.ak[v] = -1, fv.ao[v] = -1, fv.first[v] = 0u, fv.cnt32[v] = 0u;
		atomicMin(ctr + 5, (unsigned long long)v);
		return;
	}
	const int64_t first = fetch_lower(fv, (uint64_t)g.row, (uint64_t)g.beg + 1), last = fetch_lower(fv, (uint64_t)g.row, (uint64_t)g.end);
	fv.first[v] = (uint32_t)first, fv.cnt32[v] = (uint32_t)(last - first + 1);
	bool anchored = false;
	if (last < fv.n_ssa) {
		const uint64_t x = fv.tab[last], t = fv.ssa[x];
		if ((t & ((1ull << fv.ms) - 1)) == (uint64_t)g.row) fv.ak[v] = m + (int64_t)(x << fv.ss), fv.ao[v] = (int64_t)(t >> fv.ms), anchored = true;
	}
	if (!anchored) {
		fv.ak[v] = g.row, fv.ao[v] = -1; // (k_fetch_len measures the offset)
		fv.mlist[atomicAdd(ctr + 4, 1ull)] = v;
	}
}

/* the regions mlist[0, ctr[4]): ao = the length of the region's string.  ctr[0]: the next one to hand out (0 at launch), ctr[1] += LF steps, ctr[2] += samples of
 * another string met and walks longer than the index has rows, ctr[5] = the first region with end beyond the length (min) */
__global__ void __launch_bounds__(256) k_fetch_len(IdxView ix, FetchView fv, unsigned long long *ctr)
{
	const int j = threadIdx.x & 7;
	const int64_t m = ix.m, mask = ((int64_t)1 << fv.ss) - 1, nm = (int64_t)ctr[4];
	bool act = false, done = false;
	int64_t v = 0, row = 0, k = 0, t = 0;
	unsigned long long steps = 0;
	for (;;) {
		while (!act && !done) { // (the same in the eight lanes of an octet)
			const int64_t w = walk_take(ctr, j);
			if (w >= nm) { done = true; break; }
			v = fv.mlist[w], row = k = fv.reg[v].row, t = 0, act = true;
		}
		if (__ballot(act) == 0ull) break;
		int c;
		const int64_t k2 = oct_lf_self(ix, act ? k : 0, j, &c);
		if (act) {
			++steps, ++t;
			const bool at_split = c != 0 && ((k2 - m) & mask) == 0; // (k2 >= m whenever c != 0)
			if (c == 0 || at_split || t > ix.n) {
				int64_t len = t - 1;
				bool bad = c != 0 && !at_split;
				if (at_split) {
					const int64_t x2 = (k2 - m) >> fv.ss;
					const uint64_t s2 = x2 < fv.n_ssa ? fv.ssa[x2] : ~0ull;
					len = (int64_t)(s2 >> fv.ms) + t;
					if ((s2 & ((1ull << fv.ms) - 1)) != (uint64_t)row || x2 >= fv.n_ssa) bad = true;
				}
				if (j == 0) {
					fv.ao[v] = len;
					if (bad) atomicAdd(ctr + 2, 1ull);
					else if (fv.reg[v].end > len) atomicMin(ctr + 5, (unsigned long long)v);
				}
				act = false;
			}
			k = k2;
		}
	}
	if (j == 0 && steps) atomicAdd(ctr + 1, steps);
}

/* the walkers [0, ioff[nr]) of the regions [r0, r0 + nr): walker ioff[v] is the anchor of region r0 + v, the ones behind it its inner samples tab[first], tab[first + 1],
 * ...  The symbol read at offset o - 1 goes to out[off[v] + o - 1 - beg] if it lies in the region, inside [0, cap).  ctr[0]: the next walker to hand out (0 at launch),
 * ctr[1] += LF steps, ctr[2] += samples met that are not (string, offset) of their walker and sentinels read above beg, ctr[3] = the longest walk */
__global__ void __launch_bounds__(256) k_fetch_walk(IdxView ix, FetchView fv, int64_t r0, int64_t nr, uint8_t *out, int64_t cap, unsigned long long *ctr)
{
	const int j = threadIdx.x & 7;
	const int64_t m = ix.m, mask = ((int64_t)1 << fv.ss) - 1, nw = fv.ioff[nr];
	bool act = false, done = false;
	int64_t k = 0, o = 0, beg = 0, end = 0, base = 0, row = 0;
	unsigned long long steps = 0, l = 0, maxl = 0;
	for (;;) {
		while (!act && !done) { // (the same in the eight lanes of an octet)
			const int64_t w = walk_take(ctr, j);
			if (w >= nw) { done = true; break; }
			int64_t lo = 0, hi = nr; // the region of walker w: the last v with ioff[v] <= w (w < ioff[nr])
			while (hi - lo > 1) {
				const int64_t mid = (lo + hi) >> 1;
				if (fv.ioff[mid] <= w) lo = mid; else hi = mid;
			}
			const int64_t v = r0 + lo, t = w - fv.ioff[lo];
			const FetchRegion g = fv.reg[v];
			row = g.row, beg = g.beg, end = g.end, base = fv.off[lo] - beg, l = 0;
			if (t == 0) k = fv.ak[v], o = fv.ao[v];
			else {
				const int64_t i = (int64_t)fv.first[v] + t - 1;
				const uint64_t x = i < fv.n_ssa ? fv.tab[i] : 0u;
				k = m + (int64_t)(x << fv.ss), o = i < fv.n_ssa ? (int64_t)(fv.ssa[x] >> fv.ms) : 0;
			}
			act = o > beg && (uint64_t)k < (uint64_t)ix.n;
		}
		if (__ballot(act) == 0ull) break;
		int c;
		const int64_t k2 = oct_lf_self(ix, act ? k : 0, j, &c);
		if (act) {
			++steps, ++l;
			if (c == 0) { // the start of the string above beg: not the sampled suffix array of this index
				if (j == 0) atomicAdd(ctr + 2, 1ull);
				act = false;
			} else {
				--o; // (the offset of the symbol read, and of row k2)
				const int64_t p = base + o;
				if (j == 0 && o < end && p >= 0 && p < cap) out[p] = (uint8_t)c; // (o >= beg)
				if (o == beg) act = false;
				else if (((k2 - m) & mask) == 0) { // the next walker's row: it must say so
					const int64_t x2 = (k2 - m) >> fv.ss;
					if (j == 0 && (x2 >= fv.n_ssa || fv.ssa[x2] != ((uint64_t)o << fv.ms | (uint64_t)row))) atomicAdd(ctr + 2, 1ull);
					act = false;
				}
			}
			if (!act && l > maxl) maxl = l;
			k = k2;
		}
	}
	if (j == 0 && steps) atomicAdd(ctr + 1, steps);
	if (j == 0 && maxl) atomicMax(ctr + 3, maxl);
}

#endif
