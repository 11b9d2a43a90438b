/*
 * rb3gpu_reduce.h -- `overlap --reduce`: the irreducible overlaps of the string graph (no counterpart in the reference).
 *
 * All the records of `overlap` lie on the device, string r's at rec[off[r], off[r + 1]), longest overlap first and inside one length in ascending sentinel rank.  The
 * record j = (a, b, o) is reducible iff a record i = (a, c, o_c) of the same string in front of it has o_c > o and len(c) > o_c, and c's own list holds
 * (c, b, len(c) - o_c + o): c reaches beyond the end of a, and what it adds there is a prefix of what b adds.  c's list is in the same order, so that record is found
 * by one binary search on the key (len descending, rank_of[b] ascending).  A witness counts whether it is itself reducible or not: the answer for a record depends on
 * the records alone, not on any other answer, and nothing is ordered between records.
 *
 *   k_ovl_rank     rank_of[who[e]] = e: the sentinel rank of every string, the inverse of k_ovl_who's table.
 *   k_ovl_reduce   an octet of lanes per record j: the eight lanes stride over the candidates i of a's list, each with its own binary search in the list of its c; the
 *                  first hit of any lane ends the record.  One string's records are spread over as many octets, and a long list's candidates over the octet's lanes.
 *                  It reads the records and writes keep[j] once, from one lane: no atomics on the records.
 *   k_ovl_koff     koff[r] = pos[off[r]]: the kept records in front of string r, from the exclusive scan pos of keep.
 *   k_ovl_compact  out[pos[j] - kbase] = rec[j] where keep[j]: the kept records of a slice, in their order.
 */
#ifndef RB3GPU_REDUCE_H
#define RB3GPU_REDUCE_H

#include "rb3gpu_overlap.h"

/* who: m entries, each string once (k_ovl_who has checked it).  err[0] += entries that name no string */
__global__ void __launch_bounds__(256) k_ovl_rank(int64_t m, const uint32_t *who, uint32_t *rank_of, unsigned long long *err)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= m) return;
	const uint32_t r = who[e];
	if ((int64_t)r < m) rank_of[r] = (uint32_t)e;
	else atomicAdd(err, 1ull);
}

/* is (len, rank) in rec[lo, hi), a list ordered by len descending, then by rank_of[b] ascending? */
__device__ __forceinline__ bool ovl_list_has(const int4 *rec, const uint32_t *rank_of, int64_t m, int64_t lo, int64_t hi, int32_t len, uint32_t rank)
{
	while (lo < hi) {
		const int64_t mid = lo + ((hi - lo) >> 1);
		const int4 x = rec[mid];
		bool before; // x lies in front of the key
		if (x.z != len) before = x.z > len;
		else {
			const uint32_t rx = (uint64_t)(uint32_t)x.y < (uint64_t)m ? rank_of[(uint32_t)x.y] : RB3_OVL_NONE;
			if (rx == rank) return true;
			before = rx < rank;
		}
		if (before) lo = mid + 1;
		else hi = mid;
	}
	return false;
}

/* the records [j0, j1) of rec (n records in all, those of string r at [off[r], off[r + 1]), m strings): keep[j] = 1 where record j is kept, 0 where it is reducible
 * (written once per record, by lane 0 of its octet).  ctr[0] += reducible records, ctr[1] += kept records, ctr[2] += records that name a string outside the index
 * or lie outside their string's list, which are left as they were at launch (no index: the driver's guard) */
__global__ void __launch_bounds__(256) k_ovl_reduce(const OvlRec *rec_, const int64_t *off, const uint32_t *rank_of, int64_t m, int64_t n, int64_t j0, int64_t j1, uint32_t *keep,
		unsigned long long *ctr)
{
	const int4 *rec = reinterpret_cast<const int4*>(rec_);
	const int lane = threadIdx.x & 7, sh = (threadIdx.x & 63) & ~7; // the octet's bits of a ballot start at sh
	const int64_t n_oct = ((int64_t)gridDim.x * blockDim.x) >> 3;
	unsigned long long n_red = 0, n_keep = 0, n_bad = 0;
	for (int64_t j = j0 + ((((int64_t)blockIdx.x * blockDim.x + threadIdx.x)) >> 3); j < j1; j += n_oct) { // (the same in the eight lanes of an octet)
		const int4 me = rec[j]; // (a, b, o, len(b))
		const bool ok = (uint64_t)(uint32_t)me.x < (uint64_t)m && (uint64_t)(uint32_t)me.y < (uint64_t)m;
		const int64_t first = ok ? off[me.x] : j;
		const uint32_t rank_b = ok ? rank_of[(uint32_t)me.y] : 0u;
		bool hit = false, bad = !ok || first > j || off[ok ? me.x + 1 : 0] <= j;
		if (!bad)
			for (int64_t i0 = first; i0 < j; i0 += 8) { // eight candidates a round, in the list's order: the deepest first
				const int64_t i = i0 + lane;
				bool more = false; // a candidate with a longer overlap: the ones behind the last of them have none
				if (i < j) {
					const int4 w = rec[i]; // (a, c, o_c, len(c))
					more = w.z > me.z;
					if (more && w.w > w.z) { // c reaches beyond the end of a
						const uint32_t c = (uint32_t)w.y;
						if ((uint64_t)c < (uint64_t)m) {
							const int64_t lo = off[c], hi = off[c + 1];
							if (lo >= 0 && lo <= hi && hi <= n) hit = ovl_list_has(rec, rank_of, m, lo, hi, w.w - w.z + me.z, rank_b);
							else bad = true;
						} else bad = true;
					}
				}
				const unsigned oct = (unsigned)(__ballot(hit) >> sh) & 0xFFu, all_more = (unsigned)(__ballot(more) >> sh) & 0xFFu;
				if (oct != 0u || all_more != 0xFFu) { hit = oct != 0u; break; }
			}
		bad = ((unsigned)(__ballot(bad) >> sh) & 0xFFu) != 0u;
		if (lane == 0) {
			if (bad) ++n_bad;
			else if (hit) ++n_red, keep[j] = 0u;
			else ++n_keep, keep[j] = 1u;
		}
	}
	if (lane == 0) {
		if (n_red) atomicAdd(ctr + 0, n_red);
		if (n_keep) atomicAdd(ctr + 1, n_keep);
		if (n_bad) atomicAdd(ctr + 2, n_bad);
	}
}

/* koff[i] = pos[off[em[i]]] for the ne strings em[] that have records, koff[ne] = pos[off[m]]: pos has n + 1 entries, off[m] = n (-1: an offset outside them) */
__global__ void __launch_bounds__(256) k_ovl_koff(int64_t ne, const uint32_t *em, int64_t m, int64_t n, const int64_t *off, const int64_t *pos, int64_t *koff)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i > ne) return;
	const int64_t r = i < ne ? (int64_t)em[i] : m;
	const int64_t o = r <= m ? off[r] : -1;
	koff[i] = (uint64_t)o <= (uint64_t)n ? pos[o] : -1;
}

/* the records [j0, j1): the kept ones to out[pos[j] - kbase], inside [0, cap).  err[0] += kept records that would land outside */
__global__ void __launch_bounds__(256) k_ovl_compact(const OvlRec *rec, const uint32_t *keep, const int64_t *pos, int64_t j0, int64_t j1, int64_t kbase, OvlRec *out, int64_t cap,
		unsigned long long *err)
{
	const int64_t j = j0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= j1 || keep[j] == 0u) return;
	const int64_t d = pos[j] - kbase;
	if (d >= 0 && d < cap) reinterpret_cast<int4*>(out)[d] = reinterpret_cast<const int4*>(rec)[j];
	else atomicAdd(err, 1ull);
}

#endif
