/*
 * rb3gpu_remove.h -- `remove`: strings taken out of the index (no counterpart in the reference).
 *
 * String r < m occupies the rows the LF walk from row r stands on, up to and including the row whose symbol is the sentinel: len + 1 rows.  The order of
 * the rows that stay depends on the strings that stay alone, and the symbol of a row belongs to its own string, so the BWT without those strings is the
 * BWT without those rows.  Three steps:
 *
 *   mark     one bit per row of the index (32-bit words, 256 of them per group of 8192 rows), set by lane 0 of the octet that stands on the row:
 *            k_mark_walk    the step of k_get_walk, one octet per string asked for, from row r down to its sentinel;
 *            k_mark_pieces  the step of k_piece_walk over the pieces that k_piece_walk<false> and k_ssa_jump have given their strings: a piece walks
 *                           only if its string is flagged (k_mark_flag), from its splitter's row up to the row in front of the next splitter's.
 *   count    k_mark_count: the marked rows of every group (the rank of the compaction) and, from the symbols at those rows, how many of each letter go.
 *   compact  k_rm_compact: the rows of whole groups that are not marked, each to (rows kept in front of it) - p0, where that lies inside the range of
 *            new positions asked for.  This is the range source of the chunked builder (from_fmd_chunked): it reads the OLD index through a view taken
 *            before the builder ran, while the builder writes the other index buffer.
 */
#ifndef RB3GPU_REMOVE_H
#define RB3GPU_REMOVE_H

#include "rb3gpu_walk.h"

#define RB3_RM_WORDS (RB3_GRP / 32)           // bitmap words of a group: one per thread of a block of 256
static_assert(RB3_RM_WORDS == 256, "a block of 256 threads holds the bitmap of one group");

__device__ __forceinline__ void mark_row(uint32_t *bm, int64_t k)
{
	atomicOr(bm + (k >> 5), 1u << ((uint32_t)k & 31u));
}

/* the strings rows[0, nr) (each below ix.m: the driver refuses the others; one that is not inside the index is not walked).  Every row the walk stands on is
 * marked, the one that reads the sentinel included.  ctr[0]: the next string to hand out (0 at launch), ctr[1] += LF steps = rows marked, ctr[2] += walks of
 * more steps than the index has rows (no index does that) */
__global__ void __launch_bounds__(256) k_mark_walk(IdxView ix, const int64_t *rows, int64_t nr, uint32_t *bm, unsigned long long *ctr)
{
	const int j = threadIdx.x & 7;
	bool act = false, done = false;
	int64_t k = 0, t = 0;
	unsigned long long steps = 0;
	for (;;) {
		while (!act && !done) { // (the same in the eight lanes of an octet)
			const int64_t r = walk_take(ctr, j);
			if (r >= nr) { done = true; break; }
			k = rows[r], t = 0;
			act = (uint64_t)k < (uint64_t)ix.n;
		}
		if (__ballot(act) == 0ull) break;
		if (act && j == 0) mark_row(bm, k);
		int c;
		const int64_t k2 = oct_lf_self(ix, act ? k : 0, j, &c);
		if (act) {
			++steps;
			if (c == 0 || t >= ix.n) { // the sentinel: the string starts here
				if (c != 0 && j == 0) atomicAdd(ctr + 2, 1ull);
				act = false;
			} else ++t, k = k2;
		}
	}
	if (j == 0 && steps) atomicAdd(ctr + 1, steps);
}

/* after the join (lnk[p] = (RB3_SSA_END | string, D) for every piece p): the strings of the rows asked for -- row r < m is splitter r -- are flagged, one byte
 * each.  err[0] += links that do not end in a string, err[1] += strings of 2^32 symbols or more, err[2] += D = len + 1 of the flagged strings */
__global__ void __launch_bounds__(256) k_mark_flag(int64_t nr, const int64_t *rows, int64_t m, const ulonglong2 *lnk, uint8_t *flag, unsigned long long *err)
{
	const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= nr) return;
	const int64_t r = rows[v];
	if ((uint64_t)r >= (uint64_t)m) { atomicAdd(err, 1ull); return; }
	const ulonglong2 e = lnk[r];
	const uint64_t s = e.x & ~RB3_SSA_END;
	if (!(e.x & RB3_SSA_END) || s >= (uint64_t)m || e.y == 0ull) { atomicAdd(err, 1ull); return; }
	if (e.y - 1 > 0xFFFFFFFFull) atomicAdd(err + 1, 1ull);
	flag[s] = 1;
	atomicAdd(err + 2, e.y);
}

/* the pieces [0, nsp) of k_piece_walk (splitter p < m is row p, splitter p >= m is row m + ((p - m) << S)): piece p marks its rows if flag[its string] is set.
 * It stops behind the row that reads the sentinel, or in front of the next splitter's row, which the next piece marks.  ctr[0]: the next piece to hand out
 * (0 at launch), ctr[1] += LF steps = rows marked, ctr[2] += pieces without a string or of 2^24 steps and more (cannot be after k_piece_walk<false>) */
__global__ void __launch_bounds__(256) k_mark_pieces(IdxView ix, int S, int64_t nsp, const ulonglong2 *lnk, const uint8_t *flag, uint32_t *bm, unsigned long long *ctr)
{
	const int j = threadIdx.x & 7;
	const int64_t m = ix.m, maskS = ((int64_t)1 << S) - 1;
	bool act = false, done = false;
	int64_t k = 0;
	uint32_t l = 0;
	unsigned long long steps = 0;
	for (;;) {
		while (!act && !done) { // (the same in the eight lanes of an octet)
			const int64_t w = walk_take(ctr, j);
			if (w >= nsp) { done = true; break; }
			const unsigned long long x = lnk[w].x, s = x & ~RB3_SSA_END;
			if (!(x & RB3_SSA_END) || s >= (unsigned long long)m) { if (j == 0) atomicAdd(ctr + 2, 1ull); continue; }
			if (!flag[s]) continue;
			k = w < m ? w : m + ((w - m) << S), l = 0;
			act = (uint64_t)k < (uint64_t)ix.n;
		}
		if (__ballot(act) == 0ull) break;
		if (act && j == 0) mark_row(bm, k);
		int c;
		const int64_t k2 = oct_lf_self(ix, act ? k : 0, j, &c);
		if (act) {
			++steps, ++l;
			const bool at_split = c != 0 && ((k2 - m) & maskS) == 0; // (k2 >= m whenever c != 0)
			if (c == 0 || at_split) act = false;
			else if (l >= (1u << RB3_SSA_LBITS) - 1u) { if (j == 0) atomicAdd(ctr + 2, 1ull); act = false; }
			k = k2;
		}
	}
	if (j == 0 && steps) atomicAdd(ctr + 1, steps);
}

/* one block per group g < ngo of the index: cnt[g] = its marked rows; letters[c] += the marked rows whose symbol is c (c < 6; letters[6]: symbols that are none).
 * bm holds ngo * 256 words; no bit behind row ix.n - 1 is ever set. */
__global__ void __launch_bounds__(256) k_mark_count(IdxView ix, const uint32_t *bm, uint32_t *cnt, unsigned long long *letters)
{
	__shared__ uint32_t s_tot, s_let[8];
	const int t = threadIdx.x;
	const int64_t g = blockIdx.x;
	if (t < 8) s_let[t] = 0u;
	if (t == 0) s_tot = 0u;
	__syncthreads();
	uint32_t x = bm[g * RB3_RM_WORDS + t];
	if (x) atomicAdd(&s_tot, (uint32_t)__popc(x));
	while (x) {
		const int b = __ffs((int)x) - 1;
		x &= x - 1u;
		const int64_t row = (g << RB3_GRP_BITS) + t * 32 + b;
		if (row < ix.n) atomicAdd(&s_let[idx_sym(ix, row) & 7u], 1u);
	}
	__syncthreads();
	if (t == 0) cnt[g] = s_tot;
	if (t < 6 && s_let[t]) atomicAdd(letters + t, (unsigned long long)s_let[t]);
	if (t == 6 && s_let[6] + s_let[7]) atomicAdd(letters + 6, (unsigned long long)(s_let[6] + s_let[7]));
}

/* one block per group g0 + blockIdx.x of the OLD index ix: pre[g] = the marked rows in front of group g.  A row i that is not marked has i - (marked rows in
 * front of it) rows kept in front of it: its new position.  Those inside [p0, p1) get their symbol written to out[position - p0]; the others are somebody
 * else's (the driver sends whole groups that cover the range). */
__global__ void __launch_bounds__(256) k_rm_compact(IdxView ix, const uint32_t *bm, const int64_t *pre, int64_t g0, int64_t p0, int64_t p1, uint8_t *out)
{
	__shared__ uint32_t s_w[RB3_RM_WORDS], s_p[RB3_RM_WORDS];
	const int t = threadIdx.x;
	const int64_t g = g0 + blockIdx.x;
	const uint32_t w = bm[g * RB3_RM_WORDS + t], pc = (uint32_t)__popc(w);
	s_w[t] = w, s_p[t] = pc;
	__syncthreads();
	for (int d = 1; d < RB3_RM_WORDS; d <<= 1) { // inclusive scan of the words' counts
		const uint32_t v = t >= d ? s_p[t - d] : 0u;
		__syncthreads();
		s_p[t] += v;
		__syncthreads();
	}
	const int64_t base = (g << RB3_GRP_BITS) - pre[g] - p0; // the new position of the group's first row, from p0, if nothing in the group were marked
	if (base >= p1 - p0 || base + RB3_GRP - (int64_t)s_p[RB3_RM_WORDS - 1] <= 0) return; // (no row of this group lands in the range; the same in all threads)
	for (int it = 0; it < RB3_GRP / 256; ++it) {
		const int o = it * 256 + t, wi = o >> 5, bit = o & 31;
		const int64_t row = (g << RB3_GRP_BITS) + o;
		if (row >= ix.n) break;
		const uint32_t ww = s_w[wi];
		if ((ww >> bit) & 1u) continue;
		const uint32_t mb = s_p[wi] - (uint32_t)__popc(ww) + (uint32_t)__popc(ww & ((1u << bit) - 1u));
		const int64_t d = base + o - (int64_t)mb;
		if (d >= 0 && d < p1 - p0) out[d] = (uint8_t)idx_sym(ix, row);
	}
}

#endif
