/*
 * rb3gpu_hapdiv.h -- the end-to-end BWA-SW dynamic program of a window against the index (`hapdiv`; the reference's sw_core on a linear
 * chain of nodes, bwa-sw.c:329-526, with the length-only backtrack of bwa-sw.c:76-114 and the summary of bwa-sw.c:218-253).
 *
 * A WAVE per window (a block is one wave), windows handed out by a grid stride.  Row i aligns the last i symbols of the window; a cell is
 * a bidirectional interval with the scores H, E, F.  Per row:
 *   1. the backward extensions of the up to N cells of the row before, an octet per cell, eight at a time: one rank pair and the six
 *      symbols decoded at both ends each (as k_mem_walk does it), the five intervals of every cell left in `ext`;
 *   2. lane 0 merges the candidates into the table IN THE REFERENCE'S ORDER: the table is an open-addressing set keyed by (lo, hi) whose
 *      slot numbers decide ties, so its hash, probing, growth at 3/4 load (the in-place re-placement that sends displaced entries on)
 *      and the capacity kept from row to row are restated here slot by slot;
 *   3. the N cells of the largest (H, slot): N rounds of a wave-wide maximum below the one before (keys are distinct);
 *   4. the F phase, from row 2 on: a stack, first the row's cells best first, of cells whose gap extension beats the N-th best score;
 *      every pop is one extension (octet 0) and up to five merges; then step 3 again if anything was accepted, and the F parents,
 *      recorded as intervals, are resolved to columns;
 *   5. twelve bytes per cell of the row go to the backtrack matrix in global memory: where H and E came from, the F column, the flags
 *      and whether the cell's base differs from the window's symbol.
 * After the last row: cells contained in a better-ranked one on either strand are dropped, and every lane walks one surviving cell
 * back to the root counting mismatches and gap symbols.
 *
 * The table lives in LDS up to `lds_slots` slots and moves to the block's table in global memory when it outgrows them (or starts
 * there); rows, extensions and the score heap live in LDS up to HD_LDS_N cells and in global memory beyond.  Whatever cannot be
 * represented -- a table, stack or parent list beyond its capacity, a backtrack that leaves the matrix or needs an F column that
 * was not kept (the reference stops on an assertion there) -- raises ctr[2], and the call fails.
 */
#ifndef RB3GPU_HAPDIV_H
#define RB3GPU_HAPDIV_H

#include "rb3gpu_mem.h"

#define HD_LDS_SLOTS 256          // slots of the table in LDS (14 KB)
#define HD_LDS_N 32               // cells of a row held in LDS
#define HD_NONE 0xFFFFFFFFu
#define HD_UNSET 0x3FFFFFFu
#define HD_PAYLOAD 0x3Fu          // H_from (2 bits), E_from, F_from, F column known, dropped
#define HD_FSET 16u
#define HD_FLT 32u
#define HD_USED_A (1u << 30)      // the occupancy bit of a slot alternates with every growth: the old table's bits die as its entries move
#define HD_USED_B (1u << 31)

struct HdCell { int64_t lo, hi, lo_rc; int32_t H, E, F; uint32_t H_pos, E_pos, fpar, fl, pad; };   // 56 bytes
struct HdExt { int64_t lo, hi, rc; };
struct HdZ { int64_t lo, hi, lo_rc; int32_t H, F; };
struct HdOpt { int32_t N, min_sc, ma, mi, go, ge, drop, k; };
struct HdWs {                     // per block: block b uses [b * stride, (b + 1) * stride) of each
	uint32_t *bt; int64_t bt_stride;      // 3 words per cell of (k + 1) * N
	HdCell *tab; int64_t tab_cap;         // slots (a power of two)
	HdCell *row;                          // N
	HdExt *ext;                           // 5 N
	int32_t *heap;                        // N
	HdZ *stack; int64_t stack_cap;
	int64_t *fpar; int64_t fpar_cap;      // pairs
};
struct HdTab { HdCell *t; int32_t bits, count, tier; uint32_t ub; };

__device__ __forceinline__ uint32_t hd_mix(uint64_t x)
{
	x ^= x >> 30, x *= 0xbf58476d1ce4e5b9ull;
	x ^= x >> 27, x *= 0x94d049bb133111ebull;
	x ^= x >> 31;
	return (uint32_t)x;
}

__device__ __forceinline__ uint32_t hd_home(int64_t lo, int64_t hi, int bits)
{
	return ((hd_mix((uint64_t)lo) + hd_mix((uint64_t)hi)) * 2654435769u) >> (32 - bits);
}

/* twice the slots: every old entry in slot order to its new place; an entry of the old table found there takes its turn next */
__device__ static bool hd_grow(HdTab &T, HdCell *gtab, int64_t gcap, int lds_slots)
{
	const uint32_t old_n = 1u << T.bits, new_n = old_n * 2, nmask = new_n - 1;
	if (T.tier == 0 && new_n > (uint32_t)lds_slots) {
		if ((int64_t)new_n > gcap) return false;
		for (uint32_t s = 0; s < old_n; ++s) gtab[s] = T.t[s];
		T.t = gtab, T.tier = 1;
	} else if (T.tier == 1 && (int64_t)new_n > gcap) return false;
	HdCell *t = T.t;
	for (uint32_t s = old_n; s < new_n; ++s) t[s].fl = 0;
	const uint32_t ob = T.ub, nb = ob == HD_USED_A ? HD_USED_B : HD_USED_A;
	for (uint32_t j = 0; j < old_n; ++j) {
		if (!(t[j].fl & ob)) continue;
		HdCell cur = t[j];
		t[j].fl = 0;
		cur.fl &= HD_PAYLOAD;
		for (;;) {
			uint32_t i = hd_home(cur.lo, cur.hi, T.bits + 1);
			while (t[i].fl & nb) i = (i + 1) & nmask;
			if (i < old_n && (t[i].fl & ob)) {
				HdCell tmp = t[i];
				t[i] = cur, t[i].fl = cur.fl | nb;
				cur = tmp, cur.fl &= HD_PAYLOAD;
			} else {
				t[i] = cur, t[i].fl = cur.fl | nb;
				break;
			}
		}
	}
	T.bits += 1, T.ub = nb;
	return true;
}

/* the candidate into the table; strict comparisons, so the first of two equal arrivals stays.  changed: H = 1, E = 2, F = 4.  NULL: no room */
__device__ static HdCell *hd_merge(HdTab &T, const HdCell &c, int &changed, HdCell *gtab, int64_t gcap, int lds_slots)
{
	uint32_t n = 1u << T.bits;
	changed = 0;
	if ((uint32_t)T.count >= (n >> 1) + (n >> 2)) {
		if (!hd_grow(T, gtab, gcap, lds_slots)) return nullptr;
		n = 1u << T.bits;
	}
	HdCell *t = T.t;
	uint32_t i = hd_home(c.lo, c.hi, T.bits);
	while ((t[i].fl & T.ub) && !(t[i].lo == c.lo && t[i].hi == c.hi)) i = (i + 1) & (n - 1);
	HdCell *q = t + i;
	if (!(q->fl & T.ub)) {
		*q = c, q->fl = (c.fl & HD_PAYLOAD) | T.ub;
		++T.count, changed = 7;
		return q;
	}
	if (q->pad < c.pad) q->pad = c.pad; // (the symbols of the query consumed, where the caller counts them there: rb3gpu_swlocal.h; 0 otherwise)
	if (q->E < c.E) q->E = c.E, q->E_pos = c.E_pos, q->fl = (q->fl & ~4u) | (c.fl & 4u), changed |= 2;
	if (q->F < c.F) q->F = c.F, q->fl = (q->fl & ~8u) | (c.fl & 8u), changed |= 4;
	if (q->H < c.H) {
		q->H = c.H, q->fl = (q->fl & ~3u) | (c.fl & 3u), changed |= 1;
		if ((c.fl & 3u) == 0) q->H_pos = c.H_pos;
	}
	return q;
}

__device__ __forceinline__ int64_t hd_shfl64(int64_t v, int src)
{
	const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), src);
	return (int64_t)((uint64_t)hi << 32 | lo);
}

/* the backward extension of (lo, lo + size, lo_rc) by every symbol, by the octet of lane j: e[c - 1] for c = 1..5, the same in its eight lanes */
__device__ __forceinline__ void hd_extend(const IdxView &ix, int64_t lo, int64_t hi, int64_t lo_rc, int j, HdExt e[5])
{
	RankLoad rl, ru;
	oct_rank_issue(ix, lo, j, rl);
	oct_rank_issue(ix, hi, j, ru);
	int64_t l[6], s[6];
#pragma unroll
	for (int c = 0; c < 6; ++c) {
		l[c] = oct_rank_finish(rl, c, j, ix.abs);
		s[c] = oct_rank_finish(ru, c, j, ix.abs) - l[c];
	}
	int64_t at = lo_rc + s[0]; // the other strand's order: $ T G C A N
	e[3].rc = at, at += s[4];
	e[2].rc = at, at += s[3];
	e[1].rc = at, at += s[2];
	e[0].rc = at, at += s[1];
	e[4].rc = at;
#pragma unroll
	for (int c = 1; c < 6; ++c) e[c - 1].lo = l[c], e[c - 1].hi = l[c] + s[c];
}

/* the n = min(count, N) cells of the largest (H, slot) into row, largest first (all lanes; returns n in every lane) */
__device__ static int hd_top(const HdCell *t, uint32_t cap, uint32_t ub, int N, HdCell *row, int lane)
{
	unsigned long long prev = ~0ull;
	int n = 0;
	for (; n < N; ++n) {
		unsigned long long best = 0;
		for (uint32_t s = lane; s < cap; s += 64) {
			if (!(t[s].fl & ub)) continue;
			const unsigned long long key = (unsigned long long)(uint32_t)t[s].H << 32 | s;
			if (key < prev && key > best) best = key;
		}
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			const uint32_t ol = (uint32_t)__shfl_xor((int)(uint32_t)best, d), oh = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), d);
			const unsigned long long o = (unsigned long long)oh << 32 | ol;
			best = o > best ? o : best;
		}
		if (best == 0) break;
		if (lane == 0) {
			row[n] = t[(uint32_t)best];
			row[n].fl &= HD_PAYLOAD;
		}
		prev = best;
	}
	return n;
}

__device__ __forceinline__ void hd_heap_put(int32_t *heap, int &sz, int N, int32_t v) // a min-heap of the N largest scores
{
	if (sz < N) {
		int i = sz++;
		while (i > 0 && heap[(i - 1) >> 1] > v) heap[i] = heap[(i - 1) >> 1], i = (i - 1) >> 1;
		heap[i] = v;
	} else if (v > heap[0]) {
		int i = 0;
		for (;;) {
			int c = 2 * i + 1;
			if (c >= sz) break;
			if (c + 1 < sz && heap[c + 1] < heap[c]) ++c;
			if (heap[c] >= v) break;
			heap[i] = heap[c], i = c;
		}
		heap[i] = v;
	}
}

/* The rows of one query q[0, k) (steps 1-5 of the header comment) and the marking of the contained cells of the last row: the part that
 * `hapdiv` and `sw -e` share.  Mismatches, gaps of the index side and the F phase start at row end_len + 1 (every cell of row i has
 * consumed i symbols, its parent i - 1: the reference's tests on qlen, bwa-sw.c:405, 417, 445, all read i - 1 >= end_len); `hapdiv` has
 * end_len 1.  BASES: bits 5-7 of a cell's third word hold its base (1..5) instead of "differs from the query", for a backtrack that
 * writes the alignment out.  All lanes of the one wave call it; returns the cells of the last row (0: the alignment does not reach the
 * end, or -- done == false -- something could not be represented); best_sc: the best score of any row; the dedup ran if both allow it */
struct HdLds { HdCell *tab; HdTab *T; int32_t *err; };

template<bool BASES>
__device__ static int hd_rows(const IdxView &ix, const Acc7 &acc, const uint8_t *q, int k, int end_len, const HdOpt &o, const HdWs &ws, HdCell *gtab, HdCell *row, HdExt *ext,
		int32_t *heap, HdZ *stack, int64_t *fpar, uint32_t *bt, const HdLds &L, int lds_slots, int bits0, unsigned long long &n_ext, int &best_sc, bool &done)
{
	const int lane = threadIdx.x, j = lane & 7, oct = lane >> 3;
	const int N = o.N;
	HdCell *const s_tab = L.tab;
	HdTab &s_T = *L.T;
	int32_t &s_err = *L.err;
	__syncthreads();
	if (lane == 0) {
		HdTab T;
		T.bits = bits0, T.count = 0, T.ub = HD_USED_A;
		T.tier = (1 << bits0) > lds_slots ? 1 : 0;
		T.t = T.tier ? gtab : s_tab;
		s_T = T, s_err = 0;
		HdCell r;
		r.lo = 0, r.hi = acc.a[6], r.lo_rc = 0, r.H = r.E = r.F = 0, r.H_pos = r.E_pos = HD_NONE, r.fpar = HD_UNSET, r.fl = 0, r.pad = 0;
		row[0] = r;
	}
	if (lane < 3) bt[lane] = lane < 2 ? HD_NONE : 0u;
	__syncthreads();
	int n = 1;
	best_sc = 0, done = true;
	for (int i = 1; i <= k; ++i) {
		const int cq = min((int)q[k - i], 5);
		const bool inner = i > end_len;
		{ // an empty table of the capacity it has grown to
			HdCell *t = s_T.t;
			const uint32_t cap = 1u << s_T.bits;
			for (uint32_t s = lane; s < cap; s += 64) t[s].fl = 0;
		}
		for (int c0 = 0; c0 < n; c0 += 8) { // 1. the extensions of the row before
			const int col = c0 + oct;
			const bool act = col < n;
			const int64_t lo = act ? row[col].lo : 0, hi = act ? row[col].hi : 0, rc = act ? row[col].lo_rc : 0;
			HdExt e[5];
			hd_extend(ix, lo, hi, rc, j, e);
			if (act && j < 5) {
				HdExt v = e[0];
#pragma unroll
				for (int c = 1; c < 5; ++c) v = j == c ? e[c] : v;
				ext[col * 5 + j] = v;
			}
		}
		__syncthreads();
		if (lane == 0) { // 2. the candidates in the reference's order
			HdTab T = s_T;
			T.count = 0;
			bool ok = true;
			int ch;
			for (int col = 0; col < n && ok; ++col) {
				const HdCell p = row[col];
				const uint32_t pos = (uint32_t)(i - 1) * (uint32_t)N + (uint32_t)col;
				int64_t last_rc = 0;
				HdCell r;
				r.E = r.F = 0, r.H_pos = pos, r.E_pos = HD_NONE, r.fpar = HD_UNSET, r.fl = 0, r.pad = 0;
				for (int c = 1; c < 6 && ok; ++c) {
					const HdExt e = ext[col * 5 + c - 1];
					const int sc = c == cq && c != 5 ? o.ma : -o.mi;
					if (e.hi == e.lo || p.H + sc <= 0 || (c != cq && !inner)) continue;
					last_rc = e.rc;
					r.lo = e.lo, r.hi = e.hi, r.lo_rc = e.rc, r.H = p.H + sc;
					ok = hd_merge(T, r, ch, gtab, ws.tab_cap, lds_slots) != nullptr;
				}
				int32_t ev = p.H - o.go > p.E ? p.H - o.go : p.E;
				const uint32_t ef = p.H - o.go > p.E ? 0u : 4u;
				ev -= o.ge;
				if (ev > 0 && inner && ok) { // (the other strand's start of the gap cell: that of the last candidate made above, as in the reference)
					r.lo = p.lo, r.hi = p.hi, r.lo_rc = last_rc, r.H = r.E = ev, r.F = 0, r.H_pos = HD_NONE, r.E_pos = pos, r.fl = 1u | ef;
					ok = hd_merge(T, r, ch, gtab, ws.tab_cap, lds_slots) != nullptr;
				}
			}
			n_ext += n;
			if (!ok) s_err = 1;
			s_T = T;
		}
		__syncthreads();
		if (s_err) { done = false; break; }
		if (s_T.count == 0) { n = 0; break; }
		n = hd_top(s_T.t, 1u << s_T.bits, s_T.ub, N, row, lane); // 3.
		__syncthreads();
		int n_fpar = 0;
		if (inner) { // 4. the F phase
			HdTab T = s_T; // (used by lane 0)
			int hsz = 0, next = 0, sp = 0;
			bool ok = true;
			if (lane == 0) for (int t = n - 1; t >= 0; --t) hd_heap_put(heap, hsz, N, row[t].H);
			for (;;) {
				HdZ z = {0, 0, 0, 0, 0};
				int32_t f = 0, low = 0;
				uint32_t ff = 0;
				int go_on = 0;
				if (lane == 0) {
					while (ok) { // the next cell of the stack whose gap extension beats the N-th best score
						if (sp > 0) z = stack[--sp];
						else if (next < n) {
							const HdCell c = row[next++];
							if (c.H <= o.go + o.ge) continue;
							z.lo = c.lo, z.hi = c.hi, z.lo_rc = c.lo_rc, z.H = c.H, z.F = c.F;
						} else break;
						low = hsz < N ? 0 : heap[0];
						f = z.H - o.go > z.F ? z.H - o.go : z.F;
						ff = z.H - o.go > z.F ? 0u : 8u;
						f -= o.ge;
						if (f > low) { go_on = 1; break; }
					}
				}
				go_on = __shfl(go_on, 0);
				if (!go_on) break;
				const int64_t zlo = hd_shfl64(z.lo, 0), zhi = hd_shfl64(z.hi, 0), zrc = hd_shfl64(z.lo_rc, 0);
				HdExt e[5];
				hd_extend(ix, zlo, zhi, zrc, j, e);
				if (lane == 0) {
					++n_ext;
					for (int c = 0; c < 5 && ok; ++c) {
						if (e[c].hi == e[c].lo) continue;
						HdCell r;
						r.lo = e[c].lo, r.hi = e[c].hi, r.lo_rc = e[c].rc, r.H = r.F = f, r.E = 0, r.H_pos = r.E_pos = HD_NONE, r.fpar = HD_UNSET, r.fl = 2u | ff, r.pad = 0;
						int ch;
						HdCell *qc = hd_merge(T, r, ch, gtab, ws.tab_cap, lds_slots);
						if (qc == nullptr) { ok = false; break; }
						if (!(ch & 4)) continue;
						hd_heap_put(heap, hsz, N, f);
						if (n_fpar >= ws.fpar_cap || n_fpar >= (int)HD_UNSET) { ok = false; break; }
						fpar[2 * n_fpar] = z.lo, fpar[2 * n_fpar + 1] = z.hi;
						qc->fl = (qc->fl & ~8u) | ff, qc->fpar = (uint32_t)n_fpar++;
						if (f - o.ge > low) {
							if (sp >= ws.stack_cap) { ok = false; break; }
							HdZ y;
							y.lo = qc->lo, y.hi = qc->hi, y.lo_rc = qc->lo_rc, y.H = qc->H, y.F = qc->F;
							stack[sp++] = y;
						}
					}
				}
			}
			if (lane == 0) {
				s_T = T;
				if (!ok) s_err = 1;
			}
			n_fpar = __shfl(n_fpar, 0);
			__syncthreads();
			if (s_err) { done = false; break; }
			if (n_fpar > 0) {
				n = hd_top(s_T.t, 1u << s_T.bits, s_T.ub, N, row, lane);
				__syncthreads();
				for (int c = lane; c < n; c += 64) { // the F parents: from intervals to columns of the row; a parent that fell out leaves F unset
					if (row[c].F == 0 || row[c].fpar == HD_UNSET) continue;
					const int64_t plo = fpar[2 * row[c].fpar], phi = fpar[2 * row[c].fpar + 1];
					int at = -1;
					for (int d = 0; d < n && at < 0; ++d)
						if (row[d].lo == plo && row[d].hi == phi) at = d;
					if (at >= 0) row[c].fpar = (uint32_t)at, row[c].fl |= HD_FSET;
					else row[c].fpar = HD_UNSET;
				}
				__syncthreads();
			}
		}
		best_sc = max(best_sc, row[0].H);
		for (int c = lane; c < n; c += 64) { // 5. what the backtrack needs
			const HdCell x = row[c];
			int base = 0;
#pragma unroll
			for (int a = 1; a < 6; ++a) base = acc.a[a] <= x.lo ? a : base;
			const uint32_t m = (x.fl & 15u) | (x.F != 0 && (x.fl & HD_FSET) ? 16u : 0u) | (BASES ? (uint32_t)base << 5 : base != cq ? 32u : 0u) | (x.fpar & 0xFFFFFFu) << 8;
			uint32_t *d = bt + ((size_t)i * N + c) * 3;
			d[0] = x.H_pos, d[1] = x.E_pos, d[2] = m;
		}
		__syncthreads();
	}
	if (done && n > 0 && best_sc >= o.min_sc) {
		if (lane == 0) { // cells contained, on either strand, in a cell ranked before them that was kept
			for (int c = 1; c < n; ++c) {
				const HdCell p = row[c];
				bool in = false;
				for (int d = 0; d < c && !in; ++d) {
					const HdCell x = row[d];
					if (x.fl & HD_FLT) continue;
					in = (x.lo_rc <= p.lo_rc && x.lo_rc + (x.hi - x.lo) >= p.lo_rc + (p.hi - p.lo)) || (x.lo <= p.lo && x.hi >= p.hi);
				}
				if (in) row[c].fl |= HD_FLT;
			}
		}
		__syncthreads();
	}
	return n;
}

/* windows [w0, w1): window w is sym[win_off[w], win_off[w] + k); out: 9 numbers per window of the slice.
 * ctr[0] += extensions, ctr[1] += windows whose table went to global memory, ctr[2] != 0: something could not be represented */
__global__ void __launch_bounds__(64) k_hapdiv(IdxView ix, Acc7 acc, const uint8_t *sym, const int64_t *win_off, int64_t w0, int64_t w1, HdOpt o, HdWs ws,
		int lds_slots, int32_t *out, unsigned long long *ctr)
{
	__shared__ HdCell s_tab[HD_LDS_SLOTS];
	__shared__ HdCell s_row[HD_LDS_N];
	__shared__ HdExt s_ext[HD_LDS_N * 5];
	__shared__ int32_t s_heap[HD_LDS_N];
	__shared__ HdTab s_T;
	__shared__ int32_t s_res[9];
	__shared__ int32_t s_err;
	const int lane = threadIdx.x;
	const int N = o.N, k = o.k;
	const int64_t b = blockIdx.x;
	uint32_t *bt = ws.bt + b * ws.bt_stride;
	HdCell *gtab = ws.tab + b * ws.tab_cap;
	const bool small = N <= HD_LDS_N;
	HdCell *row = small ? s_row : ws.row + b * N;
	HdExt *ext = small ? s_ext : ws.ext + b * 5 * N;
	int32_t *heap = small ? s_heap : ws.heap + b * N;
	HdZ *stack = ws.stack + b * ws.stack_cap;
	int64_t *fpar = ws.fpar + b * 2 * ws.fpar_cap;
	const uint32_t total = (uint32_t)(k + 1) * (uint32_t)N;
	int bits0 = 2;
	while ((1 << bits0) < 4 * N) ++bits0;
	unsigned long long n_ext = 0, n_t2 = 0;
	const HdLds L = { s_tab, &s_T, &s_err };

	for (int64_t w = w0 + b; w < w1; w += gridDim.x) {
		const uint8_t *q = sym + win_off[w];
		if (lane < 9) s_res[lane] = 0;
		int best_sc = 0;
		bool done = true;
		const int n = hd_rows<false>(ix, acc, q, k, 1, o, ws, gtab, row, ext, heap, stack, fpar, bt, L, lds_slots, bits0, n_ext, best_sc, done);
		if (done && n > 0 && best_sc >= o.min_sc) {
			const int32_t h0 = row[0].H;
			const uint32_t limit = (uint32_t)(k + 1) * ((uint32_t)min(N, 1 << 20) + 1u);
			for (int c = lane; c < n; c += 64) {
				const HdCell x = row[c];
				if ((x.fl & HD_FLT) || (x.fl & 3u) != 0 || x.H < o.min_sc || (o.drop >= 0 && h0 - x.H > o.drop)) continue;
				uint32_t pos = (uint32_t)k * (uint32_t)N + (uint32_t)c, steps = 0;
				int last = 0, ed = 0;
				bool bad = false;
				while (pos > 0 && !bad) {
					if (pos >= total || ++steps > limit) { bad = true; break; }
					const uint32_t r = pos / (uint32_t)N, m = bt[(size_t)pos * 3 + 2];
					const int state = last == 0 ? (int)(m & 3u) : last;
					const int gext = state == 1 ? (int)(m >> 2 & 1u) : state == 2 ? (int)(m >> 3 & 1u) : 0;
					uint32_t np = 0;
					if (state == 0) np = bt[(size_t)pos * 3], ed += (int)(m >> 5 & 1u), bad = np >= r * (uint32_t)N;
					else if (state == 1) np = bt[(size_t)pos * 3 + 1], ++ed, bad = np >= r * (uint32_t)N;
					else if (state == 2 && (m & 16u)) np = r * (uint32_t)N + (m >> 8), ++ed;
					else bad = true;
					pos = np, last = gext ? state : 0;
				}
				if (bad) { atomicOr(&s_err, 1); continue; }
				atomicAdd(&s_res[0], 1);
				atomicMax(&s_res[1], ed);
				atomicAdd(&s_res[2 + min(ed, 6)], (int32_t)(uint32_t)(uint64_t)(x.hi - x.lo));
			}
		}
		__syncthreads();
		if (lane < 9) out[(w - w0) * 9 + lane] = s_res[lane];
		if (lane == 0) {
			if (s_T.tier) ++n_t2;
			if (s_err || !done) atomicAdd(ctr + 2, 1ull);
		}
	}
	if (lane == 0) {
		if (n_ext) atomicAdd(ctr, n_ext);
		if (n_t2) atomicAdd(ctr + 1, n_t2);
	}
}

#endif
