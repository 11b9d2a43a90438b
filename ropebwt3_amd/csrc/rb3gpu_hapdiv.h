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
 * Steps 1, 2, 4 and 5, the table's set-up per query and its reset per row are device functions of their own (hd_stage_ext, hd_cands,
 * hd_fphase, hd_store_bt, hd_tab_init, hd_tab_clear): hd_rows below is the loop over them for a linear query (`hapdiv`, and `sw -e` of
 * rb3gpu_sw.h), and the node loop of `sw --local` (rb3gpu_swlocal.h) calls the same functions with a predecessor list per row.  The
 * caller says where the predecessor row's cells are numbered from, what max_min_sc is, and who knows the symbols of the query a cell has
 * consumed, by which mismatches, gaps and the F phase are allowed (end_len): the row, or -- QLEN -- every cell for itself (HdCell.pad).
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

struct HdCell { int64_t lo, hi, lo_rc; int32_t H, E, F; uint32_t H_pos, E_pos, fpar, fl, pad; };   // 56 bytes; pad: the symbols of the query consumed, where cells count them (QLEN)
struct HdExt { int64_t lo, hi, rc; };
struct HdZ { int64_t lo, hi, lo_rc; int32_t H, F, qlen, fill; };   // 40 bytes; qlen: the pad of the cell
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
/* what the one wave of a block works with: its arrays (LDS, or its part of HdWs), the capacities of those in global memory, and what lane 0
 * leaves in LDS for the wave: the table's state and the error flag */
struct HdBlk {
	HdCell *s_tab, *gtab, *row; HdExt *ext; int32_t *heap; HdZ *stack; int64_t *fpar;
	int64_t tab_cap, stack_cap, fpar_cap;
	HdTab *T; int32_t *err;
	int lds_slots, bits0;
};

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
	if (q->pad < c.pad) q->pad = c.pad; // (the symbols of the query consumed, where cells count them: the larger stays; both are 0 where the row says it)
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

/* ---- the row step: what a row of the linear program (hd_rows) and a node of the graph (k_swl_fill of rb3gpu_swlocal.h) both do, once each ---- */

/* the block's arrays: rows, extensions and heap in LDS up to HD_LDS_N cells, everything else in block b's part of ws */
__device__ __forceinline__ HdBlk hd_blk(const HdWs &ws, int64_t b, int N, int lds_slots, HdCell *s_tab, HdCell *s_row, HdExt *s_ext, int32_t *s_heap, HdTab *T, int32_t *err)
{
	const bool small = N <= HD_LDS_N;
	HdBlk B;
	B.s_tab = s_tab, B.gtab = ws.tab + b * ws.tab_cap;
	B.row = small ? s_row : ws.row + b * N;
	B.ext = small ? s_ext : ws.ext + b * 5 * N;
	B.heap = small ? s_heap : ws.heap + b * N;
	B.stack = ws.stack + b * ws.stack_cap;
	B.fpar = ws.fpar + b * 2 * ws.fpar_cap;
	B.tab_cap = ws.tab_cap, B.stack_cap = ws.stack_cap, B.fpar_cap = ws.fpar_cap;
	B.T = T, B.err = err;
	B.lds_slots = lds_slots, B.bits0 = 2;
	while ((1 << B.bits0) < 4 * N) ++B.bits0;
	return B;
}

/* lane 0, once per query: an empty table of its first capacity, in LDS if that fits, and no error */
__device__ __forceinline__ void hd_tab_init(const HdBlk &B)
{
	HdTab T;
	T.bits = B.bits0, T.count = 0, T.ub = HD_USED_A;
	T.tier = (1 << B.bits0) > B.lds_slots ? 1 : 0;
	T.t = T.tier ? B.gtab : B.s_tab;
	*B.T = T, *B.err = 0;
}

/* the cell every query starts from: all rows of the index, nothing consumed */
__device__ __forceinline__ HdCell hd_root(const Acc7 &acc)
{
	HdCell r;
	r.lo = 0, r.hi = acc.a[6], r.lo_rc = 0, r.H = r.E = r.F = 0, r.H_pos = r.E_pos = HD_NONE, r.fpar = HD_UNSET, r.fl = 0, r.pad = 0;
	return r;
}

/* all lanes, once per row: an empty table of the capacity it has grown to */
__device__ __forceinline__ void hd_tab_clear(const HdBlk &B, int lane)
{
	HdCell *t = B.T->t;
	const uint32_t cap = 1u << B.T->bits;
	for (uint32_t s = lane; s < cap; s += 64) t[s].fl = 0;
	if (lane == 0) B.T->count = 0;
}

/* all lanes: the backward extensions of the n cells in row, an octet per cell, eight cells at a time, to ext[col * 5 + c - 1] */
__device__ __forceinline__ void hd_stage_ext(const IdxView &ix, const HdBlk &B, int n, int lane)
{
	const int j = lane & 7, oct = lane >> 3;
	for (int c0 = 0; c0 < n; c0 += 8) {
		const int col = c0 + oct;
		const bool act = col < n;
		const int64_t lo = act ? B.row[col].lo : 0, hi = act ? B.row[col].hi : 0, rc = act ? B.row[col].lo_rc : 0;
		HdExt e[5];
		hd_extend(ix, lo, hi, rc, j, e);
		if (act && j < 5) {
			HdExt v = e[0];
#pragma unroll
			for (int c = 1; c < 5; ++c) v = j == c ? e[c] : v;
			B.ext[col * 5 + j] = v;
		}
	}
}

/* lane 0: the candidates of the n staged cells of a predecessor row into the table, in the reference's order (bwa-sw.c:398-431): per cell the five
 * symbols, then the gap of the query side.  pos0: the number of the predecessor's first cell in the backtrack matrix; cq: the symbol of this row.
 * A mismatch and a gap need a cell that has consumed end_len symbols (bwa-sw.c:405, 417).  mm is the reference's max_min_sc: a cell that cannot
 * reach it even by a match, and a candidate below it, are passed over.  A linear query has one predecessor per row and passes 0, where the three
 * tests on mm say nothing new: a kept cell has H >= 0, so with a match score that is not negative p.H + ma < 0 never holds, and p.H + sc < 0 and
 * ev < 0 are cases of the p.H + sc <= 0 and ev <= 0 that are passed over anyway.
 * QLEN says who knows the symbols of the query a cell has consumed: the cell (pad; a candidate gets its parent's and one more), as the rows of a
 * graph need it, or the row, row_qlen for all n cells, pad staying 0.  Counting per cell on a linear query gives the same bytes, every cell of row
 * i - 1 having consumed i - 1, and was measured: the bookkeeping lies on lane 0's serial path and costs `hapdiv` and `sw -e` 1 % of their kernel
 * time (profiles/sw_share_ab.json), so it is a parameter at compile time.  Returns the symbols that the last cell visited, cut or not, has
 * consumed: the F phase of a row runs iff the last cell of its last predecessor has consumed end_len (bwa-sw.c:445) */
template<bool QLEN>
__device__ __forceinline__ int32_t hd_cands(const HdBlk &B, const HdOpt &o, int n, uint32_t pos0, int cq, int end_len, int32_t row_qlen, int32_t mm, unsigned long long &n_ext)
{
	HdTab T = *B.T;
	bool ok = true;
	int ch;
	int32_t lastq = 0;
	for (int col = 0; col < n && ok; ++col) {
		const HdCell p = B.row[col];
		lastq = QLEN ? (int32_t)p.pad : row_qlen;
		if (p.H + o.ma < mm) continue;
		const uint32_t pos = pos0 + (uint32_t)col;
		const bool inner = lastq >= end_len;
		int64_t last_rc = 0;
		HdCell r;
		r.E = r.F = 0, r.H_pos = pos, r.E_pos = HD_NONE, r.fpar = HD_UNSET, r.fl = 0, r.pad = QLEN ? p.pad + 1 : 0;
		for (int c = 1; c < 6 && ok; ++c) {
			const HdExt e = B.ext[col * 5 + c - 1];
			const int sc = c == cq && c != 5 ? o.ma : -o.mi;
			if (e.hi == e.lo || p.H + sc <= 0 || p.H + sc < mm || (c != cq && !inner)) continue;
			last_rc = e.rc;
			r.lo = e.lo, r.hi = e.hi, r.lo_rc = e.rc, r.H = p.H + sc;
			ok = hd_merge(T, r, ch, B.gtab, B.tab_cap, B.lds_slots) != nullptr;
		}
		int32_t ev = p.H - o.go > p.E ? p.H - o.go : p.E;
		const uint32_t ef = p.H - o.go > p.E ? 0u : 4u;
		ev -= o.ge;
		if (ev > 0 && ev >= mm && inner && ok) { // (the other strand's start of the gap cell: that of the last candidate made above, as in the reference)
			r.lo = p.lo, r.hi = p.hi, r.lo_rc = last_rc, r.H = r.E = ev, r.F = 0, r.H_pos = HD_NONE, r.E_pos = pos, r.fl = 1u | ef;
			ok = hd_merge(T, r, ch, B.gtab, B.tab_cap, B.lds_slots) != nullptr;
		}
	}
	n_ext += n;
	if (!ok) *B.err = 1;
	*B.T = T;
	return lastq;
}

/* all lanes: the F phase over the n selected cells of row (bwa-sw.c:445-493): a stack, first the row's cells best first, of cells whose gap extension
 * beats the N-th best score; every pop is one extension (octet 0) and up to five merges, a candidate inheriting the consumed symbols of the cell it
 * leaves (QLEN, as hd_cands); then the selection once more if anything was accepted, and the F parents, recorded as intervals, resolved to columns.  n: the cells of
 * row afterwards.  false: something could not be represented */
template<bool QLEN>
__device__ __forceinline__ bool hd_fphase(const IdxView &ix, const HdBlk &B, const HdOpt &o, int &n, unsigned long long &n_ext, int lane)
{
	const int N = o.N, j = lane & 7;
	HdCell *const row = B.row;
	int32_t *const heap = B.heap;
	HdTab T = *B.T; // (used by lane 0)
	int hsz = 0, next = 0, sp = 0, n_fpar = 0;
	bool ok = true;
	if (lane == 0) for (int t = n - 1; t >= 0; --t) hd_heap_put(heap, hsz, N, row[t].H);
	for (;;) {
		HdZ z = {0, 0, 0, 0, 0, 0, 0};
		int32_t f = 0, low = 0;
		uint32_t ff = 0;
		int go_on = 0;
		if (lane == 0) {
			while (ok) { // the next cell of the stack whose gap extension beats the N-th best score
				if (sp > 0) z = B.stack[--sp];
				else if (next < n) {
					const HdCell c = row[next++];
					if (c.H <= o.go + o.ge) continue;
					z.lo = c.lo, z.hi = c.hi, z.lo_rc = c.lo_rc, z.H = c.H, z.F = c.F, z.qlen = QLEN ? (int32_t)c.pad : 0;
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
				r.lo = e[c].lo, r.hi = e[c].hi, r.lo_rc = e[c].rc, r.H = r.F = f, r.E = 0, r.H_pos = r.E_pos = HD_NONE, r.fpar = HD_UNSET, r.fl = 2u | ff, r.pad = QLEN ? (uint32_t)z.qlen : 0;
				int ch;
				HdCell *qc = hd_merge(T, r, ch, B.gtab, B.tab_cap, B.lds_slots);
				if (qc == nullptr) { ok = false; break; }
				if (!(ch & 4)) continue;
				hd_heap_put(heap, hsz, N, f);
				if (n_fpar >= B.fpar_cap || n_fpar >= (int)HD_UNSET) { ok = false; break; }
				B.fpar[2 * n_fpar] = z.lo, B.fpar[2 * n_fpar + 1] = z.hi;
				qc->fl = (qc->fl & ~8u) | ff, qc->fpar = (uint32_t)n_fpar++;
				if (f - o.ge > low) {
					if (sp >= B.stack_cap) { ok = false; break; }
					HdZ y;
					y.lo = qc->lo, y.hi = qc->hi, y.lo_rc = qc->lo_rc, y.H = qc->H, y.F = qc->F, y.qlen = QLEN ? (int32_t)qc->pad : 0, y.fill = 0;
					B.stack[sp++] = y;
				}
			}
		}
	}
	if (lane == 0) {
		*B.T = T;
		if (!ok) *B.err = 1;
	}
	n_fpar = __shfl(n_fpar, 0);
	__syncthreads();
	if (*B.err) return false;
	if (n_fpar > 0) {
		n = hd_top(B.T->t, 1u << B.T->bits, B.T->ub, N, row, lane);
		__syncthreads();
		for (int c = lane; c < n; c += 64) { // the F parents: from intervals to columns of the row; a parent that fell out leaves F unset
			if (row[c].F == 0 || row[c].fpar == HD_UNSET) continue;
			const int64_t plo = B.fpar[2 * row[c].fpar], phi = B.fpar[2 * row[c].fpar + 1];
			int at = -1;
			for (int d = 0; d < n && at < 0; ++d)
				if (row[d].lo == plo && row[d].hi == phi) at = d;
			if (at >= 0) row[c].fpar = (uint32_t)at, row[c].fl |= HD_FSET;
			else row[c].fpar = HD_UNSET;
		}
		__syncthreads();
	}
	return true;
}

/* all lanes: what the backtrack needs of the n finished cells of row, twelve bytes a cell from d on: where H and E came from; the flags, the F column
 * and in bits 5-7 the cell's base (BASES: for a backtrack that writes the alignment out) or whether it differs from the row's symbol cq */
template<bool BASES>
__device__ __forceinline__ void hd_store_bt(const Acc7 &acc, const HdCell *row, int n, int cq, uint32_t *d, int lane)
{
	for (int c = lane; c < n; c += 64) {
		const HdCell x = row[c];
		int base = 0;
#pragma unroll
		for (int a = 1; a < 6; ++a) base = acc.a[a] <= x.lo ? a : base;
		const uint32_t m = (x.fl & 15u) | (x.F != 0 && (x.fl & HD_FSET) ? 16u : 0u) | (BASES ? (uint32_t)base << 5 : base != cq ? 32u : 0u) | (x.fpar & 0xFFFFFFu) << 8;
		d[c * 3] = x.H_pos, d[c * 3 + 1] = x.E_pos, d[c * 3 + 2] = m;
	}
}

/* The rows of one query q[0, k) (steps 1-5 of the header comment) and the marking of the contained cells of the last row: the part that
 * `hapdiv` and `sw -e` share.  Every cell of row i has consumed i symbols, its parent i - 1, so the reference's tests on qlen (bwa-sw.c:405,
 * 417, 445) all read i - 1 >= end_len here: mismatches, gaps of the index side and the F phase start at row end_len + 1; `hapdiv` has end_len 1.
 * All lanes of the one wave call it; returns the cells of the last row (0: the alignment does not reach the end, or -- done == false --
 * something could not be represented); best_sc: the best score of any row; the dedup ran if both allow it */
template<bool BASES>
__device__ static int hd_rows(const IdxView &ix, const Acc7 &acc, const uint8_t *q, int k, int end_len, const HdOpt &o, const HdBlk &B, uint32_t *bt,
		unsigned long long &n_ext, int &best_sc, bool &done)
{
	const int lane = threadIdx.x;
	const int N = o.N;
	HdCell *const row = B.row;
	__syncthreads();
	if (lane == 0) hd_tab_init(B), row[0] = hd_root(acc);
	if (lane < 3) bt[lane] = lane < 2 ? HD_NONE : 0u;
	__syncthreads();
	int n = 1;
	best_sc = 0, done = true;
	for (int i = 1; i <= k; ++i) {
		const int cq = min((int)q[k - i], 5);
		hd_tab_clear(B, lane);
		hd_stage_ext(ix, B, n, lane); // 1. the extensions of the row before
		__syncthreads();
		if (lane == 0) (void)hd_cands<false>(B, o, n, (uint32_t)(i - 1) * (uint32_t)N, cq, end_len, i - 1, 0, n_ext); // 2.
		__syncthreads();
		if (*B.err) { done = false; break; }
		if (B.T->count == 0) { n = 0; break; }
		n = hd_top(B.T->t, 1u << B.T->bits, B.T->ub, N, row, lane); // 3.
		__syncthreads();
		if (i > end_len && !hd_fphase<false>(ix, B, o, n, n_ext, lane)) { done = false; break; } // 4. (every cell of row i - 1 has consumed i - 1 symbols: what hd_cands returns)
		best_sc = max(best_sc, row[0].H);
		hd_store_bt<BASES>(acc, row, n, cq, bt + (size_t)i * N * 3, lane); // 5.
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
	const HdBlk B = hd_blk(ws, b, N, lds_slots, s_tab, s_row, s_ext, s_heap, &s_T, &s_err);
	const HdCell *row = B.row;
	const uint32_t total = (uint32_t)(k + 1) * (uint32_t)N;
	unsigned long long n_ext = 0, n_t2 = 0;

	for (int64_t w = w0 + b; w < w1; w += gridDim.x) {
		const uint8_t *q = sym + win_off[w];
		if (lane < 9) s_res[lane] = 0;
		int best_sc = 0;
		bool done = true;
		const int n = hd_rows<false>(ix, acc, q, k, 1, o, B, bt, n_ext, best_sc, done);
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
