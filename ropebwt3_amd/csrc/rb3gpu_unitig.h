/*
 * rb3gpu_unitig.h -- `unitig`: the unambiguous paths of the string graph, spelled (no counterpart in the reference).
 *
 * The kept records of `overlap --reduce` lie on the device (rec, keep, pos: rb3gpu_reduce.h).  The vertices are the strings.  A kept record (a, b, o) is SIMPLE iff it is the
 * only kept record out of a, the only one into b, and a != b; the simple records are next[a] = b, prev[b] = a, o_in[b] = o, and they form disjoint paths and cycles.  A
 * chain is a path from its head (no prev) to its tail (no next), or a cycle cut in front of its smallest row.
 *
 *   k_utg_degree   dout[a] += 1, din[b] += 1 per kept record.
 *   k_utg_simple   next, prev and o_in from the simple records: a simple record is the only writer of its two slots.
 *   k_utg_asym     with both strands: the vertices v with a next for which next[next[v] ^ 1] != v ^ 1.
 *   k_utg_init, k_utg_jump   list ranking by pointer jumping along prev, double-buffered: vertex v carries (ptr, cnt, mn, root) and sym -- the vertex 2^r in front of it, the
 *                  members and the symbols between the two, the smallest row among those members and v, and, once ptr has run off the head, the head.  A path vertex of
 *                  rank r is done after ceil(log2(r + 1)) rounds; a cycle vertex never is, and after r rounds its mn is the minimum over 2^r vertices.
 *   k_utg_cut      the cycle vertex that is its cycle's minimum becomes a head: circ = o_in, o_in = 0, the simple record into it is taken out of next and prev.  The cycle's
 *                  vertices are then initialised and ranked again, as a path.
 *   k_utg_tails    every tail names its chain to its head: the tail, the members, the length, and whether the chain is output.
 *   k_utg_table    the unitigs in ascending order of their heads, at the scanned positions of the heads that are output.
 *   k_utg_members  member v of an output chain to slot member_off[unitig] + cnt[v]: a scatter, no sort.
 *   k_utg_emit     an octet of lanes per member, handed out from a counter as in k_get_walk: LF from row v for exactly len(v) - o_in(v) steps, symbol t to
 *                  uoff[u] + off(v) + len(v) - 1 - t.  The LF walk spells a string from its last symbol, and what a member adds to its unitig are its last symbols: one LF
 *                  step per symbol of the output, not one per indexed symbol.
 *   k_utg_linkflag, k_utg_links   the kept records that are not simple, their ends as (unitig, orientation), compacted in their order.
 */
#ifndef RB3GPU_UNITIG_H
#define RB3GPU_UNITIG_H

#include "rb3gpu_walk.h"
#include "rb3gpu_reduce.h"

#define RB3_UTG_NONE 0xFFFFFFFFu

struct UtgRec { int32_t head, tail, members, circ; int64_t len; }; // rb3gpu_unitig_t
struct UtgMem { int32_t row, o_in; int64_t off; };                 // rb3gpu_unitig_member_t
struct UtgLink { int32_t from, to, len; uint8_t from_rev, to_rev, pad[2]; }; // rb3gpu_unitig_link_t

/* c += the threads of the wave for which x holds: one atomic per wave.  Every thread of the wave calls it */
__device__ __forceinline__ void utg_count(bool x, unsigned long long *c)
{
	const unsigned long long b = __ballot(x);
	if (b != 0ull && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) atomicAdd(c, (unsigned long long)__popcll(b));
}

/* (a record that names a string outside the index is never simple: k_utg_degree counts it, and the driver ends the call) */
__device__ __forceinline__ bool utg_simple(const int4 r, int64_t m, const uint32_t *dout, const uint32_t *din)
{
	return (uint64_t)(uint32_t)r.x < (uint64_t)m && (uint64_t)(uint32_t)r.y < (uint64_t)m && r.x != r.y && dout[r.x] == 1u && din[r.y] == 1u;
}

/* the records [0, n) of m strings.  ctr[0] += kept records that name a string outside the index (left alone) */
__global__ void __launch_bounds__(256) k_utg_degree(int64_t n, const OvlRec *rec, const uint32_t *keep, int64_t m, uint32_t *dout, uint32_t *din, unsigned long long *ctr)
{
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool bad = false;
	if (j < n && keep[j] != 0u) {
		const int4 r = reinterpret_cast<const int4*>(rec)[j];
		bad = (uint64_t)(uint32_t)r.x >= (uint64_t)m || (uint64_t)(uint32_t)r.y >= (uint64_t)m;
		if (!bad) atomicAdd(dout + r.x, 1u), atomicAdd(din + r.y, 1u);
	}
	utg_count(bad, ctr);
}

/* next and prev are RB3_UTG_NONE, o_in is 0 at launch (k_utg_degree has checked the records).  ctr[0] += simple records */
__global__ void __launch_bounds__(256) k_utg_simple(int64_t n, const OvlRec *rec, const uint32_t *keep, int64_t m, const uint32_t *dout, const uint32_t *din, uint32_t *next, uint32_t *prev,
		int32_t *o_in, unsigned long long *ctr)
{
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool s = false;
	if (j < n && keep[j] != 0u) {
		const int4 r = reinterpret_cast<const int4*>(rec)[j];
		s = utg_simple(r, m, dout, din);
		if (s) next[r.x] = (uint32_t)r.y, prev[r.y] = (uint32_t)r.x, o_in[r.y] = r.z;
	}
	utg_count(s, ctr);
}

/* m is even: row v ^ 1 is the other strand of row v.  ctr[0] += vertices whose simple record has no mirror image */
__global__ void __launch_bounds__(256) k_utg_asym(int64_t m, const uint32_t *next, unsigned long long *ctr)
{
	const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool bad = false;
	if (v < m && next[v] != RB3_UTG_NONE) bad = next[next[v] ^ 1u] != ((uint32_t)v ^ 1u);
	utg_count(bad, ctr);
}

/* st[v] = (prev[v], members in front, v, the head if v is one) and sym[v] = the symbols in front of v's start as far as prev[v]'s.  live_only: only the vertices whose
 * st[v].x is a vertex (the cycle vertices, after k_utg_cut); the others stay.  ctr[0] += vertices with a pointer */
__global__ void __launch_bounds__(256) k_utg_init(int64_t m, const uint32_t *prev, const int32_t *o_in, const uint32_t *len32, int live_only, uint4 *st, uint64_t *sym, unsigned long long *ctr)
{
	const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool live = false;
	if (v < m && (!live_only || st[v].x != RB3_UTG_NONE)) {
		const uint32_t p = prev[v];
		live = p != RB3_UTG_NONE;
		st[v] = make_uint4(p, live ? 1u : 0u, (uint32_t)v, live ? RB3_UTG_NONE : (uint32_t)v);
		sym[v] = live ? (uint64_t)len32[p] - (uint64_t)(uint32_t)o_in[v] : 0ull;
	}
	utg_count(live, ctr);
}

/* one round: reads (st, sym), writes (st2, sym2).  ctr[0] += vertices that still have a pointer */
__global__ void __launch_bounds__(256) k_utg_jump(int64_t m, const uint4 *st, const uint64_t *sym, uint4 *st2, uint64_t *sym2, unsigned long long *ctr)
{
	const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool live = false;
	if (v < m) {
		uint4 a = st[v];
		uint64_t s = sym[v];
		if (a.x != RB3_UTG_NONE && (uint64_t)a.x < (uint64_t)m) {
			const uint4 q = st[a.x];
			s += sym[a.x];
			a = make_uint4(q.x, a.y + q.y, min(a.z, q.z), q.x == RB3_UTG_NONE ? q.w : a.w);
		}
		live = a.x != RB3_UTG_NONE;
		st2[v] = a, sym2[v] = s;
	}
	utg_count(live, ctr);
}

/* the vertices that still have a pointer lie on cycles and have seen all of theirs: the one that is the minimum becomes the head.  ctr[0] += cycles */
__global__ void __launch_bounds__(256) k_utg_cut(int64_t m, const uint4 *st, uint32_t *next, uint32_t *prev, int32_t *o_in, int32_t *circ, unsigned long long *ctr)
{
	const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool cut = false;
	if (v < m) {
		const uint4 a = st[v];
		cut = a.x != RB3_UTG_NONE && a.z == (uint32_t)v && (uint64_t)prev[v] < (uint64_t)m;
		if (cut) {
			next[prev[v]] = RB3_UTG_NONE; // (the tail: another vertex, a self-loop is never simple; no one else writes it, no one reads next here)
			prev[v] = RB3_UTG_NONE, circ[v] = o_in[v], o_in[v] = 0;
		}
	}
	utg_count(cut, ctr);
}

/* flag[] = 0 and utail[] = RB3_UTG_NONE at launch.  A tail v of head h: utail[h] = v, umem[h], ulen[h], and flag[h] = 1 iff the chain is output: always on one strand;
 * with pair a path iff h <= v ^ 1, a cycle iff its head is even.  ctr[0] += tails, ctr[1] += their members, ctr[2] += tails that are not done or whose head is taken */
__global__ void __launch_bounds__(256) k_utg_tails(int64_t m, int pair, const uint32_t *next, const uint4 *st, const uint64_t *sym, const uint32_t *len32, const int32_t *circ,
		uint32_t *flag, uint32_t *utail, uint32_t *umem, int64_t *ulen, unsigned long long *ctr)
{
	const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool tail = false, bad = false;
	unsigned long long mem = 0;
	if (v < m && next[v] == RB3_UTG_NONE) {
		const uint4 a = st[v];
		tail = true;
		bad = a.x != RB3_UTG_NONE || (uint64_t)a.w >= (uint64_t)m;
		if (!bad) bad = atomicExch(utail + a.w, (uint32_t)v) != RB3_UTG_NONE;
		if (!bad) {
			const uint32_t h = a.w;
			mem = (unsigned long long)a.y + 1ull;
			umem[h] = a.y + 1u, ulen[h] = (int64_t)(sym[v] + (uint64_t)len32[v]);
			flag[h] = !pair || (circ[h] != 0 ? (h & 1u) == 0u : h <= ((uint32_t)v ^ 1u)) ? 1u : 0u;
		}
	}
	utg_count(tail, ctr);
	utg_count(bad, ctr + 2);
	if (mem) atomicAdd(ctr + 1, mem);
}

/* upos: the exclusive scan of flag.  U[upos[h]] for every head that is output, inside [0, cap).  ctr[0] += unitigs written */
__global__ void __launch_bounds__(256) k_utg_table(int64_t m, const uint32_t *flag, const int64_t *upos, const uint32_t *utail, const uint32_t *umem, const int64_t *ulen,
		const int32_t *circ, UtgRec *U, int64_t cap, unsigned long long *ctr)
{
	const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool put = false;
	if (h < m && flag[h] != 0u) {
		const int64_t u = upos[h];
		put = u >= 0 && u < cap;
		if (put) {
			UtgRec r;
			r.head = (int32_t)h, r.tail = (int32_t)utail[h], r.members = (int32_t)umem[h], r.circ = circ[h], r.len = ulen[h];
			U[u] = r;
		}
	}
	utg_count(put, ctr);
}

/* moff[u]: the members in front of unitig u (n_u + 1 entries).  ctr[0] += members stored, ctr[1] += members of output chains that fall outside their unitig's slots */
__global__ void __launch_bounds__(256) k_utg_members(int64_t m, const uint4 *st, const uint64_t *sym, const int32_t *o_in, const uint32_t *flag, const int64_t *upos,
		const int64_t *moff, int64_t n_u, UtgMem *M, uint32_t *mu, unsigned long long *ctr)
{
	const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool put = false, bad = false;
	if (v < m) {
		const uint4 a = st[v];
		bad = a.x != RB3_UTG_NONE || (uint64_t)a.w >= (uint64_t)m;
		if (!bad && flag[a.w] != 0u) {
			const int64_t u = upos[a.w];
			bad = u < 0 || u >= n_u;
			if (!bad) {
				const int64_t slot = moff[u] + (int64_t)a.y;
				bad = slot < moff[u] || slot >= moff[u + 1];
				if (!bad) {
					UtgMem r;
					r.row = (int32_t)v, r.o_in = o_in[v], r.off = (int64_t)sym[v];
					M[slot] = r, mu[slot] = (uint32_t)u;
					put = true;
				}
			}
		}
	}
	utg_count(put, ctr);
	utg_count(bad, ctr + 1);
}

/* the members [i0, i1) of M (each of unitig mu[i], whose symbols start at soff[mu[i]]): symbol t of the walk of row M[i].row to out[soff[u] - base0 + off + len - 1 - t]
 * for t < len - o_in, inside [0, cap).  ctr[0]: the next member to hand out (0 at launch), ctr[1] += LF steps that gave a symbol, ctr[2] += walks that met the sentinel
 * before their last step, ctr[3] += symbols that would land outside the slice (neither happens: the driver answers RB3GPU_EINTERNAL) */
__global__ void __launch_bounds__(256) k_utg_emit(IdxView ix, const UtgMem *M, const uint32_t *mu, const int64_t *soff, const uint32_t *len32, int64_t n_u, int64_t i0, int64_t i1, int64_t base0,
		uint8_t *out, int64_t cap, unsigned long long *ctr)
{
	const int j = threadIdx.x & 7;
	bool act = false, done = false;
	int64_t k = 0, base = 0;
	int32_t t = 0, todo = 0;
	unsigned long long steps = 0, early = 0, outside = 0;
	for (;;) {
		while (!act && !done) { // (the same in the eight lanes of an octet)
			const int64_t i = i0 + walk_take(ctr, j);
			if (i >= i1) { done = true; break; }
			const UtgMem me = M[i];
			k = (int64_t)me.row, t = 0;
			if ((uint64_t)k < (uint64_t)ix.m && (uint64_t)mu[i] < (uint64_t)n_u) { // (every slot has been written: the driver has counted them)
				const int32_t len = (int32_t)len32[k];
				todo = len - me.o_in; // (a member that is wholly the overlap: nothing to write)
				base = soff[mu[i]] - base0 + me.off + (int64_t)len - 1;
				act = todo > 0;
			}
		}
		if (__ballot(act) == 0ull) break;
		int c;
		const int64_t k2 = oct_lf_self(ix, act ? k : 0, j, &c);
		if (act) {
			if (c == 0) ++early, act = false;
			else {
				const int64_t p = base - t;
				++steps;
				if (p >= 0 && p < cap) { if (j == 0) out[p] = (uint8_t)c; }
				else ++outside;
				k = k2;
				if (++t == todo) act = false;
			}
		}
	}
	if (j == 0) {
		if (steps) atomicAdd(ctr + 1, steps);
		if (early) atomicAdd(ctr + 2, early);
		if (outside) atomicAdd(ctr + 3, outside);
	}
}

/* lflag[j] = 1 for the kept records that are links and are output: not simple, and with pair a <= b ^ 1 (lflag[n] = 0 stays) */
__global__ void __launch_bounds__(256) k_utg_linkflag(int64_t n, const OvlRec *rec, const uint32_t *keep, int64_t m, const uint32_t *dout, const uint32_t *din, int pair, uint32_t *lflag)
{
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= n) return;
	uint32_t f = 0u;
	if (keep[j] != 0u) {
		const int4 r = reinterpret_cast<const int4*>(rec)[j];
		f = !utg_simple(r, m, dout, din) && (!pair || (uint32_t)r.x <= ((uint32_t)r.y ^ 1u)) ? 1u : 0u;
	}
	lflag[j] = f;
}

/* the end v of a link: its chain's unitig with +, or, where that chain is not output, the unitig of the other strand's chain with - */
__device__ __forceinline__ bool utg_end(uint32_t v, int pair, const uint4 *st, const uint32_t *flag, const int64_t *upos, int64_t m, int32_t *u, uint8_t *rev)
{
	for (int r = 0; r <= (pair ? 1 : 0); ++r) {
		const uint32_t h = st[v ^ (uint32_t)r].w;
		if ((uint64_t)h < (uint64_t)m && flag[h] != 0u) { *u = (int32_t)upos[h], *rev = (uint8_t)r; return true; }
	}
	return false;
}

/* L[lpos[j]] for the flagged records, inside [0, cap).  ctr[0] += links stored, ctr[1] += links that do not go from a tail to a head, whose ends have no unitig or that
 * would land outside */
__global__ void __launch_bounds__(256) k_utg_links(int64_t n, const OvlRec *rec, const uint32_t *lflag, const int64_t *lpos, const uint32_t *next, const uint32_t *prev, const uint4 *st,
		const uint32_t *flag, const int64_t *upos, int64_t m, int pair, UtgLink *L, int64_t cap, unsigned long long *ctr)
{
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool put = false, bad = false;
	if (j < n && lflag[j] != 0u) {
		const int4 r = reinterpret_cast<const int4*>(rec)[j];
		const int64_t d = lpos[j];
		UtgLink l;
		l.len = r.z, l.pad[0] = l.pad[1] = 0;
		bad = next[r.x] != RB3_UTG_NONE || prev[r.y] != RB3_UTG_NONE || d < 0 || d >= cap;
		if (!bad) bad = !utg_end((uint32_t)r.x, pair, st, flag, upos, m, &l.from, &l.from_rev) || !utg_end((uint32_t)r.y, pair, st, flag, upos, m, &l.to, &l.to_rev);
		if (!bad) L[d] = l, put = true;
	}
	utg_count(put, ctr);
	utg_count(bad, ctr + 1);
}

#endif
