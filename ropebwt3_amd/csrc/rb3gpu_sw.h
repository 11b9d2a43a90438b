/*
 * rb3gpu_sw.h -- end-to-end alignments of whole queries against the index with the alignment written out (`sw -e`, `--all-e2e`, `-g`: the
 * reference's sw_core on a linear query, bwa-sw.c:329-526, and its sw_backtrack / sw_backtrack1_core, bwa-sw.c:76-114, 218-253).
 *
 * The dynamic program is that of `hapdiv` (hd_rows of rb3gpu_hapdiv.h: one row loop for both, over the row step that `sw --local` uses
 * too), with three differences: a query has its own length, mismatches and gaps start after end_len symbols, and a cell of the backtrack matrix keeps its base (bits 5-7 of its third word; the
 * matrix stays at 12 bytes a cell and the F column keeps its 24 bits).  The matrices of ALL queries of a slice stay in global memory, query q
 * at cell bt_off[q] (a prefix sum of (len + 1) * N over the slice), because the alignments are written in a second pass:
 *
 *   k_sw_fill   a wave per query, queries handed out by a grid stride: the rows, the dedup of the last row, and for every surviving cell --
 *               not filtered, H from H, H >= min_sc, within e2e_drop -- a walk back to the root that only COUNTS its steps.  Column c of
 *               query q is slot (q - q0) * N + c of the slice: flag[slot], cnt[slot] steps, raw[slot] the hit (lo, hi, score, lengths);
 *   scan        exclusive sums of flag[] and cnt[] give every hit its place among the hits and its bytes among the steps, in column order;
 *   k_sw_emit   a lane per slot: the hit to its place, and the walk once more, now writing one byte per step, (op << 4 | base) with op
 *               0 `=`, 1 `X`, 2 `I`, 3 `D`, in the order sw_backtrack1_core pushes them: the first byte is query position 0.  `=` is
 *               "base equals the query's symbol", so N against N is `=`.
 *
 * sw_walk is the one backtrack of this file and of rb3gpu_swlocal.h: it is told the rows of the matrix, the cell to start from and how to read the
 * query's symbol of a row.  A walk that leaves the matrix, runs longer than rows * (N + 1) steps or needs an F column that was not kept raises ctr[2]
 * like everything hd_rows cannot represent, and the call fails.
 */
#ifndef RB3GPU_SW_H
#define RB3GPU_SW_H

#include "rb3gpu_hapdiv.h"

struct SwRaw { int64_t lo, hi; int32_t score, qlen, rlen, n_steps; int64_t step_off; };   // 40 bytes; the host reads (lo, hi) of the dense array with stride 5

/* how the walk reads the symbol of row r of the query q[0, k): its last r symbols are aligned there */
struct SwQrySym {
	const uint8_t *q; int k;
	__device__ __forceinline__ int operator()(uint32_t r) const { return min((int)q[k - (int)r], 5); }
};

/* the walk from cell `pos` (row * N + column) of a matrix of `rows` rows to the root; sym(r): the query's symbol of row r (SwQrySym here, the node's symbol
 * in rb3gpu_swlocal.h).  EMIT: one byte per step to out.  Returns the steps, -1 if the walk cannot be represented -- it leaves the matrix, takes more
 * than the rows * (N + 1) steps of the longest walk there is (every row once, and its N columns through gaps of the index side) or, EMIT, more than
 * `room` bytes; qlen / rlen: symbols of the query / of the index it consumed */
template<bool EMIT, class Sym>
__device__ static int sw_walk(const uint32_t *bt, int N, int64_t rows, uint32_t pos, const Sym sym, uint8_t *out, uint32_t room, int &qlen, int &rlen)
{
	const uint64_t total = (uint64_t)rows * (uint32_t)N, limit = (uint64_t)rows * ((uint64_t)N + 1);
	uint64_t steps = 0;
	int last = 0;
	qlen = rlen = 0;
	while (pos > 0) {
		if (pos >= total || steps >= limit || steps >= 0x7fffffffu) return -1;
		const uint32_t r = pos / (uint32_t)N, m = bt[(size_t)pos * 3 + 2];
		const int state = last == 0 ? (int)(m & 3u) : last;
		const int gext = state == 1 ? (int)(m >> 2 & 1u) : state == 2 ? (int)(m >> 3 & 1u) : 0;
		const int base = (int)(m >> 5 & 7u);
		uint32_t np = 0;
		int op;
		if (state == 0) {
			np = bt[(size_t)pos * 3];
			if (np >= r * (uint32_t)N) return -1;
			op = base == sym(r) ? 0 : 1, ++qlen, ++rlen;
		} else if (state == 1) {
			np = bt[(size_t)pos * 3 + 1];
			if (np >= r * (uint32_t)N) return -1;
			op = 2, ++qlen;
		} else if (state == 2 && (m & 16u) && (m >> 8) < (uint32_t)N) {
			np = r * (uint32_t)N + (m >> 8);
			op = 3, ++rlen;
		} else return -1;
		if (EMIT) {
			if (steps >= room) return -1;
			out[steps] = (uint8_t)(op << 4 | base);
		}
		++steps;
		pos = np, last = gext ? state : 0;
	}
	return (int)steps;
}

/* queries [q0, q1): query q is sym[qoff[q], qoff[q + 1]); its matrix starts at cell bt_off[q] of ws.bt (ws.bt_stride is not used).  Per slot of
 * the slice flag, cnt, raw (every slot is written); n_hit[q - q0].  ctr as k_hapdiv: [0] += extensions, [1] += queries whose table went to global
 * memory, [2] != 0: something could not be represented */
__global__ void __launch_bounds__(64) k_sw_fill(IdxView ix, Acc7 acc, const uint8_t *sym, const int64_t *qoff, const int64_t *bt_off, int64_t q0, int64_t q1, HdOpt o, int end_len,
		HdWs ws, int lds_slots, uint32_t *flag, uint32_t *cnt, SwRaw *raw, int32_t *n_hit, unsigned long long *ctr)
{
	__shared__ HdCell s_tab[HD_LDS_SLOTS];
	__shared__ HdCell s_row[HD_LDS_N];
	__shared__ HdExt s_ext[HD_LDS_N * 5];
	__shared__ int32_t s_heap[HD_LDS_N];
	__shared__ HdTab s_T;
	__shared__ int32_t s_err;
	const int lane = threadIdx.x;
	const int N = o.N;
	const int64_t b = blockIdx.x;
	const HdBlk B = hd_blk(ws, b, N, lds_slots, s_tab, s_row, s_ext, s_heap, &s_T, &s_err);
	const HdCell *row = B.row;
	unsigned long long n_ext = 0, n_t2 = 0;

	for (int64_t w = q0 + b; w < q1; w += gridDim.x) {
		const uint8_t *q = sym + qoff[w];
		const int k = (int)(qoff[w + 1] - qoff[w]);
		uint32_t *bt = ws.bt + bt_off[w] * 3;
		const int64_t slot0 = (w - q0) * N;
		int best_sc = 0, n = 0, hits = 0;
		bool done = true;
		if (k > 0) n = hd_rows<true>(ix, acc, q, k, end_len, o, B, bt, n_ext, best_sc, done);
		else { // (no rows: no hits)
			__syncthreads();
			if (lane == 0) s_err = 0;
			__syncthreads();
		}
		const bool any = k > 0 && done && n > 0 && best_sc >= o.min_sc;
		const int32_t h0 = any ? row[0].H : 0;
		for (int c0 = 0; c0 < N; c0 += 64) {
			const int c = c0 + lane;
			SwRaw r;
			r.lo = r.hi = 0, r.score = r.qlen = r.rlen = r.n_steps = 0, r.step_off = 0;
			bool hit = false;
			if (any && c < n) {
				const HdCell x = row[c];
				hit = !(x.fl & HD_FLT) && (x.fl & 3u) == 0 && x.H >= o.min_sc && (o.drop < 0 || h0 - x.H <= o.drop);
				if (hit) {
					int ql, rl;
					const int steps = sw_walk<false>(bt, N, (int64_t)k + 1, (uint32_t)k * (uint32_t)N + (uint32_t)c, SwQrySym{q, k}, nullptr, 0u, ql, rl);
					if (steps < 0) atomicOr(&s_err, 1), hit = false;
					else r.lo = x.lo, r.hi = x.hi, r.score = x.H, r.qlen = ql, r.rlen = rl, r.n_steps = steps;
				}
			}
			if (c < N) flag[slot0 + c] = hit ? 1u : 0u, cnt[slot0 + c] = (uint32_t)r.n_steps, raw[slot0 + c] = r;
			hits += __popcll(__ballot(hit));
		}
		__syncthreads();
		if (lane == 0) {
			n_hit[w - q0] = hits;
			if (k > 0 && s_T.tier) ++n_t2;
			if (s_err || !done) atomicAdd(ctr + 2, 1ull);
		}
	}
	if (lane == 0) {
		if (n_ext) atomicAdd(ctr, n_ext);
		if (n_t2) atomicAdd(ctr + 1, n_t2);
	}
}

/* the slots [0, n_slot) of the slice that starts at query q0: a hit to out[hoff[slot]], its steps to steps[soff[slot], ...) */
__global__ void __launch_bounds__(256) k_sw_emit(const uint8_t *sym, const int64_t *qoff, const int64_t *bt_off, int64_t q0, int N, const uint32_t *bt, int64_t n_slot,
		const uint32_t *flag, const SwRaw *raw, const int64_t *hoff, const int64_t *soff, SwRaw *out, uint8_t *steps, unsigned long long *ctr)
{
	for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_slot; s += (int64_t)gridDim.x * blockDim.x) {
		if (!flag[s]) continue;
		const int64_t w = q0 + s / N;
		const int c = (int)(s % N), k = (int)(qoff[w + 1] - qoff[w]);
		SwRaw r = raw[s];
		int ql, rl;
		r.step_off = soff[s];
		const int n = sw_walk<true>(bt + bt_off[w] * 3, N, (int64_t)k + 1, (uint32_t)k * (uint32_t)N + (uint32_t)c, SwQrySym{sym + qoff[w], k}, steps + soff[s], (uint32_t)r.n_steps, ql, rl);
		if (n != r.n_steps || ql != r.qlen || rl != r.rlen) atomicAdd(ctr + 2, 1ull); // (the same walk twice: cannot happen)
		out[hoff[s]] = r;
	}
}

#endif
