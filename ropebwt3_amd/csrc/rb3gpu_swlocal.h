/*
 * rb3gpu_swlocal.h -- local alignment of whole queries against the index over the query's DAWG (`sw --local`: the reference's sw_core in its
 * general form, bwa-sw.c:329-526, and the backtrack of its one best hit, bwa-sw.c:76-114, 154-195, 254-258).
 *
 * The rows of the dynamic program are the NODES of the query's directed acyclic word graph (host/dawg.c), in topological order; a node has a
 * symbol and a list of predecessors, any earlier nodes.  The table, growth, selection, extension, heap and the whole row step of rb3gpu_hapdiv.h
 * (hd_tab_clear, hd_stage_ext, hd_cands, hd_fphase, hd_store_bt) are used as they are, and the backtrack is sw_walk of rb3gpu_sw.h; this file keeps
 * what the graph adds to the linear program (hd_rows):
 *   - the kept cells of EVERY node of a query stay in global memory (n_node * N cells of 56 bytes from cell_off[q] on, their count per node
 *     beside them), because any later node may read them; the 12-byte backtrack words lie beside them as in `sw -e`, word node * N + column;
 *   - a node with several predecessors whose cells number more than N drops what cannot reach its best N: max_min_sc is the (N + 1)-th largest
 *     H of those cells (a wave-wide bisection on the value: only the value matters) less max(go + ge, mis), at least 0;
 *   - candidates arrive predecessor by predecessor in list order, cell by cell in column order; a predecessor's cells are staged in the row
 *     buffer, extended an octet per cell, and merged by lane 0.  (A node's cells are extended once per successor here; the reference keeps
 *     the extensions in a cache: DESIGN.md 7h);
 *   - the symbols of the query a cell has consumed (HdCell.pad; the larger stays when two candidates meet) differ within a row, so the rule that
 *     hd_rows states by row is stated by cell: the F phase of a node runs iff the LAST predecessor cell the loops visited (what hd_cands
 *     returns) has consumed end_len symbols, cut or not.
 * The hit of a query is column 0 of the first node whose best H is above that of every node before it, if that H reaches min_sc.
 *
 *   k_swl_fill   a wave per query, queries by grid stride: the nodes, then lane 0 walks from the best cell back to the root and COUNTS the steps:
 *                flag[q], cnt[q], raw[q] and node[q] of the slice;
 *   scan         exclusive sums of flag[] and cnt[], as for `sw -e`;
 *   k_swl_emit   a lane per query: the hit to its place and the walk once more, writing the step bytes of rb3gpu_sw.h; `=` is "the base
 *                equals the NODE's symbol", so an N of the query, a node of symbol 1, is `=` against an indexed A.
 *
 * Every index read from memory is checked before it is used: a predecessor that is not an earlier node, a list outside pre[], a count above N, a
 * walk that leaves the matrix, runs longer than n_node * (N + 1) steps or needs an F column that was not kept raise ctr[2] like everything
 * hd_rows cannot represent, and the call fails.
 */
#ifndef RB3GPU_SWLOCAL_H
#define RB3GPU_SWLOCAL_H

#include "rb3gpu_sw.h"

struct SlWs {
	HdWs w;                          // the per-block arrays as everywhere; w.bt: 3 words per cell of the slice, query q from cell_off[q] on (w.bt_stride is not used)
	HdCell *cells; int32_t *ncnt;    // of the slice: the cells from cell_off[q] on, their counts per node of the slice
};

/* how sw_walk reads the symbol of row r: that of node r */
struct SlNodeSym {
	const uint8_t *nsym;
	__device__ __forceinline__ int operator()(uint32_t r) const { return (int)nsym[r]; }
};

/* cells of the predecessors [p0, p1) of pre[] whose H is at least v (all lanes; the same number in every lane) */
__device__ static int sl_count_ge(const HdCell *cells, const int32_t *ncnt, const int32_t *pre, int64_t p0, int64_t p1, int N, int32_t v, int lane)
{
	int n = 0;
	for (int64_t j = p0; j < p1; ++j) {
		const int32_t pid = pre[j], cn = ncnt[pid];
		for (int c = lane; c < cn; c += 64) n += cells[(size_t)pid * N + c].H >= v;
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
	return n;
}

/* queries [q0, q1): query q owns the nodes [node_off[q], node_off[q + 1]) of nsym[] and pre_off[] (pre_off has one more entry than there are nodes and
 * names places of pre[0, n_pre_all), whose entries are node numbers within the query); its cells start at cell_off[q] of ws.cells / ws.w.bt, its counts at
 * node_off[q] - node_off[q0] of ws.ncnt.  Per query of the slice flag, cnt, raw, node (every one is written).  ctr as k_sw_fill */
__global__ void __launch_bounds__(64) k_swl_fill(IdxView ix, Acc7 acc, const int64_t *node_off, const uint8_t *nsym, const int64_t *pre_off, const int32_t *pre, int64_t n_pre_all,
		const int64_t *cell_off, int64_t q0, int64_t q1, HdOpt o, int end_len, SlWs ws, int lds_slots, uint32_t *flag, uint32_t *cnt, SwRaw *raw, int32_t *node,
		unsigned long long *ctr)
{
	__shared__ HdCell s_tab[HD_LDS_SLOTS];
	__shared__ HdCell s_row[HD_LDS_N];
	__shared__ HdExt s_ext[HD_LDS_N * 5];
	__shared__ int32_t s_heap[HD_LDS_N];
	__shared__ HdTab s_T;
	__shared__ int32_t s_err, s_lastq;
	const int lane = threadIdx.x;
	const int N = o.N;
	const int64_t b = blockIdx.x;
	const HdBlk B = hd_blk(ws.w, b, N, lds_slots, s_tab, s_row, s_ext, s_heap, &s_T, &s_err);
	HdCell *const row = B.row;
	unsigned long long n_ext = 0, n_t2 = 0;
	const int64_t node0 = node_off[q0];

	for (int64_t w = q0 + b; w < q1; w += gridDim.x) {
		const int64_t g0 = node_off[w], n_node = node_off[w + 1] - g0;
		const uint8_t *sym = nsym + g0;
		const int64_t *poff = pre_off + g0;
		HdCell *cells = ws.cells + cell_off[w];
		uint32_t *bt = ws.w.bt + cell_off[w] * 3;
		int32_t *ncnt = ws.ncnt + (g0 - node0);
		int32_t best = 0;
		uint32_t best_pos = 0;
		bool done = n_node >= 1 && (uint64_t)n_node * (uint32_t)N < 0xFFFFFFFFull;
		__syncthreads();
		if (lane == 0) {
			hd_tab_init(B), s_lastq = 0;
			if (done) cells[0] = hd_root(acc), ncnt[0] = 1;
		}
		if (done && lane < 3) bt[lane] = lane < 2 ? HD_NONE : 0u;
		__syncthreads();
		for (int64_t i = 1; i < n_node && done; ++i) {
			const int cq = (int)sym[i];
			const int64_t p0 = poff[i], p1 = poff[i + 1];
			if (p0 < 0 || p1 < p0 || p1 > n_pre_all) { done = false; break; }
			bool okp = true;
			int64_t n_cell = 0;
			for (int64_t j = p0; j < p1; ++j) { // (every lane reads the same words)
				const int32_t pid = pre[j];
				if (pid < 0 || pid >= i) { okp = false; break; }
				const int32_t cn = ncnt[pid];
				if (cn < 0 || cn > N) { okp = false; break; }
				n_cell += cn;
			}
			if (!okp) { done = false; break; }
			int32_t mm = 0; // max_min_sc
			if (p1 - p0 > 1) {
				if (n_cell > N) {
					int32_t hv = 0, lv = 0;
					for (int64_t j = p0; j < p1; ++j) {
						const int32_t pid = pre[j], cn = ncnt[pid];
						for (int c = lane; c < cn; c += 64) hv = max(hv, cells[(size_t)pid * N + c].H);
					}
#pragma unroll
					for (int d = 32; d >= 1; d >>= 1) hv = max(hv, __shfl_xor(hv, d));
					while (lv < hv) { // the largest v that N + 1 cells reach: the (N + 1)-th largest H
						const int32_t mid = lv + (hv - lv + 1) / 2;
						if (sl_count_ge(cells, ncnt, pre, p0, p1, N, mid, lane) >= N + 1) lv = mid;
						else hv = mid - 1;
					}
					mm = lv;
				}
				mm -= max(o.go + o.ge, o.mi);
				mm = max(mm, 0);
			}
			hd_tab_clear(B, lane);
			__syncthreads();
			for (int64_t j = p0; j < p1; ++j) { // the candidates, predecessor by predecessor
				const int32_t pid = pre[j], n = ncnt[pid];
				if (n == 0) continue;
				{
					const uint32_t *src = (const uint32_t*)(cells + (size_t)pid * N);
					uint32_t *dst = (uint32_t*)row;
					for (int x = lane; x < n * (int)(sizeof(HdCell) / 4); x += 64) dst[x] = src[x];
				}
				__syncthreads();
				hd_stage_ext(ix, B, n, lane);
				__syncthreads();
				if (lane == 0) s_lastq = hd_cands<true>(B, o, n, (uint32_t)pid * (uint32_t)N, cq, end_len, 0, mm, n_ext);
				__syncthreads();
				if (s_err) break;
			}
			if (s_err) { done = false; break; }
			if (s_T.count == 0) { // no cell: later nodes see an empty predecessor
				if (lane == 0) ncnt[i] = 0;
				__syncthreads();
				continue;
			}
			int n = hd_top(s_T.t, 1u << s_T.bits, s_T.ub, N, row, lane);
			__syncthreads();
			if (s_lastq >= end_len && !hd_fphase<true>(ix, B, o, n, n_ext, lane)) { done = false; break; } // (by the LAST predecessor cell visited, cut or not)
			if (row[0].H > best) best = row[0].H, best_pos = (uint32_t)i * (uint32_t)N;
			hd_store_bt<true>(acc, row, n, cq, bt + (size_t)i * N * 3, lane); // what the backtrack needs, and the cells for the nodes to come
			for (int c = lane; c < n; c += 64) cells[(size_t)i * N + c] = row[c];
			if (lane == 0) ncnt[i] = n;
			__syncthreads();
		}
		__syncthreads();
		if (lane == 0) {
			SwRaw r;
			r.lo = r.hi = 0, r.score = r.qlen = r.rlen = r.n_steps = 0, r.step_off = 0;
			bool hit = false;
			if (done && !s_err && best >= o.min_sc) {
				int ql, rl;
				const int steps = sw_walk<false>(bt, N, n_node, best_pos, SlNodeSym{sym}, nullptr, 0u, ql, rl);
				if (steps < 0) s_err = 1;
				else {
					const HdCell x = cells[best_pos];
					hit = true, r.lo = x.lo, r.hi = x.hi, r.score = best, r.qlen = ql, r.rlen = rl, r.n_steps = steps;
				}
			}
			flag[w - q0] = hit ? 1u : 0u, cnt[w - q0] = (uint32_t)r.n_steps, raw[w - q0] = r, node[w - q0] = hit ? (int32_t)(best_pos / (uint32_t)N) : -1;
			if (s_T.tier) ++n_t2;
			if (s_err || !done) atomicAdd(ctr + 2, 1ull);
		}
	}
	if (lane == 0) {
		if (n_ext) atomicAdd(ctr, n_ext);
		if (n_t2) atomicAdd(ctr + 1, n_t2);
	}
}

/* the queries [0, nq) of the slice that starts at query q0: a hit to out[hoff[q]], its steps to steps[soff[q], ...) */
__global__ void __launch_bounds__(256) k_swl_emit(const int64_t *node_off, const uint8_t *nsym, const int64_t *cell_off, int64_t q0, int N, const uint32_t *bt, int64_t nq,
		const uint32_t *flag, const SwRaw *raw, const int32_t *node, const int64_t *hoff, const int64_t *soff, SwRaw *out, uint8_t *steps, unsigned long long *ctr)
{
	for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < nq; s += (int64_t)gridDim.x * blockDim.x) {
		if (!flag[s]) continue;
		const int64_t w = q0 + s, n_node = node_off[w + 1] - node_off[w];
		SwRaw r = raw[s];
		int ql = 0, rl = 0, n = -1;
		r.step_off = soff[s];
		if (node[s] >= 0 && node[s] < n_node)
			n = sw_walk<true>(bt + cell_off[w] * 3, N, n_node, (uint32_t)node[s] * (uint32_t)N, SlNodeSym{nsym + node_off[w]}, steps + soff[s], (uint32_t)r.n_steps, ql, rl);
		if (n != r.n_steps || ql != r.qlen || rl != r.rlen) atomicAdd(ctr + 2, 1ull); // (the same walk twice: cannot happen)
		out[hoff[s]] = r;
	}
}

#endif
