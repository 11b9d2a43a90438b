/*
 * rb3gpu_swlocal.h -- local alignment of whole queries against the index over the query's DAWG (`sw --local`: the reference's sw_core in its
 * general form, bwa-sw.c:329-526, and the backtrack of its one best hit, bwa-sw.c:76-114, 154-195, 254-258).
 *
 * The rows of the dynamic program are the NODES of the query's directed acyclic word graph (host/dawg.c), in topological order; a node has a
 * symbol and a list of predecessors, any earlier nodes.  So, against the linear program of rb3gpu_hapdiv.h (hd_rows), whose table, growth,
 * selection, extension and heap are used as they are:
 *   - the kept cells of EVERY node of a query stay in global memory (n_node * N cells of 56 bytes from cell_off[q] on, their count per node
 *     beside them), because any later node may read them; the 12-byte backtrack words lie beside them as in `sw -e`, word node * N + column;
 *   - a node with several predecessors whose cells number more than N drops what cannot reach its best N: max_min_sc is the (N + 1)-th largest
 *     H of those cells (a wave-wide bisection on the value: only the value matters) less max(go + ge, mis), at least 0;
 *   - candidates arrive predecessor by predecessor in list order, cell by cell in column order; a predecessor's cells are staged in the row
 *     buffer, extended an octet per cell, and merged by lane 0.  (A node's cells are extended once per successor here; the reference keeps
 *     the extensions in a cache: DESIGN.md 7h);
 *   - a cell carries the symbols of the query it has consumed (HdCell.pad; the larger stays when two candidates meet), and a mismatch, a gap
 *     of the index side and the F phase are allowed by that number, not by the row: the F phase of a node runs iff the LAST predecessor cell
 *     the loops visited has consumed end_len symbols, cut or not.
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

struct SlZ { int64_t lo, hi, lo_rc; int32_t H, F, qlen, pad; };
struct SlWs {
	HdCell *cells; uint32_t *bt; int32_t *ncnt;   // of the slice: cells and 3 words per cell from cell_off[q] on, counts per node of the slice
	HdCell *tab; int64_t tab_cap;                 // per block, as HdWs
	HdCell *row;                                  // N
	HdExt *ext;                                   // 5 N
	int32_t *heap;                                // N
	SlZ *stack; int64_t stack_cap;
	int64_t *fpar; int64_t fpar_cap;              // pairs
};

/* the walk from cell `pos` (node * N + column) of a query of n_node nodes with symbols nsym[] to the root; as sw_walk of rb3gpu_sw.h */
template<bool EMIT>
__device__ static int sl_walk(const uint32_t *bt, int N, int64_t n_node, const uint8_t *nsym, uint32_t pos, uint8_t *out, uint32_t room, int &qlen, int &rlen)
{
	const uint64_t total = (uint64_t)n_node * (uint32_t)N, limit = (uint64_t)n_node * ((uint64_t)N + 1);
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
			op = base == (int)nsym[r] ? 0 : 1, ++qlen, ++rlen;
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
 * names places of pre[0, n_pre_all), whose entries are node numbers within the query); its cells start at cell_off[q] of ws.cells / ws.bt, its counts at
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
	const int lane = threadIdx.x, j8 = lane & 7, oct = lane >> 3;
	const int N = o.N;
	const int64_t b = blockIdx.x;
	HdCell *gtab = ws.tab + b * ws.tab_cap;
	const bool small = N <= HD_LDS_N;
	HdCell *row = small ? s_row : ws.row + b * N;
	HdExt *ext = small ? s_ext : ws.ext + b * 5 * N;
	int32_t *heap = small ? s_heap : ws.heap + b * N;
	SlZ *stack = ws.stack + b * ws.stack_cap;
	int64_t *fpar = ws.fpar + b * 2 * ws.fpar_cap;
	int bits0 = 2;
	while ((1 << bits0) < 4 * N) ++bits0;
	unsigned long long n_ext = 0, n_t2 = 0;
	const int64_t node0 = node_off[q0];

	for (int64_t w = q0 + b; w < q1; w += gridDim.x) {
		const int64_t g0 = node_off[w], n_node = node_off[w + 1] - g0;
		const uint8_t *sym = nsym + g0;
		const int64_t *poff = pre_off + g0;
		HdCell *cells = ws.cells + cell_off[w];
		uint32_t *bt = ws.bt + cell_off[w] * 3;
		int32_t *ncnt = ws.ncnt + (g0 - node0);
		int32_t best = 0;
		uint32_t best_pos = 0;
		bool done = n_node >= 1 && (uint64_t)n_node * (uint32_t)N < 0xFFFFFFFFull;
		__syncthreads();
		if (lane == 0) {
			HdTab T;
			T.bits = bits0, T.count = 0, T.ub = HD_USED_A;
			T.tier = (1 << bits0) > lds_slots ? 1 : 0;
			T.t = T.tier ? gtab : s_tab;
			s_T = T, s_err = 0, s_lastq = 0;
			if (done) {
				HdCell r;
				r.lo = 0, r.hi = acc.a[6], r.lo_rc = 0, r.H = r.E = r.F = 0, r.H_pos = r.E_pos = HD_NONE, r.fpar = HD_UNSET, r.fl = 0, r.pad = 0;
				cells[0] = r, ncnt[0] = 1;
			}
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
			{ // an empty table of the capacity it has grown to
				HdCell *t = s_T.t;
				const uint32_t cap = 1u << s_T.bits;
				for (uint32_t s = lane; s < cap; s += 64) t[s].fl = 0;
				if (lane == 0) s_T.count = 0;
			}
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
				for (int c0 = 0; c0 < n; c0 += 8) {
					const int col = c0 + oct;
					const bool act = col < n;
					const int64_t lo = act ? row[col].lo : 0, hi = act ? row[col].hi : 0, rc = act ? row[col].lo_rc : 0;
					HdExt e[5];
					hd_extend(ix, lo, hi, rc, j8, e);
					if (act && j8 < 5) {
						HdExt v = e[0];
#pragma unroll
						for (int c = 1; c < 5; ++c) v = j8 == c ? e[c] : v;
						ext[col * 5 + j8] = v;
					}
				}
				__syncthreads();
				if (lane == 0) {
					HdTab T = s_T;
					bool ok = true;
					int ch;
					for (int col = 0; col < n && ok; ++col) {
						const HdCell p = row[col];
						s_lastq = (int32_t)p.pad;
						if (p.H + o.ma < mm) continue;
						const uint32_t pos = (uint32_t)pid * (uint32_t)N + (uint32_t)col;
						const bool inner = (int32_t)p.pad >= end_len;
						int64_t last_rc = 0;
						HdCell r;
						r.E = r.F = 0, r.H_pos = pos, r.E_pos = HD_NONE, r.fpar = HD_UNSET, r.fl = 0, r.pad = p.pad + 1;
						for (int c = 1; c < 6 && ok; ++c) {
							const HdExt e = ext[col * 5 + c - 1];
							const int sc = c == cq && c != 5 ? o.ma : -o.mi;
							if (e.hi == e.lo || p.H + sc <= 0 || p.H + sc < mm || (c != cq && !inner)) continue;
							last_rc = e.rc;
							r.lo = e.lo, r.hi = e.hi, r.lo_rc = e.rc, r.H = p.H + sc;
							ok = hd_merge(T, r, ch, gtab, ws.tab_cap, lds_slots) != nullptr;
						}
						int32_t ev = p.H - o.go > p.E ? p.H - o.go : p.E;
						const uint32_t ef = p.H - o.go > p.E ? 0u : 4u;
						ev -= o.ge;
						if (ev > 0 && ev >= mm && inner && ok) {
							r.lo = p.lo, r.hi = p.hi, r.lo_rc = last_rc, r.H = r.E = ev, r.F = 0, r.H_pos = HD_NONE, r.E_pos = pos, r.fl = 1u | ef;
							ok = hd_merge(T, r, ch, gtab, ws.tab_cap, lds_slots) != nullptr;
						}
					}
					n_ext += n;
					if (!ok) s_err = 1;
					s_T = T;
				}
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
			int n_fpar = 0;
			if (s_lastq >= end_len) { // the F phase of hd_rows; a candidate inherits the consumed symbols of the cell it leaves
				HdTab T = s_T; // (used by lane 0)
				int hsz = 0, next = 0, sp = 0;
				bool ok = true;
				if (lane == 0) for (int t = n - 1; t >= 0; --t) hd_heap_put(heap, hsz, N, row[t].H);
				for (;;) {
					SlZ z = {0, 0, 0, 0, 0, 0, 0};
					int32_t f = 0, low = 0;
					uint32_t ff = 0;
					int go_on = 0;
					if (lane == 0) {
						while (ok) {
							if (sp > 0) z = stack[--sp];
							else if (next < n) {
								const HdCell c = row[next++];
								if (c.H <= o.go + o.ge) continue;
								z.lo = c.lo, z.hi = c.hi, z.lo_rc = c.lo_rc, z.H = c.H, z.F = c.F, z.qlen = (int32_t)c.pad;
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
					hd_extend(ix, zlo, zhi, zrc, j8, e);
					if (lane == 0) {
						++n_ext;
						for (int c = 0; c < 5 && ok; ++c) {
							if (e[c].hi == e[c].lo) continue;
							HdCell r;
							r.lo = e[c].lo, r.hi = e[c].hi, r.lo_rc = e[c].rc, r.H = r.F = f, r.E = 0, r.H_pos = r.E_pos = HD_NONE, r.fpar = HD_UNSET, r.fl = 2u | ff, r.pad = (uint32_t)z.qlen;
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
								SlZ y;
								y.lo = qc->lo, y.hi = qc->hi, y.lo_rc = qc->lo_rc, y.H = qc->H, y.F = qc->F, y.qlen = (int32_t)qc->pad, y.pad = 0;
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
					for (int c = lane; c < n; c += 64) {
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
			if (row[0].H > best) best = row[0].H, best_pos = (uint32_t)i * (uint32_t)N;
			for (int c = lane; c < n; c += 64) { // the cells for the nodes to come, and what the backtrack needs
				const HdCell x = row[c];
				int base = 0;
#pragma unroll
				for (int a = 1; a < 6; ++a) base = acc.a[a] <= x.lo ? a : base;
				const uint32_t m = (x.fl & 15u) | (x.F != 0 && (x.fl & HD_FSET) ? 16u : 0u) | (uint32_t)base << 5 | (x.fpar & 0xFFFFFFu) << 8;
				uint32_t *d = bt + ((size_t)i * N + c) * 3;
				d[0] = x.H_pos, d[1] = x.E_pos, d[2] = m;
				cells[(size_t)i * N + c] = x;
			}
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
				const int steps = sl_walk<false>(bt, N, n_node, sym, best_pos, nullptr, 0u, ql, rl);
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
			n = sl_walk<true>(bt + cell_off[w] * 3, N, n_node, nsym + node_off[w], (uint32_t)node[s] * (uint32_t)N, steps + soff[s], (uint32_t)r.n_steps, ql, rl);
		if (n != r.n_steps || ql != r.qlen || rl != r.rlen) atomicAdd(ctr + 2, 1ull); // (the same walk twice: cannot happen)
		out[hoff[s]] = r;
	}
}

#endif
