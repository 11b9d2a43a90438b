/*
 * rb3gpu_order.hip -- the strings of one batch put into a sorted order on the GPU (build -s / -r).
 *
 * The reference's ropebwt2 insertion (mr_insert_multi, mrope.c:216-385) builds the BWT of a collection in
 * reverse lexicographic order (RLO, -s) or reverse-complement lexicographic order (RCLO, -r).  Its output is
 * the ordinary (input-order) BWT of the same collection with the strings reordered so that their REVERSED
 * contents ascend, $ < A < C < G < T < N (RLO) or $ < T < G < C < A < N (RCLO; N last), a string that is a
 * suffix of another first.  Identical strings may come in any order: the bytes are the same.
 *
 * The order is read off a suffix sort of the reversed batch: write every string reversed (and complemented for
 * RCLO, which maps T G C A onto A C G T and keeps N last) in its own place, suffix-sort that text with the
 * batch sorter (rb3gpu_sort.hip: GSA order, sentinel i before sentinel i + 1, so equal strings stay in input
 * order and a string that runs out first sorts first), and sort the strings by the rank of the suffix that starts
 * at their first symbol.  The sorter handles any amount of shared tails (duplicated contigs) in its doubling
 * rounds; nothing here depends on how long the strings are.  Then the strings are gathered into their new
 * places, back into the caller's buffer: the batch's suffix sort, its BWT and text-order words, and the merge all
 * see the ordered batch.
 */
#include <cstring>
#include <algorithm>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <stdint.h>

struct rb3sort_ws;
int rb3sort_bwt(rb3sort_ws *ws, hipStream_t st, int64_t n, const uint8_t *d_text, uint8_t *d_bwt, int64_t step, int64_t *d_ckrow, int *rounds, uint64_t *d_tw, uint32_t *d_sa);

struct rb3order_ws {
	void *p[12] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	size_t cap[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	int64_t bytes = 0;
};

enum { O_SID, O_REV, O_BWT, O_TW, O_ENDS, O_KA, O_KB, O_VA, O_VB, O_INV, O_TMP };

static int o_ensure(rb3order_ws *ws, int i, size_t bytes)
{
	if (ws->cap[i] >= bytes && ws->p[i]) return 0;
	if (ws->p[i]) { (void)hipFree(ws->p[i]); ws->bytes -= (int64_t)ws->cap[i]; }
	ws->p[i] = nullptr, ws->cap[i] = 0;
	const size_t want = bytes + (bytes >> 3) + 256;
	if (hipMalloc(&ws->p[i], want) != hipSuccess) { (void)hipGetLastError(); return -1; }
	ws->cap[i] = want, ws->bytes += (int64_t)want;
	return 0;
}

rb3order_ws *rb3order_create(void) { return new rb3order_ws; }

void rb3order_destroy(rb3order_ws *ws)
{
	if (!ws) return;
	for (int i = 0; i < 12; ++i) if (ws->p[i]) (void)hipFree(ws->p[i]);
	delete ws;
}

int64_t rb3order_bytes(const rb3order_ws *ws) { return ws ? ws->bytes : 0; }

/* ---- kernels ---- */

__global__ void __launch_bounds__(256) k_o_flag(const uint8_t *text, int64_t n, uint32_t *flag, unsigned long long *bad)
{
	const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= n) return;
	const uint8_t c = text[p];
	flag[p] = c == 0 ? 1u : 0u;
	if (c > 5) atomicAdd(bad, 1ull);
}

/* ends[i] = position of the sentinel of string i (sid[p]: sentinels before p, i.e. the string p belongs to) */
__global__ void __launch_bounds__(256) k_o_ends(const uint8_t *text, int64_t n, const uint32_t *sid, uint32_t *ends)
{
	const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p < n && text[p] == 0) ends[sid[p]] = (uint32_t)p;
}

/* every string reversed in its own place, its sentinel where it was; comp: A <-> T, C <-> G (N stays) */
__global__ void __launch_bounds__(256) k_o_reverse(const uint8_t *text, int64_t n, const uint32_t *sid, const uint32_t *ends, int comp, uint8_t *rev)
{
	const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= n) return;
	const uint8_t c = text[p];
	if (c == 0) { rev[p] = 0; return; }
	const uint32_t i = sid[p];
	const int64_t b = i ? (int64_t)ends[i - 1] + 1 : 0, e = ends[i];
	rev[b + (e - 1 - p)] = comp && c >= 1 && c <= 4 ? (uint8_t)(5 - c) : c;
}

/* the sort key of string i: the rank of the reversed text's suffix at the string's first position (tw = rank << 3 | symbol) */
__global__ void __launch_bounds__(256) k_o_keys(const uint64_t *tw, const uint32_t *ends, int64_t m, uint32_t *key, uint32_t *val)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= m) return;
	const int64_t b = i ? (int64_t)ends[i - 1] + 1 : 0;
	key[i] = (uint32_t)(tw[b] >> 3), val[i] = (uint32_t)i;
}

/* string order[k] goes k-th: its length (with the sentinel) for the scan of the new starts, and inv[string] = k */
__global__ void __launch_bounds__(256) k_o_lens(const uint32_t *order, const uint32_t *ends, int64_t m, uint32_t *len, uint32_t *inv)
{
	const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= m) return;
	const uint32_t i = order[k];
	const int64_t b = i ? (int64_t)ends[i - 1] + 1 : 0;
	len[k] = (uint32_t)((int64_t)ends[i] - b + 1), inv[i] = (uint32_t)k;
}

__global__ void __launch_bounds__(256) k_o_gather(const uint8_t *text, int64_t n, const uint32_t *sid, const uint32_t *ends, const uint32_t *inv, const uint32_t *nstart, uint8_t *out)
{
	const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= n) return;
	const uint32_t i = sid[p];
	const int64_t b = i ? (int64_t)ends[i - 1] + 1 : 0;
	out[(int64_t)nstart[inv[i]] + (p - b)] = text[p];
}

#define O_HIP(x) do { if ((x) != hipSuccess) { (void)hipGetLastError(); return -2; } } while (0)
#define O_GRID(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, st

/* d_text: n symbols (0..5, the last one 0) in device memory, reordered in place by order so (1 RLO, 2 RCLO); sws: the suffix sorter's scratch
 * (the reversed text is sorted with it).  Returns 0, -1 (out of memory), -2 (HIP error), -3 (bad text or order); *rounds: the sorter's doubling rounds. */
int rb3order_text(rb3order_ws *ws, rb3sort_ws *sws, hipStream_t st, int64_t n, uint8_t *d_text, int so, int *rounds)
{
	if (!ws || !sws || !d_text || n <= 0 || n >= (1LL << 31) || (so != 1 && so != 2)) return -3;
	// 14 bytes per symbol: string numbers, the reversed text (later the gathered one), its BWT and its text-order words (whose buffer holds the
	// sentinel flags and a counter until the sort writes them)
	if (o_ensure(ws, O_SID, (size_t)n * 4) || o_ensure(ws, O_REV, (size_t)n + 16) || o_ensure(ws, O_BWT, (size_t)n + 16) || o_ensure(ws, O_TW, (size_t)n * 8 + 64)) return -1;
	uint32_t *sid = (uint32_t*)ws->p[O_SID], *flag = (uint32_t*)ws->p[O_TW];
	uint8_t *rev = (uint8_t*)ws->p[O_REV], *bwt = (uint8_t*)ws->p[O_BWT];
	uint64_t *tw = (uint64_t*)ws->p[O_TW];
	unsigned long long *bad = (unsigned long long*)(flag + n + ((4 - (n & 3)) & 3)); // (behind the flags, 8-byte aligned)
	size_t tb = 0, b = 0;
	O_HIP(rocprim::exclusive_scan(nullptr, b, flag, sid, 0u, (size_t)n, rocprim::plus<uint32_t>(), st)); tb = std::max(tb, b);
	O_HIP(hipMemsetAsync(bad, 0, 8, st));
	hipLaunchKernelGGL(k_o_flag, O_GRID(n), d_text, n, flag, bad);
	if (o_ensure(ws, O_TMP, tb + 256)) return -1;
	b = ws->cap[O_TMP]; O_HIP(rocprim::exclusive_scan(ws->p[O_TMP], b, flag, sid, 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
	uint32_t before_last = 0;
	uint8_t last = 1;
	unsigned long long nbad = 0;
	O_HIP(hipMemcpyAsync(&before_last, sid + n - 1, 4, hipMemcpyDeviceToHost, st));
	O_HIP(hipMemcpyAsync(&last, d_text + n - 1, 1, hipMemcpyDeviceToHost, st));
	O_HIP(hipMemcpyAsync(&nbad, bad, 8, hipMemcpyDeviceToHost, st));
	O_HIP(hipStreamSynchronize(st));
	if (nbad != 0 || last != 0) return -3;
	const int64_t m = (int64_t)before_last + 1; // (the last symbol is a sentinel)
	if (m == 1) { if (rounds) *rounds = 0; return 0; } // one string: nothing to reorder
	if (o_ensure(ws, O_ENDS, (size_t)m * 4) || o_ensure(ws, O_KA, (size_t)m * 4) || o_ensure(ws, O_KB, (size_t)m * 4) ||
		o_ensure(ws, O_VA, (size_t)m * 4) || o_ensure(ws, O_VB, (size_t)m * 4) || o_ensure(ws, O_INV, (size_t)m * 4)) return -1;
	uint32_t *ends = (uint32_t*)ws->p[O_ENDS], *ka = (uint32_t*)ws->p[O_KA], *kb = (uint32_t*)ws->p[O_KB];
	uint32_t *va = (uint32_t*)ws->p[O_VA], *vb = (uint32_t*)ws->p[O_VB], *inv = (uint32_t*)ws->p[O_INV];
	hipLaunchKernelGGL(k_o_ends, O_GRID(n), d_text, n, (const uint32_t*)sid, ends);
	hipLaunchKernelGGL(k_o_reverse, O_GRID(n), d_text, n, (const uint32_t*)sid, (const uint32_t*)ends, so == 2 ? 1 : 0, rev);
	const int r = rb3sort_bwt(sws, st, n, rev, bwt, 0, nullptr, rounds, tw, nullptr);
	if (r < 0) return r;
	int nb = 1;
	while ((1LL << nb) < n) ++nb; // ranks are below n
	hipLaunchKernelGGL(k_o_keys, O_GRID(m), (const uint64_t*)tw, (const uint32_t*)ends, m, ka, va);
	O_HIP(rocprim::radix_sort_pairs(nullptr, b, ka, kb, va, vb, (size_t)m, 0, nb, st));
	size_t b2 = 0;
	O_HIP(rocprim::exclusive_scan(nullptr, b2, ka, kb, 0u, (size_t)m, rocprim::plus<uint32_t>(), st));
	if (o_ensure(ws, O_TMP, std::max(b, b2) + 256)) return -1;
	b = ws->cap[O_TMP]; O_HIP(rocprim::radix_sort_pairs(ws->p[O_TMP], b, ka, kb, va, vb, (size_t)m, 0, nb, st)); // vb: the strings in their new order
	hipLaunchKernelGGL(k_o_lens, O_GRID(m), (const uint32_t*)vb, (const uint32_t*)ends, m, ka, inv);
	b = ws->cap[O_TMP]; O_HIP(rocprim::exclusive_scan(ws->p[O_TMP], b, ka, kb, 0u, (size_t)m, rocprim::plus<uint32_t>(), st)); // kb: new starts
	hipLaunchKernelGGL(k_o_gather, O_GRID(n), d_text, n, (const uint32_t*)sid, (const uint32_t*)ends, (const uint32_t*)inv, (const uint32_t*)kb, rev); // (the reversed text is not needed any more)
	O_HIP(hipMemcpyAsync(d_text, rev, (size_t)n, hipMemcpyDeviceToDevice, st));
	O_HIP(hipStreamSynchronize(st));
	return 0;
}
