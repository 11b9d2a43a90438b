/*
 * rb3gpu_bre.hip -- the BRE interchange format on the device (bre.c / bre.h of the reference; mr_print_bre, build.c:85-106;
 * rld_restore's BRE branch, rld0.c:245-283).  A BRE record is one symbol byte and b_per_run length bytes, little-endian; a run
 * longer than max = 2^(8 b_per_run) - 1 is written as records of max and a remainder, and a reader joins consecutive records
 * of one symbol.  Header and footer are the host's (host/bre.c); this file packs and unpacks the RECORDS.
 *
 *   packing    (rb3bre_enc_*)  run words start << 3 | sym of maximal runs, a piece at a time:
 *                k_bre_count   records of every run, ceil(len / max)
 *                scan          exclusive, 64-bit, in place (rocPRIM): the first record of every run, and the piece's total
 *                k_bre_emit    a block owns 4096 bytes of OUTPUT; a lane takes every 256th record that touches them, finds its run
 *                              by a search in the scanned offsets, assembles it in LDS; then every lane stores 16 bytes
 *   unpacking  (rb3bre_dec_*)  raw records in HBM:
 *                k_bre_scan    lengths out of the records, validated; records whose symbol differs from their predecessor's counted
 *                scan          exclusive, in place: the start of every record, and the number of symbols
 *                k_bre_fill    symbols [p0, p1), one byte each: a lane owns 16 bytes of OUTPUT, finds the record of its first one by
 *                              a search in the starts and walks on from there -- records hold at least one symbol, so 16 steps at most
 * Neither direction has a loop over the length of a run.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <rocprim/rocprim.hpp>
#include "rb3gpu.h"

#define BRE_TILE 4096 /* bytes of output per block: 256 lanes x 16 */
#define BRE_HIP(x) do { if ((x) != hipSuccess) { (void)hipGetLastError(); ret = -2; goto done; } } while (0)

/* the largest i in [lo, hi] with a[i] <= x (a ascending; a[lo] <= x is the caller's) */
__device__ __forceinline__ int64_t bre_find(const uint64_t *a, int64_t lo, int64_t hi, uint64_t x)
{
	while (lo < hi) {
		const int64_t mid = (lo + hi + 1) >> 1;
		if (a[mid] <= x) lo = mid; else hi = mid - 1;
	}
	return lo;
}

/* ---- packing ---- */

/* w[0 .. m]: the starts of m maximal runs and, in w[m], the position behind the last of them */
__global__ void __launch_bounds__(256) k_bre_count(const uint64_t *w, int64_t m, uint64_t maxlen, uint64_t *cnt, unsigned long long *bad)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i > m) return;
	if (i == m) { cnt[m] = 0; return; }
	const uint64_t a = w[i] >> 3, b = w[i + 1] >> 3;
	if (b <= a || (w[i] & 7) > 5) { atomicAdd(bad, 1ull); cnt[i] = 0; return; }
	cnt[i] = (b - a + maxlen - 1) / maxlen;
}

/* Bytes [B0, B1) of the piece's record stream (record r lies at r * (1 + bpr)) to out[byte - B0]; out is 16-byte aligned and B0 a multiple of
 * the tile, so a block's stores are aligned whatever the record size is.  Records straddle tiles (and windows): a record's bytes are
 * written by whichever tile they fall into.  The lanes that hold the ragged tail of the range store their bytes one by one, every other
 * lane one dwordx4. */
__global__ void __launch_bounds__(256) k_bre_emit(const uint64_t *w, const uint64_t *roff, int64_t m, uint64_t maxlen, int bpr, int64_t B0, int64_t B1, uint8_t *out)
{
	__shared__ uint4 tile4[BRE_TILE / 16];
	__shared__ int64_t s_run[2];
	uint8_t *tile = (uint8_t*)tile4;
	const int rs = 1 + bpr, tid = (int)threadIdx.x;
	const int64_t o0 = (int64_t)blockIdx.x * BRE_TILE, s0 = B0 + o0; // the tile in `out` and in the stream
	const int64_t lo = s0, hi = s0 + BRE_TILE < B1 ? s0 + BRE_TILE : B1;
	if (lo >= hi) return;
	const int64_t r0 = lo / rs, r1 = (hi + rs - 1) / rs; // the records that touch the tile
	if (tid < 2) s_run[tid] = bre_find(roff, 0, m - 1, (uint64_t)(tid == 0 ? r0 : r1 - 1));
	__syncthreads();
	const int64_t ia = s_run[0], ib = s_run[1];
	for (int64_t r = r0 + tid; r < r1; r += 256) {
		const int64_t i = bre_find(roff, ia, ib, (uint64_t)r);
		const uint64_t k = (uint64_t)r - roff[i], n = roff[i + 1] - roff[i], ww = w[i];
		const uint64_t l = k + 1 < n ? maxlen : (w[i + 1] >> 3) - (ww >> 3) - k * maxlen;
		const int64_t at = r * rs - s0;
		if (at >= 0 && at < BRE_TILE) tile[at] = (uint8_t)(ww & 7);
		for (int j = 0; j < bpr; ++j) {
			const int64_t p = at + 1 + j;
			if (p >= 0 && p < BRE_TILE) tile[p] = (uint8_t)(l >> (8 * j));
		}
	}
	__syncthreads();
	const int64_t a = s0 + tid * 16;
	if (a + 16 <= hi) *(uint4*)(out + o0 + tid * 16) = tile4[tid];
	else
		for (int j = 0; j < 16 && a + j < hi; ++j) out[o0 + tid * 16 + j] = tile[tid * 16 + j];
}

struct rb3bre_enc {
	hipStream_t st;
	int bpr;
	int64_t cap, win, carry;
	uint64_t *w, *roff;
	void *tmp;
	size_t tb;
	uint8_t *out[2], *host[2]; // a window of record bytes on the device, and where the host takes it from
	bool own_host;
	unsigned long long *bad;
	hipEvent_t ev[6]; // [0..1] a window's copy is done, [2..5] around the emit kernel of the window in buffer 0 / 1
	uint64_t *hm; // pinned: [0] the sentinel word, [1] total, [2] bad
	rb3gpu_bre_stats_t stt;
};

void rb3bre_enc_abort(rb3bre_enc *e)
{
	if (!e) return;
	(void)hipStreamSynchronize(e->st);
	if (e->w) (void)hipFree(e->w);
	if (e->roff) (void)hipFree(e->roff);
	if (e->tmp) (void)hipFree(e->tmp);
	if (e->bad) (void)hipFree(e->bad);
	for (int i = 0; i < 2; ++i) {
		if (e->out[i]) (void)hipFree(e->out[i]);
		if (e->own_host && e->host[i]) (void)hipHostFree(e->host[i]);
	}
	for (int i = 0; i < 6; ++i) if (e->ev[i]) (void)hipEventDestroy(e->ev[i]);
	if (e->hm) (void)hipHostFree(e->hm);
	(void)hipGetLastError();
	delete e;
}

/* cap_runs: the most runs one piece brings; win: bytes of records per window, a multiple of 4096 (stage[], if given, holds as many).
 * 0, -1 (out of memory) or -2 (HIP error) */
int rb3bre_enc_begin(hipStream_t st, int bpr, int64_t cap_runs, int64_t win, uint8_t *stage[2], rb3bre_enc **out)
{
	int ret = 0;
	*out = nullptr;
	rb3bre_enc *e = new (std::nothrow) rb3bre_enc;
	if (!e) return -1;
	memset(e, 0, sizeof(*e));
	e->st = st, e->bpr = bpr, e->cap = cap_runs + 2, e->win = win; // (+ the run carried over from the piece before and the position behind the last one)
	if (hipMalloc(&e->w, (size_t)e->cap * 8) != hipSuccess || hipMalloc(&e->roff, (size_t)e->cap * 8) != hipSuccess || hipMalloc(&e->bad, 8) != hipSuccess ||
		hipMalloc(&e->out[0], (size_t)win + 16) != hipSuccess || hipMalloc(&e->out[1], (size_t)win + 16) != hipSuccess) { ret = -1; goto done; }
	if (rocprim::exclusive_scan(nullptr, e->tb, e->roff, e->roff, (uint64_t)0, (size_t)e->cap, rocprim::plus<uint64_t>(), st) != hipSuccess) { ret = -2; goto done; }
	if (hipMalloc(&e->tmp, e->tb + 256) != hipSuccess) { ret = -1; goto done; }
	if (stage && stage[0] && stage[1]) e->host[0] = stage[0], e->host[1] = stage[1];
	else {
		e->own_host = true;
		for (int i = 0; i < 2; ++i) if (hipHostMalloc((void**)&e->host[i], (size_t)win, hipHostMallocDefault) != hipSuccess) { ret = -1; goto done; }
	}
	if (hipHostMalloc((void**)&e->hm, 64, hipHostMallocDefault) != hipSuccess) { ret = -1; goto done; }
	for (int i = 0; i < 6; ++i) BRE_HIP(hipEventCreate(&e->ev[i]));
	BRE_HIP(hipMemsetAsync(e->bad, 0, 8, st));
	*out = e;
	return 0;
done:
	(void)hipGetLastError();
	rb3bre_enc_abort(e);
	return ret;
}

/* where the run words of the next piece go, and how many fit */
uint64_t *rb3bre_enc_buffer(rb3bre_enc *e, int64_t *room)
{
	if (room) *room = e->cap - 1 - e->carry;
	return e->w + e->carry;
}

/* n_new run words have been written to rb3bre_enc_buffer (on the stream).  The last run of a piece ends where the next piece starts, so it is
 * carried over; end >= 0 says that this piece is the last one and the index ends there.  The records go to emit window by window: while the
 * host consumes one, the device writes the next.  0, -2 (HIP error), -3 (the runs are not ascending), -4 (emit refused) */
int rb3bre_enc_piece(rb3bre_enc *e, int64_t n_new, int64_t end, rb3gpu_emit_bytes_f emit, void *data)
{
	int ret = 0;
	hipStream_t st = e->st;
	const int rs = 1 + e->bpr;
	const uint64_t maxlen = e->bpr >= 8 ? ~0ull : (1ull << (8 * e->bpr)) - 1;
	const int64_t all = e->carry + n_new;
	int64_t m = all;
	hipEvent_t t0 = e->ev[2], t1 = e->ev[3];
	if (end >= 0) {
		e->hm[0] = (uint64_t)end << 3;
		BRE_HIP(hipMemcpyAsync(e->w + all, e->hm, 8, hipMemcpyHostToDevice, st));
	} else --m;
	if (m <= 0) { e->carry = all; return 0; }
	BRE_HIP(hipEventRecord(t0, st));
	hipLaunchKernelGGL(k_bre_count, dim3((unsigned)((m + 1 + 255) / 256)), dim3(256), 0, st, (const uint64_t*)e->w, m, maxlen, e->roff, e->bad);
	{ size_t b = e->tb; BRE_HIP(rocprim::exclusive_scan(e->tmp, b, e->roff, e->roff, (uint64_t)0, (size_t)(m + 1), rocprim::plus<uint64_t>(), st)); }
	BRE_HIP(hipEventRecord(t1, st));
	BRE_HIP(hipMemcpyAsync(e->hm + 1, e->roff + m, 8, hipMemcpyDeviceToHost, st));
	BRE_HIP(hipMemcpyAsync(e->hm + 2, e->bad, 8, hipMemcpyDeviceToHost, st));
	BRE_HIP(hipStreamSynchronize(st));
	{ float ms = 0; if (hipEventElapsedTime(&ms, t0, t1) == hipSuccess) e->stt.ms_scan += ms; }
	if (e->hm[2] != 0) return -3;
	{
		const int64_t n_rec = (int64_t)e->hm[1], nb = n_rec * rs;
		int64_t pend_len = -1;
		int pend = 0, i = 0;
		for (int64_t B0 = 0; B0 < nb; B0 += e->win, i ^= 1) {
			const int64_t B1 = B0 + e->win < nb ? B0 + e->win : nb;
			BRE_HIP(hipEventRecord(e->ev[2 + 2 * i], st));
			hipLaunchKernelGGL(k_bre_emit, dim3((unsigned)((B1 - B0 + BRE_TILE - 1) / BRE_TILE)), dim3(256), 0, st, (const uint64_t*)e->w, (const uint64_t*)e->roff, m, maxlen, e->bpr, B0, B1, e->out[i]);
			BRE_HIP(hipEventRecord(e->ev[3 + 2 * i], st));
			BRE_HIP(hipMemcpyAsync(e->host[i], e->out[i], (size_t)(B1 - B0), hipMemcpyDeviceToHost, st));
			BRE_HIP(hipEventRecord(e->ev[i], st));
			if (pend_len >= 0) { // the window before: its copy is done, the device is busy with this one
				float ms = 0;
				BRE_HIP(hipEventSynchronize(e->ev[pend]));
				if (hipEventElapsedTime(&ms, e->ev[2 + 2 * pend], e->ev[3 + 2 * pend]) == hipSuccess) e->stt.ms_pack += ms;
				if (emit(data, pend_len, e->host[pend]) != 0) { ret = -4; goto done; }
			}
			pend = i, pend_len = B1 - B0;
		}
		if (pend_len >= 0) {
			float ms = 0;
			BRE_HIP(hipEventSynchronize(e->ev[pend]));
			if (hipEventElapsedTime(&ms, e->ev[2 + 2 * pend], e->ev[3 + 2 * pend]) == hipSuccess) e->stt.ms_pack += ms;
			if (emit(data, pend_len, e->host[pend]) != 0) { ret = -4; goto done; }
		}
		e->stt.n_rec += n_rec, e->stt.n_run += m, e->stt.n_pieces += 1;
	}
	if (end < 0) { // the run that ends in the next piece
		BRE_HIP(hipMemcpyAsync(e->w, e->w + m, 8, hipMemcpyDeviceToDevice, st));
		e->carry = 1;
	} else e->carry = 0;
done:
	if (ret != 0) (void)hipStreamSynchronize(st);
	return ret;
}

void rb3bre_enc_end(rb3bre_enc *e, rb3gpu_bre_stats_t *st)
{
	if (st) *st = e->stt;
	rb3bre_enc_abort(e);
}

/* ---- unpacking ---- */

__global__ void __launch_bounds__(256) k_bre_scan(const uint8_t *rec, int64_t n_rec, int bpr, uint64_t *len, unsigned long long *flag)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int rs = 1 + bpr;
	int first = 0;
	if (i < n_rec) {
		const uint8_t *p = rec + i * rs;
		const int c = p[0];
		uint64_t l = 0;
		for (int j = 0; j < bpr; ++j) l |= (uint64_t)p[1 + j] << (8 * j);
		if (c > 5 || l == 0 || l >= (1ull << 56)) { atomicOr(flag, 1ull); l = 0; }
		len[i] = l;
		first = i == 0 || p[-rs] != c;
	} else if (i == n_rec) len[i] = 0;
	const int n = __syncthreads_count(first);
	if (threadIdx.x == 0 && n > 0) atomicAdd(flag + 1, (unsigned long long)n);
}

/* symbols [p0, p1) to out[0 .. p1 - p0); out is 16-byte aligned.  start[0 .. n_rec]: where every record starts, and the total */
__global__ void __launch_bounds__(256) k_bre_fill(const uint8_t *rec, const uint64_t *start, int64_t n_rec, int bpr, int64_t p0, int64_t p1, uint8_t *out)
{
	__shared__ int64_t s_rec[2];
	const int rs = 1 + bpr, tid = (int)threadIdx.x;
	const int64_t q0 = p0 + (int64_t)blockIdx.x * BRE_TILE, q1 = q0 + BRE_TILE < p1 ? q0 + BRE_TILE : p1;
	if (q0 >= q1) return;
	if (tid < 2) s_rec[tid] = bre_find(start, 0, n_rec - 1, (uint64_t)(tid == 0 ? q0 : q1 - 1));
	__syncthreads();
	const int64_t q = q0 + tid * 16;
	if (q >= q1) return;
	int64_t r = bre_find(start, s_rec[0], s_rec[1], (uint64_t)q);
	uint64_t nxt = start[r + 1];
	uint32_t c = rec[r * rs], v[4] = { 0, 0, 0, 0 };
	const int nb = q + 16 <= q1 ? 16 : (int)(q1 - q);
	for (int j = 0; j < nb; ++j) {
		while ((uint64_t)(q + j) >= nxt) ++r, nxt = start[r + 1], c = rec[r * rs]; // (q + j < p1 <= the total: r stays below n_rec)
		v[j >> 2] |= c << (8 * (j & 3));
	}
	uint8_t *o = out + (q - p0);
	if (nb == 16) *(uint4*)o = make_uint4(v[0], v[1], v[2], v[3]);
	else for (int j = 0; j < nb; ++j) o[j] = (uint8_t)(v[j >> 2] >> (8 * (j & 3)));
}

struct rb3bre_dec {
	hipStream_t st;
	int bpr;
	int64_t n_rec;
	const uint8_t *rec;
	uint64_t *start;
	void *tmp;
	unsigned long long *flag; // [0] an invalid record, [1] records that open a run
};

void rb3bre_dec_end(rb3bre_dec *c)
{
	if (!c) return;
	(void)hipStreamSynchronize(c->st);
	if (c->start) (void)hipFree(c->start);
	if (c->tmp) (void)hipFree(c->tmp);
	if (c->flag) (void)hipFree(c->flag);
	(void)hipGetLastError();
	delete c;
}

/* d_rec: n_rec records in device memory.  0 with the counts of the stream and the time of scan, -1 (out of memory), -2 (HIP error), -3 (an invalid record) */
int rb3bre_dec_begin(hipStream_t st, int bpr, int64_t n_rec, const uint8_t *d_rec, rb3bre_dec **ctx, int64_t *n_sym, int64_t *n_run, double *ms_scan)
{
	int ret = 0;
	size_t tb = 0;
	unsigned long long hflag[2] = { 0, 0 };
	uint64_t tot = 0;
	hipEvent_t ev[2] = { nullptr, nullptr };
	*ctx = nullptr, *n_sym = *n_run = 0;
	rb3bre_dec *c = new (std::nothrow) rb3bre_dec;
	if (!c) return -1;
	memset(c, 0, sizeof(*c));
	c->st = st, c->bpr = bpr, c->n_rec = n_rec, c->rec = d_rec;
	if (hipMalloc(&c->start, (size_t)(n_rec + 1) * 8) != hipSuccess || hipMalloc(&c->flag, 16) != hipSuccess) { ret = -1; goto done; }
	BRE_HIP(rocprim::exclusive_scan(nullptr, tb, c->start, c->start, (uint64_t)0, (size_t)(n_rec + 1), rocprim::plus<uint64_t>(), st));
	if (hipMalloc(&c->tmp, tb + 256) != hipSuccess) { ret = -1; goto done; }
	BRE_HIP(hipEventCreate(&ev[0]));
	BRE_HIP(hipEventCreate(&ev[1]));
	BRE_HIP(hipMemsetAsync(c->flag, 0, 16, st));
	BRE_HIP(hipEventRecord(ev[0], st));
	hipLaunchKernelGGL(k_bre_scan, dim3((unsigned)((n_rec + 1 + 255) / 256)), dim3(256), 0, st, d_rec, n_rec, bpr, c->start, c->flag);
	{ size_t b = tb; BRE_HIP(rocprim::exclusive_scan(c->tmp, b, c->start, c->start, (uint64_t)0, (size_t)(n_rec + 1), rocprim::plus<uint64_t>(), st)); }
	BRE_HIP(hipEventRecord(ev[1], st));
	BRE_HIP(hipMemcpyAsync(hflag, c->flag, 16, hipMemcpyDeviceToHost, st));
	BRE_HIP(hipMemcpyAsync(&tot, c->start + n_rec, 8, hipMemcpyDeviceToHost, st));
	BRE_HIP(hipStreamSynchronize(st));
	if (ms_scan) { float ms = 0; if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) *ms_scan = ms; }
	if (hflag[0] != 0 || tot == 0 || tot >= (1ull << 62)) { ret = -3; goto done; }
	*n_sym = (int64_t)tot, *n_run = (int64_t)hflag[1];
done:
	for (int i = 0; i < 2; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]);
	if (ret != 0) { (void)hipGetLastError(); rb3bre_dec_end(c); return ret; }
	*ctx = c;
	return 0;
}

/* the symbols of [p0, p1) into d_out (p1 - p0 bytes, 16-byte aligned), queued on the stream; the context stays open */
int rb3bre_dec_range(rb3bre_dec *c, int64_t p0, int64_t p1, uint8_t *d_out)
{
	if (p1 <= p0) return 0;
	hipLaunchKernelGGL(k_bre_fill, dim3((unsigned)((p1 - p0 + BRE_TILE - 1) / BRE_TILE)), dim3(256), 0, c->st, c->rec, (const uint64_t*)c->start, c->n_rec, c->bpr, p0, p1, d_out);
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

int64_t rb3bre_dec_bytes(const rb3bre_dec *c) { return c ? (c->n_rec + 1) * 8 : 0; }
