/*
 * main.c -- `ropebwt3-amd`: the `build` command of ropebwt3 with the merge path running on an
 * MI355X through the C ABI of include/rb3gpu.h.  Same options, same input handling and the
 * same output bytes as the reference's build.c:136-263 (FMD and plain output are byte-identical;
 * FMR is loadable by the reference but, as in the reference, not canonical).
 *
 * Host side stays C: sequence parsing (seqio.c), per-batch suffix sorting (sais.c), FMD/FMR
 * codecs (fmd.c, fmr.c).  What build.c does on an mrope_t* is done on an rb3gpu_t*:
 *   rb3_enc_plain2fmr  (build.c:77,223)  -> rb3gpu_from_plain
 *   rb3_fmi_merge_plain (build.c:78,226) -> rb3gpu_merge_plain
 *   rb3_enc_fmd2fmr / mr_restore (180-181) -> rb3h_index_read_runs + rb3gpu_from_runs
 *   rb3_enc_fmr2fmd + rld_dump (249-252), mr_dump (247), mr_print_bwt (254) -> rb3gpu_export_runs
 *     feeding rb3h_fmdw_* / rb3h_fmrw_* / the plain printer
 * There is no CPU merge path in this program: without a HIP device it exits with an error.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <getopt.h>
#include <pthread.h>
#include "rb3host.h"
#include "rb3gpu.h"

#define BF_NO_FOR 0x1
#define BF_NO_REV 0x2
#define BF_LINE   0x4

enum { FMT_PLAIN = 0, FMT_FMD, FMT_FMR, FMT_BRE };

typedef struct {
	int64_t flag, batch_size;
	int fmt, n_threads, sais_threads, block_len, max_nodes;
	int device, n_gpus, split_log2, rebatch, gpu_sort, host_fmd, interval;
	int64_t gpu_batch;      /* with GPU suffix sorting a batch (-m) is cut into sub-batches of at most this many symbols, at record
	                           boundaries: the .fmd does not depend on the batching, and the GPU sorter takes < 2^31 */
	int64_t gpu_sort_limit; /* batches of this many symbols or more go to the host sorter (one record longer than a sub-batch) */
	int so;                 /* string order (-s RLO, -r RCLO; RB3GPU_SO_*): asked for, then the one the build uses (main_build) */
} bopt_t;

/* how the batches of this run were sorted (for the closing statistics line) */
static struct { int64_t n_gpu, n_host, sym_gpu, sym_host; double ms_upload, ms_sort, ms_order; } g_sorted;
static int g_order = 0; /* the build's string order (RB3GPU_SO_*): its batches are ordered on the GPU, never sorted on the host */
static pthread_mutex_t g_sorted_mtx = PTHREAD_MUTEX_INITIALIZER; /* (the slices of a multi-GPU build end at different times) */
/* what the handles of the other slices of a multi-GPU build did, added up before they are destroyed (the closing statistics) */
static struct { double ms_path; int64_t n_sym; } g_other_slices;

static void bopt_init(bopt_t *o) /* build.c:31-41 */
{
	memset(o, 0, sizeof(*o));
	o->n_threads = 4, o->sais_threads = -1, o->fmt = FMT_PLAIN;
	o->block_len = 512, o->max_nodes = 64, o->batch_size = 7000000000LL;
	o->device = 0, o->n_gpus = 1, o->split_log2 = 0, o->rebatch = 0, o->gpu_sort = 1, o->host_fmd = 0;
	o->gpu_batch = 1LL << 29, o->gpu_sort_limit = (int64_t)INT32_MAX - 16;
}

/* the size at which the reader cuts batches: -m, or the GPU sub-batch size if that is smaller */
static int64_t batch_cut(const bopt_t *o)
{
	if (o->gpu_sort && o->gpu_batch > 0 && (o->batch_size <= 0 || o->gpu_batch < o->batch_size)) return o->gpu_batch;
	return o->batch_size;
}

static int usage_build(FILE *fp, const bopt_t *opt)
{
	fprintf(fp, "Usage: ropebwt3-amd build [options] <in.fa> [...]\n");
	fprintf(fp, "Options:\n");
	fprintf(fp, "  Algorithm:\n");
	fprintf(fp, "    -m NUM      batch size [7G]\n");
	fprintf(fp, "    -t INT      total number of threads [%d]\n", opt->n_threads);
	fprintf(fp, "    -p INT      sort INT batches at once ahead of the GPU merge: sorter threads with a GPU sorter each (at most 3;\n");
	fprintf(fp, "                default 1) or, with --host-sort, host sorter threads (default 0: sort and merge in turn)\n");
	fprintf(fp, "    -l INT      leaf block size in B+-tree (FMR output only) [%d]\n", opt->block_len);
	fprintf(fp, "    -n INT      max number children per internal node (FMR output only) [%d]\n", opt->max_nodes);
	fprintf(fp, "    --gpu INT   HIP device ordinal [%d]\n", opt->device);
	fprintf(fp, "    --gpus INT  build on INT GPUs: the input files are cut into INT contiguous slices, every GPU indexes one (devices --gpu,\n");
	fprintf(fp, "                --gpu + 1, ...), and the indexes are merged pairwise in input order (same output) [1]\n");
	fprintf(fp, "    --interval  with --gpus INT: ONE index cut into INT intervals of positions, one per GPU; every batch after the first is\n");
	fprintf(fp, "                merged by all GPUs in lock step, its strings' LF chains hopping between the GPUs that own their insertion\n");
	fprintf(fp, "                points (for batches of short strings: one round per symbol of the longest one; same output)\n");
	fprintf(fp, "    --split INT start extra LF walkers every 2^INT rows (0=auto, -1=never) [%d]\n", opt->split_log2);
	fprintf(fp, "    --rebatch   let a batch span input files (same output, fewer merge rounds)\n");
	fprintf(fp, "    --host-sort suffix-sort the batches on the host (default: on the GPU; same output; -p then sets the number\n");
	fprintf(fp, "                of host sorter threads)\n");
	fprintf(fp, "    --gpu-batch NUM  with GPU sorting, cut the batches of -m into sub-batches of at most NUM symbols at record\n");
	fprintf(fp, "                boundaries (the output does not depend on the batching; the GPU sorter takes < 2^31) [512M]\n");
	fprintf(fp, "    --host-fmd  pack/unpack FMD files on the host even where the GPU could\n");
	fprintf(fp, "  Input:\n");
	fprintf(fp, "    -i FILE     read existing index from FILE []\n");
	fprintf(fp, "    -L          one sequence per line in the input\n");
	fprintf(fp, "    -F          no forward strand\n");
	fprintf(fp, "    -R          no reverse strand\n");
	fprintf(fp, "  Output:\n");
	fprintf(fp, "    -o FILE     output to FILE [stdout]\n");
	fprintf(fp, "    -d          dump in the fermi-delta format (FMD)\n");
	fprintf(fp, "    -e          dump in the BRE format (records packed on the GPU)\n");
	fprintf(fp, "    --bre-run-bytes INT  bytes of a BRE record's run length, 1..4 [2]\n");
	fprintf(fp, "    -b          dump in the ropebwt format (FMR)\n");
	fprintf(fp, "    -S FILE     save the current index to FILE after each input file []\n");
	fprintf(fp, "  String order:\n");
	fprintf(fp, "    -s          reverse lexicographic order (RLO): fewer runs for short reads (GPU sorting, one GPU)\n");
	fprintf(fp, "    -r          reverse-complement lexicographic order (RCLO)\n");
	fprintf(fp, "  Not available in this build (ropebwt2 insertion and debugging formats): -2 -T -e\n");
	return fp == stdout ? 0 : 1;
}

/* ---- batch buffers in page-locked memory ------------------------------------------------------
 * The reader writes every batch straight into memory from rb3gpu_pinned_alloc, so its way to HBM is one DMA at PCIe speed
 * (through pageable memory a single host thread has to stage it first, at half that or less: 88 of the 437 ms of the merge
 * path of a 152-genome build).  Obtaining page-locked memory is slow (it is mapped for the device), so the buffers of
 * finished batches go on a free list and the reader takes them from there: a build allocates a handful, at its start. */
#define PINPOOL_MAX 8
#define PINPOOL_SLOTS 64
static struct { pthread_mutex_t mtx; void *p[PINPOOL_SLOTS]; int64_t cap[PINPOOL_SLOTS]; int busy[PINPOOL_SLOTS]; int n; } g_pin = { PTHREAD_MUTEX_INITIALIZER, {0}, {0}, {0}, 0 };
static int64_t g_pin_limit = 0; /* RB3_PINNED_LIMIT (tests): requests above it are answered as if the runtime had none */
static volatile int g_pin_off = 0; /* page-locked memory could not be had: pageable buffers from then on */

static void *pin_alloc(int64_t min_bytes, int64_t *cap)
{
	int i, best = -1, n_free = 0;
	void *p = 0;
	pthread_mutex_lock(&g_pin.mtx);
	for (i = 0; i < g_pin.n; ++i)
		if (!g_pin.busy[i]) {
			++n_free;
			if (g_pin.cap[i] >= min_bytes && (best < 0 || g_pin.cap[i] < g_pin.cap[best])) best = i;
		}
	if (best >= 0) g_pin.busy[best] = 1, p = g_pin.p[best], *cap = g_pin.cap[best];
	else if (n_free > 0) { /* nothing large enough: the small ones only hold on to page-locked memory */
		for (i = 0; i < g_pin.n; ++i)
			if (!g_pin.busy[i]) {
				rb3gpu_pinned_free(g_pin.p[i]);
				g_pin.p[i] = g_pin.p[g_pin.n - 1], g_pin.cap[i] = g_pin.cap[g_pin.n - 1], g_pin.busy[i] = g_pin.busy[g_pin.n - 1];
				--g_pin.n, --i;
			}
	}
	pthread_mutex_unlock(&g_pin.mtx);
	if (p) return p;
	if (min_bytes < (16 << 20)) min_bytes = 16 << 20; /* (a batch of one short line still gets a buffer worth keeping) */
	/* Page-locked memory is an optimisation (one DMA per batch), not a requirement: where the runtime cannot supply it (a multi-GB
	 * batch with --host-sort) or the table is full (many --gpus slices), the batch lives in pageable memory, which the engine
	 * stages (rb3gpu.h: "NULL: use malloc").  pin_release() tells the two apart by the table. */
	p = g_pin_off || (g_pin_limit > 0 && min_bytes > g_pin_limit) ? 0 : rb3gpu_pinned_alloc(min_bytes);
	if (p != 0) {
		pthread_mutex_lock(&g_pin.mtx);
		if (g_pin.n < PINPOOL_SLOTS) g_pin.p[g_pin.n] = p, g_pin.cap[g_pin.n] = min_bytes, g_pin.busy[g_pin.n] = 1, ++g_pin.n;
		else { rb3gpu_pinned_free(p); p = 0; }
		pthread_mutex_unlock(&g_pin.mtx);
	} else if (!g_pin_off && g_pin_limit <= 0) {
		g_pin_off = 1; /* (asking again for every batch would cost a failed system call each time) */
		if (rb3h_verbose >= 2) fprintf(stderr, "WARNING: no page-locked memory for a batch of %ld bytes; batches are staged from pageable memory from here on\n", (long)min_bytes);
	}
	if (p == 0 && (p = malloc((size_t)min_bytes)) == 0) return 0;
	*cap = min_bytes;
	return p;
}

static void pin_release(void *p)
{
	int i, n_free = 0, pooled = 0;
	pthread_mutex_lock(&g_pin.mtx);
	for (i = 0; i < g_pin.n; ++i) {
		if (g_pin.p[i] == p) g_pin.busy[i] = 0, pooled = 1;
		n_free += !g_pin.busy[i];
	}
	if (!pooled) { /* a pageable stand-in (pin_alloc): a busy page-locked buffer is always in the table */
		pthread_mutex_unlock(&g_pin.mtx);
		free(p);
		return;
	}
	if (n_free > PINPOOL_MAX) { /* give the smallest idle one back */
		int k = -1;
		for (i = 0; i < g_pin.n; ++i)
			if (!g_pin.busy[i] && (k < 0 || g_pin.cap[i] < g_pin.cap[k])) k = i;
		if (k >= 0) {
			rb3gpu_pinned_free(g_pin.p[k]);
			g_pin.p[k] = g_pin.p[g_pin.n - 1], g_pin.cap[k] = g_pin.cap[g_pin.n - 1], g_pin.busy[k] = g_pin.busy[g_pin.n - 1];
			--g_pin.n;
		}
	}
	pthread_mutex_unlock(&g_pin.mtx);
}

static void pin_drain(void)
{
	int i;
	pthread_mutex_lock(&g_pin.mtx);
	for (i = 0; i < g_pin.n; ++i) rb3gpu_pinned_free(g_pin.p[i]);
	g_pin.n = 0;
	pthread_mutex_unlock(&g_pin.mtx);
}

/* ---- run sinks --------------------------------------------------------------------------- */

typedef struct { uint64_t *a; int64_t n, m; } runvec_t;

static int sink_runvec(void *data, int c, int64_t l)
{
	runvec_t *v = (runvec_t*)data;
	if (v->n == v->m) {
		v->m = v->m ? v->m * 2 : 1 << 16;
		v->a = (uint64_t*)realloc(v->a, (size_t)v->m * 8);
		if (v->a == 0) return -1;
	}
	v->a[v->n++] = (uint64_t)l << 3 | (uint64_t)c;
	return 0;
}

static int sink_fmd_words(void *data, int64_t n, const uint64_t *words, int64_t end) { return rb3h_fmdw_enc_words((rb3h_fmdw_t*)data, n, words, end); }

/* the .fmd of the index (rb3_enc_fmr2fmd + rld_dump, build.c:248-252): the data section is packed on the GPU (16-bit and
 * 32-bit block headers); if a block needs a 64-bit header or the device has no room for the packer, the GPU finds the runs
 * and the host packs them; the rank index is built here */
static int g_host_fmd = 0; /* --host-fmd */

static int write_fmd(rb3gpu_t *h, FILE *fp)
{
	rb3h_fmdw_t *w = rb3h_fmdw_init();
	uint64_t *words = 0;
	int64_t n_words = 0, acc[7];
	int ret;
	if (w == 0) return -1;
	ret = g_host_fmd ? RB3GPU_EUNSUP : rb3gpu_export_fmd_words(h, &words, &n_words);
	if (ret == 0) {
		rb3gpu_get_acc(h, acc);
		ret = rb3h_fmdw_adopt(w, words, n_words, acc); /* takes the array over */
		if (ret < 0) rb3gpu_host_free(words);
		else if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] packed the FMD on the GPU\n", __func__, rb3h_realtime(), rb3h_percent_cpu());
	} else if (ret != RB3GPU_ESTATE && ret != RB3GPU_EINVAL) { /* wider block headers needed, no room to pack the whole index at once -- or the packer gave up: the host's encoder takes the runs chunk by chunk */
		if (ret != RB3GPU_EUNSUP && ret != RB3GPU_ENOMEM && rb3h_verbose >= 2) fprintf(stderr, "[W::%s] the GPU's FMD packer failed (%s); encoding on the host\n", __func__, rb3gpu_strerror(ret));
		ret = rb3gpu_export_run_words(h, sink_fmd_words, w);
		if (ret == 0) ret = rb3h_fmdw_finish(w);
	}
	if (ret == 0) ret = rb3h_fmdw_dump(w, fp);
	rb3h_fmdw_destroy(w);
	return ret;
}
static int sink_fmr(void *data, int c, int64_t l) { return rb3h_fmrw_enc((rb3h_fmrw_t*)data, l, c); }

/* the .bre of the index (mr_print_bre, build.c:85-106): header, the records packed on the GPU, footer with the counts the device found; with
 * --host-fmd the GPU finds the runs and the host's packer writes the records */
static int g_bre_run_bytes = 2; /* --bre-run-bytes */

static int sink_bre_bytes(void *data, int64_t n, const uint8_t *bytes) { return fwrite(bytes, 1, (size_t)n, (FILE*)data) == (size_t)n ? 0 : -1; }
static int sink_bre_words(void *data, int64_t n, const uint64_t *words, int64_t end) { return rb3h_brew_enc_words((rb3h_brew_t*)data, n, words, end); }

static int write_bre_host(rb3gpu_t *h, rb3gpu_shard_t *sh, FILE *fp)
{
	rb3h_brew_t *w = rb3h_brew_init(fp, g_bre_run_bytes);
	int ret;
	if (w == 0) return -1;
	ret = sh ? rb3gpu_shard_export_run_words(sh, sink_bre_words, w) : rb3gpu_export_run_words(h, sink_bre_words, w);
	if (ret == 0) ret = rb3h_brew_finish(w);
	rb3h_brew_destroy(w);
	return ret;
}

static int write_bre(rb3gpu_t *h, FILE *fp)
{
	rb3gpu_bre_stats_t st;
	int ret;
	if (g_host_fmd) return write_bre_host(h, 0, fp);
	if (rb3h_bre_write_header(fp, g_bre_run_bytes) < 0) return -1;
	if ((ret = rb3gpu_export_bre(h, g_bre_run_bytes, sink_bre_bytes, fp, &st)) < 0) return ret;
	if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] packed %ld BRE records on the GPU\n", __func__, rb3h_realtime(), rb3h_percent_cpu(), (long)st.n_rec);
	return rb3h_bre_write_footer(fp, g_bre_run_bytes, st.n_rec, st.n_sym, st.n_run);
}

static int sink_plain(void *data, int c, int64_t l) /* mr_print_bwt, mrope.c:201-214 */
{
	FILE *fp = (FILE*)data;
	char buf[4096];
	memset(buf, "$ACGTN"[c], l < 4096 ? (size_t)l : 4096);
	while (l > 0) {
		size_t t = l < 4096 ? (size_t)l : 4096;
		if (fwrite(buf, 1, t, fp) != t) return -1;
		l -= (int64_t)t;
	}
	return 0;
}

static int iv_live(void);
static int iv_get_acc(int64_t acc[7]);
static int iv_export_runs(rb3gpu_emit_f sink, void *data);

/* the index as an FMR file -- from the handle, or, once --interval has cut it, from the intervals in rank order where they are
 * (-S after each input file, build.c:232-238, and the final -r output) */
static int dump_fmr(rb3gpu_t *h, const bopt_t *opt, FILE *fp)
{
	int64_t acc[7];
	rb3h_fmrw_t *w;
	int ret;
	if (iv_live()) iv_get_acc(acc);
	else rb3gpu_get_acc(h, acc);
	w = rb3h_fmrw_init(acc, opt->max_nodes, opt->block_len);
	if (w == 0) return -1;
	rb3h_fmrw_set_order(w, opt->so); /* mr_dump, mrope.c:155-156 */
	ret = iv_live() ? iv_export_runs(sink_fmr, w) : rb3gpu_export_runs(h, sink_fmr, w);
	if (ret == 0) ret = rb3h_fmrw_dump(w, fp);
	rb3h_fmrw_destroy(w);
	return ret;
}

/* the string order of an index file: byte 3 of an FMR header (mr_restore, mrope.c:170), input order for anything else */
static int index_order(const char *fn)
{
	FILE *fp = fopen(fn, "rb");
	unsigned char magic[4];
	int so = RB3GPU_SO_IO;
	if (fp == 0) return so; /* (load_index reports it) */
	if (fread(magic, 1, 4, fp) == 4 && memcmp(magic, "RB\2", 3) == 0 && magic[3] <= RB3GPU_SO_RCLO) so = magic[3];
	fclose(fp);
	return so;
}

/* an existing index into HBM (build.c:172-184, rb3_fmi_restore): an FMD file is decoded on the device
 * (rb3gpu_from_fmd_words); an FMR file, a stream, or an FMD the device declined goes through the host decoder */
/* an index file in host memory, before a device has seen it: the undecoded words of an FMD file (z != NULL) or the runs of any index file */
typedef struct { uint64_t *z; int64_t nw, mc[6]; runvec_t rv; rb3h_bre_t bre; } index_host_t; /* bre.rec != NULL: the raw records of a BRE file */

static void index_host_free(index_host_t *x)
{
	free(x->z); free(x->rv.a);
	rb3h_bre_free(&x->bre);
	x->z = 0, x->rv.a = 0, x->rv.n = x->rv.m = 0;
}

static int index_host_runs(const char *fn, index_host_t *x)
{
	if (rb3h_index_read_runs(fn, sink_runvec, &x->rv) < 0 || x->rv.n == 0) { index_host_free(x); return -1; }
	return 0;
}

/* ONE open of the file -- it may be a pipe, or stdin --, then by its magic: the records of a BRE file and the words of an FMD file stay as they are
 * for the device; an FMR file, anything with --host-fmd and an FMD on stdin (which the fallback of index_upload could not read again) become runs */
static int index_host_read(const char *fn, index_host_t *x)
{
	char magic[4];
	FILE *fp = rb3h_index_open(fn, magic);
	const int kind = fp ? rb3h_index_kind(magic) : RB3H_INDEX_NONE;
	int r;
	if (fp == 0) return -1;
	if (!g_host_fmd && kind == RB3H_INDEX_BRE) r = rb3h_bre_read_fp(fp, &x->bre) == 0 ? 0 : -1;
	else if (!g_host_fmd && kind == RB3H_INDEX_FMD && fp != stdin) {
		r = rb3h_fmd_read_words_fp(fp, &x->z, &x->nw, x->mc) == 0 ? 0 : -1;
		if (r != 0) x->z = 0;
	} else r = rb3h_index_read_runs_fp(fp, magic, sink_runvec, &x->rv) < 0 || x->rv.n == 0 ? -1 : 0;
	if (fp != stdin) fclose(fp);
	if (r != 0) index_host_free(x);
	return r;
}

/* the number of sentinels (acc[1]) and of symbols (acc[6]) of the index that was read */
static int64_t index_host_sentinels(const index_host_t *x, int64_t *n_sym)
{
	int64_t i, m = 0, n = 0;
	if (x->bre.rec) { /* (the footer's total; the sentinels are counted in the records) */
		const int rs = 1 + x->bre.b_per_run;
		for (i = 0; i < x->bre.n_rec; ++i)
			if (x->bre.rec[i * rs] == 0) { int j; uint64_t l = 0; for (j = 0; j < x->bre.b_per_run; ++j) l |= (uint64_t)x->bre.rec[i * rs + 1 + j] << (8 * j); m += (int64_t)l; }
		n = x->bre.ftr[1];
	} else if (x->z) {
		for (i = 0; i < 6; ++i) n += x->mc[i];
		m = x->mc[0];
	} else for (i = 0; i < x->rv.n; ++i) {
		n += (int64_t)(x->rv.a[i] >> 3);
		if ((x->rv.a[i] & 7) == 0) m += (int64_t)(x->rv.a[i] >> 3);
	}
	*n_sym = n;
	return m;
}

static int index_upload(rb3gpu_t *h, const char *fn, index_host_t *x)
{
	int r;
	if (x->bre.rec) {
		rb3gpu_bre_stats_t st;
		rb3gpu_tune(h, "verbose", 0); /* (the file may still be refused: the engine says nothing about it until its counts are accepted) */
		r = rb3gpu_from_bre(h, x->bre.b_per_run, x->bre.n_rec, x->bre.rec, &st);
		rb3gpu_tune(h, "verbose", rb3h_verbose);
		if (r == 0 && (st.n_rec != x->bre.ftr[0] || st.n_sym != x->bre.ftr[1] || st.n_run != x->bre.ftr[2])) r = RB3GPU_ESYMBOL; /* the footer disagrees with what the device counted */
		if (r == RB3GPU_ESYMBOL) { index_host_free(x); return -1; } /* not a valid file: the host decoder would say the same */
		if (r == 0) {
			if (rb3h_verbose >= 3)
				fprintf(stderr, "[M::%s::%.3f*%.2f] %ld BRE records of %d bytes unpacked on the GPU: %ld symbols in %ld runs (scan %.3f ms, fill %.3f ms, %ld piece%s)\n", __func__, rb3h_realtime(), rb3h_percent_cpu(),
						(long)st.n_rec, 1 + x->bre.b_per_run, (long)st.n_sym, (long)st.n_run, st.ms_scan, st.ms_fill, (long)st.n_pieces, st.n_pieces == 1 ? "" : "s");
			index_host_free(x);
			return 0;
		}
		if (rb3h_verbose >= 2) fprintf(stderr, "[W::%s] the GPU did not decode '%s' (%s); decoding it on the host\n", __func__, fn, rb3gpu_strerror(r));
		if (rb3h_bre_decode_runs(&x->bre, sink_runvec, &x->rv) < 0 || x->rv.n == 0) { index_host_free(x); return -1; }
		rb3h_bre_free(&x->bre);
	}
	if (x->z) {
		r = rb3gpu_from_fmd_words(h, x->nw, x->z, x->mc);
		free(x->z), x->z = 0;
		if (r == 0) return 0;
		if (rb3h_verbose >= 2) fprintf(stderr, "[W::%s] the GPU did not decode '%s' (%s); decoding it on the host\n", __func__, fn, rb3gpu_strerror(r));
		if (index_host_runs(fn, x) < 0) return -1;
	}
	r = rb3gpu_from_runs(h, x->rv.n, x->rv.a);
	index_host_free(x);
	return r < 0 ? -2 : 0;
}

static int load_index(rb3gpu_t *h, const char *fn)
{
	index_host_t x;
	memset(&x, 0, sizeof(x));
	if (index_host_read(fn, &x) < 0) return -1;
	return index_upload(h, fn, &x);
}

/* ---- what the query commands share (their batches come from rb3h_qbatch_read) -------------- */

/* a handle on --gpu `device` with the index `fn` in HBM; x != NULL: the index as index_host_read left it (`mem -p` has looked at it first).  NULL behind the command's one line */
static rb3gpu_t *open_index(int device, const char *fn, index_host_t *x)
{
	rb3gpu_opt_t gopt;
	rb3gpu_t *h;
	rb3gpu_opt_init(&gopt);
	gopt.device = device, gopt.verbose = rb3h_verbose;
	h = rb3gpu_create(&gopt);
	if (h == 0) { fprintf(stderr, "ERROR: no usable MI355X/HIP device; there is no CPU fallback\n"); return 0; }
	if ((x ? index_upload(h, fn, x) : load_index(h, fn)) < 0) {
		if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: failed to load index '%s'\n", fn);
		rb3gpu_destroy(h);
		return 0;
	}
	return h;
}

/* rb3_fmi_is_symmetric, fm-index.h:135, with the line of the commands that need both strands */
static int both_strands(const int64_t acc[7])
{
	if ((acc[1] & 1) == 0 && acc[2] - acc[1] == acc[5] - acc[4] && acc[3] - acc[2] == acc[4] - acc[3]) return 1;
	if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: BWT doesn't contain both strands\n");
	return 0;
}

/* `out` to stdout once it is past 1 MiB, or whatever it holds when forced; -1: the write failed */
static int out_flush(rb3h_buf_t *out, int force)
{
	int r = 0;
	if (out->l <= (1 << 20) && !force) return 0;
	if (out->l > 0 && fwrite(out->s, 1, (size_t)out->l, stdout) != (size_t)out->l) r = -1;
	out->l = 0;
	return r;
}

/* the two files beside an index, <fn>.ssa and <fn>.len.gz (rb3_fmi_load_all, fm-index.c:606-640): each NULL if it is not there or is no such file.
 * Whether they belong to the index, and whether they are needed, is the command's to say */
static void side_read(const char *fn, rb3h_ssa_t **sa, rb3h_sid_t **sid)
{
	const size_t l = strlen(fn);
	char *t = (char*)malloc(l + 8);
	*sa = 0, *sid = 0;
	if (t == 0) return;
	memcpy(t, fn, l);
	strcpy(t + l, ".ssa"), *sa = rb3h_ssa_read(t);
	strcpy(t + l, ".len.gz"), *sid = rb3h_sid_read(t);
	free(t);
}

/* ---- batches ----------------------------------------------------------------------------- */

typedef struct {
	int64_t n_seq, len, n_walkers, step;
	uint8_t *bwt;             /* host: the BWT, or the text if raw */
	rb3h_walker_t *walkers;
	int walkers_pinned;       /* the list lives in a buffer of the page-locked pool (pin_release, not free) */
	int ret, raw;             /* raw: not sorted yet, the consumer's GPU handle sorts it */
	void *d_bwt;              /* device: the BWT from a sorter thread's own GPU sorter (gs), to be released after the merge */
	void *d_tw;               /* device: its text-order words (long strings: the walkers are then given by text position) */
	void *d_sa;               /* device: its suffix array, behind them (the engine leaves its records in text order where that pays) */
	rb3gpu_sorter_t *gs;
	int64_t *sent, n_sent;    /* --interval: text positions of the batch's sentinels (where its LF chains start) */
} batch_t;

static int g_pin_on = 0; /* batch buffers (and walker lists) in page-locked memory */

/* The walker list goes to the device inside the merge call, between the LF kernels and the walkers: out of page-locked memory
 * that is one DMA; out of malloc'd memory the engine first copies it into its staging buffer while the device waits. */
static void walkers_pin(batch_t *b)
{
	int64_t cap = 0;
	const int64_t bytes = b->n_walkers * (int64_t)sizeof(rb3h_walker_t);
	void *p;
	if (!g_pin_on || b->walkers == 0 || b->walkers_pinned || bytes <= 0 || bytes > (16 << 20)) return;
	if ((p = pin_alloc(bytes, &cap)) == 0) return;
	memcpy(p, b->walkers, (size_t)bytes);
	free(b->walkers);
	b->walkers = (rb3h_walker_t*)p, b->walkers_pinned = 1;
}

static void walkers_free(batch_t *b)
{
	if (b->walkers_pinned) pin_release(b->walkers);
	else free(b->walkers);
	b->walkers = 0, b->walkers_pinned = 0;
}

/* --gpus N --interval: the index lives in N intervals on N devices from the second batch on (rb3gpu_shard_*, include/rb3gpu.h) */
static struct { int n, devices[RB3GPU_SH_MAXIV]; rb3gpu_shard_t *s; rb3gpu_opt_t gopt; double t_walk; int64_t rounds, batches; } g_iv;

static int64_t *sentinels_of(const uint8_t *text, int64_t len, int64_t n_hint, int64_t *n_out)
{
	int64_t n = 0, m = n_hint > 16 ? n_hint : 16, *a = (int64_t*)malloc((size_t)m * 8);
	const uint8_t *p = text, *end = text + len;
	while (a && p < end && (p = (const uint8_t*)memchr(p, 0, (size_t)(end - p))) != 0) {
		if (n == m) { int64_t *t = (int64_t*)realloc(a, (size_t)(m *= 2) * 8); if (t == 0) { free(a); a = 0; break; } a = t; }
		a[n++] = p - text, ++p;
	}
	*n_out = a ? n : 0;
	return a;
}

static int iv_live(void) { return g_iv.s != 0; }
static int iv_get_acc(int64_t acc[7]) { return rb3gpu_shard_get_acc(g_iv.s, acc); }
static int iv_export_runs(rb3gpu_emit_f sink, void *data) { return rb3gpu_shard_export_runs(g_iv.s, sink, data); }

/* one batch into the sharded index; the first call cuts the index the handle holds into its intervals */
static int interval_merge(rb3gpu_t *h, int64_t len, const void *d_bwt, const void *d_tw, int64_t n_sent, const int64_t *sent)
{
	int64_t rounds = 0;
	int r;
	const double t0 = rb3h_realtime();
	if (sent == 0 || n_sent <= 0 || d_tw == 0) return RB3GPU_EINVAL;
	if (rb3h_verbose >= 2) { /* one lock-step round per symbol of the longest string: say so before a batch of long strings takes minutes */
		int64_t i, longest = sent[0] + 1;
		for (i = 1; i < n_sent; ++i) if (sent[i] - sent[i - 1] > longest) longest = sent[i] - sent[i - 1];
		if (longest > 100000) fprintf(stderr, "WARNING: --interval walks a batch in lock step, one round (~20 us or more) per symbol of its longest string: %ld rounds for this batch; it is meant for reads (without --interval the strings are cut among many walkers)\n", (long)longest);
	}
	if (g_iv.s == 0) {
		if (rb3gpu_get_tot(h) < g_iv.n) return rb3gpu_merge_text_dev(h, len, (const uint8_t*)d_bwt, (const uint64_t*)d_tw, n_sent, 0, 1); /* (fewer symbols than intervals: not cut yet) */
		if ((g_iv.s = rb3gpu_shard_split(h, g_iv.n, g_iv.devices, &g_iv.gopt)) == 0) return RB3GPU_ENODEV;
		if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] index cut into %d intervals\n", "main_build", rb3h_realtime(), rb3h_percent_cpu(), g_iv.n);
	}
	r = rb3gpu_shard_merge(g_iv.s, len, (const uint8_t*)d_bwt, (const uint64_t*)d_tw, n_sent, sent, &rounds);
	g_iv.t_walk += rb3h_realtime() - t0, g_iv.rounds += rounds, ++g_iv.batches;
	return r;
}

/* --gpu-sort: the batch arrives as text; suffix sorting, BWT and inverse suffix array on the GPU
 * (rb3gpu_sort_text / rb3gpu_bwt_from_text instead of rb3_build_sais, build.c:220), the BWT never leaves HBM */
static int process_raw_batch(rb3gpu_t *h, batch_t *b, int *has_index)
{
	void *d_bwt = 0, *d_tw = 0;
	const int text_walk = *has_index; /* text-order words; long strings: walkers by text position, short ones: one walker per string */
	int ret;
	/* only "no room on the device" sends the batch to the host sorter (return 1); any other failure is an error of the build */
	if ((ret = rb3gpu_dev_alloc(h, b->len + 16, &d_bwt)) < 0) return ret == RB3GPU_ENOMEM ? 1 : ret;
	if (text_walk && (ret = rb3gpu_dev_alloc(h, b->len * 8, &d_tw)) < 0) { rb3gpu_dev_free(h, d_bwt); return ret == RB3GPU_ENOMEM ? 1 : ret; }
	if (text_walk) ret = rb3gpu_sort_text(h, b->len, b->bwt, (uint8_t*)d_bwt, (uint64_t*)d_tw);
	else ret = rb3gpu_bwt_from_text(h, b->len, b->bwt, (uint8_t*)d_bwt, 0, 0);
	if (ret == RB3GPU_ENOMEM) { /* the sorter's scratch did not fit: the caller sorts this batch on the host */
		if (d_tw) rb3gpu_dev_free(h, d_tw);
		rb3gpu_dev_free(h, d_bwt);
		return 1;
	}
	if (ret == 0) __sync_fetch_and_add(&g_sorted.n_gpu, 1), __sync_fetch_and_add(&g_sorted.sym_gpu, b->len);
	if (ret == 0 && rb3h_verbose >= 3)
		fprintf(stderr, "[M::%s::%.3f*%.2f] constructed partial BWT for %ld symbols on the GPU\n", "main_build", rb3h_realtime(), rb3h_percent_cpu(), (long)b->len);
	if (ret == 0 && !*has_index) ret = rb3gpu_from_plain_dev(h, b->len, (const uint8_t*)d_bwt);
	else if (ret == 0 && text_walk && g_iv.n > 1) {
		int64_t n_sent = 0, *sent = sentinels_of(b->bwt, b->len, b->n_seq, &n_sent);
		ret = sent ? interval_merge(h, b->len, d_bwt, d_tw, n_sent, sent) : RB3GPU_ENOMEM;
		free(sent);
	} else if (ret == 0 && text_walk) {
		if (b->step > 0) ret = rb3gpu_merge_text_step_dev(h, b->len, (const uint8_t*)d_bwt, (const uint64_t*)d_tw, 0, b->n_seq, b->step, 1); /* long strings: the walker list (one per string, one every `step` positions) is made on the device */
		else ret = rb3gpu_merge_text_dev(h, b->len, (const uint8_t*)d_bwt, (const uint64_t*)d_tw, b->n_seq, 0, 1); /* short strings: one walker per string */
	} else if (ret == 0) ret = rb3gpu_merge_plain_dev(h, b->len, (const uint8_t*)d_bwt, 1);
	if (d_tw) rb3gpu_dev_free(h, d_tw);
	rb3gpu_dev_free(h, d_bwt);
	return ret;
}

static int process_batch(rb3gpu_t *h, batch_t *b, int *has_index)
{
	int ret;
	if (b->d_bwt) { /* sorted on the GPU by a sorter thread while the batch before was being merged */
		const int first = !*has_index;
		if (first) ret = rb3gpu_from_plain_dev(h, b->len, (const uint8_t*)b->d_bwt);
		else if (g_iv.n > 1) ret = interval_merge(h, b->len, b->d_bwt, b->d_tw, b->n_sent, b->sent);
		else if (b->walkers && b->d_tw) ret = rb3gpu_merge_text_sa_dev(h, b->len, (const uint8_t*)b->d_bwt, (const uint64_t*)b->d_tw, (const uint32_t*)b->d_sa, b->n_walkers, (const rb3gpu_walker_t*)b->walkers, 1); /* (RB3_HOST_WALKERS: the list of rounds 2-4, made by the sorter thread) */
		else if (b->d_tw && b->step > 0 && b->n_seq > 0) ret = rb3gpu_merge_text_step_dev(h, b->len, (const uint8_t*)b->d_bwt, (const uint64_t*)b->d_tw, (const uint32_t*)b->d_sa, b->n_seq, b->step, 1); /* long strings: walker list made on the device */
		else if (b->d_tw && b->step == 0 && b->n_seq > 0) ret = rb3gpu_merge_text_sa_dev(h, b->len, (const uint8_t*)b->d_bwt, (const uint64_t*)b->d_tw, (const uint32_t*)b->d_sa, b->n_seq, 0, 1); /* short strings: one walker per string */
		else ret = rb3gpu_merge_plain_dev(h, b->len, (const uint8_t*)b->d_bwt, 1);
		rb3gpu_sorter_release(b->gs, b->d_bwt);
		b->d_bwt = b->d_tw = b->d_sa = 0;
		if (ret == 0 && rb3h_verbose >= 3)
			fprintf(stderr, "[M::%s::%.3f*%.2f] %s the partial BWT for %ld symbols\n", "main_build", rb3h_realtime(), rb3h_percent_cpu(), first ? "encoded" : "merged", (long)b->len);
	} else if (b->raw) {
		const int first = !*has_index;
		ret = process_raw_batch(h, b, has_index);
		if (ret == 1) { /* host sorter instead */
			if (g_order) {
				fprintf(stderr, "ERROR: the GPU could not take a batch of %ld symbols; -s/-r put batches into order on the GPU only\n", (long)b->len);
				return -1;
			}
			if (rb3h_verbose >= 2) fprintf(stderr, "[W::%s] the GPU suffix sorter could not take a batch of %ld symbols; sorting it on the host\n", "main_build", (long)b->len);
			ret = b->step > 0 ? rb3h_build_bwt_walkers(b->n_seq, b->len, b->bwt, 1, b->step, &b->n_walkers, &b->walkers) : rb3h_build_bwt(b->n_seq, b->len, b->bwt, 1);
			if (ret < 0) { fprintf(stderr, "ERROR: failed to construct the partial BWT (code %d)\n", ret); return -1; }
			b->raw = 0;
			return process_batch(h, b, has_index);
		}
		if (ret == 0 && rb3h_verbose >= 3)
			fprintf(stderr, "[M::%s::%.3f*%.2f] %s the partial BWT for %ld symbols\n", "main_build", rb3h_realtime(), rb3h_percent_cpu(), first ? "encoded" : "merged", (long)b->len);
	} else if (!*has_index) {
		ret = rb3gpu_from_plain(h, b->len, b->bwt);
		if (ret == 0 && rb3h_verbose >= 3)
			fprintf(stderr, "[M::%s::%.3f*%.2f] encoded the partial BWT for %ld symbols\n", "main_build", rb3h_realtime(), rb3h_percent_cpu(), (long)b->len);
	} else {
		/* long strings: hand over the sampled inverse suffix array as LF walkers (same result, text-regular
		 * parallelism); short strings (reads): one walker per string is what the engine does by itself */
		if (g_iv.s) { /* --interval and a batch the HOST had to sort (a record beyond the GPU sorter's limit, no device room): there are no text-order
		                 words to walk the intervals with, so the intervals go back into one handle, this batch is merged the ordinary way, and the
		                 next GPU-sorted batch cuts the index again (a long build must not die of one such batch) */
			const int r = rb3gpu_shard_gather(g_iv.s);
			g_iv.s = 0;
			if (r < 0) { fprintf(stderr, "ERROR: the GPU engine failed to put the intervals together for a host-sorted batch: %s\n", rb3gpu_strerror(r)); return -1; }
			if (rb3h_verbose >= 2) fprintf(stderr, "[W::%s] --interval: a host-sorted batch of %ld symbols is merged on one device; the index is cut again afterwards\n", "main_build", (long)b->len);
		}
		if (b->walkers) ret = rb3gpu_merge_plain_walkers(h, b->len, b->bwt, b->n_walkers, (const rb3gpu_walker_t*)b->walkers);
		else ret = rb3gpu_merge_plain(h, b->len, b->bwt);
		if (ret == 0 && rb3h_verbose >= 3)
			fprintf(stderr, "[M::%s::%.3f*%.2f] merged the partial BWT for %ld symbols\n", "main_build", rb3h_realtime(), rb3h_percent_cpu(), (long)b->len);
	}
	if (ret < 0) {
		fprintf(stderr, "ERROR: the GPU engine failed on a batch of %ld symbols: %s\n", (long)b->len, rb3gpu_strerror(ret));
		return ret;
	}
	*has_index = 1;
	return 0;
}

/* Pipeline (build.c:55-83, 186-201, generalised).  The reference overlaps the suffix sorting of batch
 * i+1 with the merge of batch i.  Here the merge takes milliseconds and the suffix sorter is the slow
 * stage, so `-p N` runs N sorter threads: one reader thread cuts the batches in input order, the
 * sorters work on N batches at once, and the calling thread feeds the GPU strictly in input order. */
typedef struct {
	rb3h_buf_t seq;      /* raw text of the batch */
	int64_t n_seq;
	batch_t *out;        /* sorted batch */
	int state;           /* 0 free, 1 raw, 2 being sorted, 3 ready (or an end-of-file marker), */
	int end_of_file, err;
} job_t;

typedef struct {
	pthread_mutex_t mtx;
	pthread_cond_t cv;
	job_t *ring;
	int cap;
	int64_t head, tail, next_sort; /* next to consume / to fill / to sort */
	int reader_done;
	const bopt_t *opt;
	int device;
} pool_t;

static int sort_batch(const bopt_t *opt, int device, rb3h_buf_t *seq, int64_t n_seq, int n_threads, batch_t **out, rb3gpu_sorter_t *gs)
{
	batch_t *b;
	int64_t n_walkers = 0;
	rb3h_walker_t *walkers = 0;
	/* walkers inside long strings: as many as the walker kernel keeps resident on the GPU (rb3gpu_walker_step), or every 2^k positions (-k) */
	int64_t step = opt->split_log2 > 0 ? 1LL << opt->split_log2 : rb3gpu_walker_step(device, seq->l, n_seq); /* (the device of this slice: --gpus N) */
	int r;
	if (step < 192 && opt->split_log2 <= 0) step = 384; /* (no such device: the merge will say so) */
	if (step < (seq->l >> 20)) step = seq->l >> 20; /* at most ~2^20 walkers per batch: the engine's stretch table is finite */
	if (opt->gpu_sort && seq->l < opt->gpu_sort_limit) { /* the GPU sorts (its sorter handles < 2^31 symbols; batches are cut to fit, see batch_cut) */
		b = (batch_t*)calloc(1, sizeof(batch_t)); /* (counted in g_sorted where the sort really happens: below, or in process_batch) */
		b->n_seq = n_seq, b->len = seq->l, b->bwt = seq->s, b->raw = 1;
		b->step = (opt->split_log2 >= 0 && n_seq > 0 && seq->l / n_seq > 4 * step && seq->l / step + n_seq < (1 << 22)) ? step : 0;
		seq->s = 0, seq->l = seq->m = 0;
		if (gs) { /* this thread has a GPU sorter of its own: sort now, while the consumer merges the batch before */
			/* long strings: also the text-order words, and LF walkers by text position (same result, text-regular parallelism);
			 * short strings (reads): one walker per string is what the engine does by itself */
			/* a few long records on both strands: only the forward strands cross PCIe, the reverse complements are made on the device */
			int64_t pair_start[32], n_pairs = 0;
			int r2 = -1;
			if (!(opt->flag & (BF_NO_FOR | BF_NO_REV))) n_pairs = rb3h_strand_pairs(b->len, b->bwt, n_seq, 32, pair_start);
			if (n_pairs > 0 && (r2 = rb3gpu_sorter_upload_fwd(gs, b->len, b->bwt, n_pairs, pair_start)) == 0)
				r2 = rb3gpu_sorter_sort_uploaded_sa(gs, b->len, &b->d_bwt, &b->d_tw, &b->d_sa);
			if (n_pairs <= 0 || r2 == RB3GPU_EINVAL) r2 = rb3gpu_sorter_sort_sa(gs, b->len, b->bwt, &b->d_bwt, &b->d_tw, &b->d_sa);
			if (r2 == 0) {
				if (rb3h_verbose >= 3)
					fprintf(stderr, "[M::%s::%.3f*%.2f] constructed partial BWT for %ld symbols on the GPU\n", "main_build", rb3h_realtime(), rb3h_percent_cpu(), (long)b->len);
				if (b->step > 0 && !g_order && getenv("RB3_HOST_WALKERS") && rb3h_walkers_text(b->len, b->bwt, b->step, &b->n_walkers, &b->walkers) < 0) b->walkers = 0, b->n_walkers = 0; /* (experiments: the host's list) */
				walkers_pin(b);
				b->gs = gs, b->raw = 0; /* (the walker list of a batch of long strings is made on the device, inside the merge call: b->n_seq and b->step say how) */
				if (opt->interval) b->sent = sentinels_of(b->bwt, b->len, n_seq, &b->n_sent);
				__sync_fetch_and_add(&g_sorted.n_gpu, 1), __sync_fetch_and_add(&g_sorted.sym_gpu, b->len);
				rb3h_batch_free(b->bwt); b->bwt = 0; /* the text is not needed any more */
			} else b->d_bwt = b->d_tw = b->d_sa = 0; /* leave it to the consumer (its handle's sorter, then the host sorter) */
		}
		*out = b;
		return 0;
	}
	if (g_order) { /* (a record longer than the GPU sorter takes) */
		fprintf(stderr, "ERROR: a batch of %ld symbols is beyond the GPU sorter; -s/-r put batches into order on the GPU only\n", (long)seq->l);
		return -1;
	}
	__sync_fetch_and_add(&g_sorted.n_host, 1), __sync_fetch_and_add(&g_sorted.sym_host, seq->l);
	if (opt->split_log2 >= 0 && n_seq > 0 && seq->l / n_seq > 4 * step && seq->l / step + n_seq < (1 << 22))
		r = rb3h_build_bwt_walkers(n_seq, seq->l, seq->s, n_threads, step, &n_walkers, &walkers);
	else r = rb3h_build_bwt(n_seq, seq->l, seq->s, n_threads);
	if (r < 0) {
		fprintf(stderr, "ERROR: failed to construct the partial BWT (code %d)\n", r);
		return -1;
	}
	if (rb3h_verbose >= 3)
		fprintf(stderr, "[M::%s::%.3f*%.2f] constructed partial BWT for %ld symbols\n", "main_build", rb3h_realtime(), rb3h_percent_cpu(), (long)seq->l);
	b = (batch_t*)calloc(1, sizeof(batch_t));
	b->n_seq = n_seq, b->len = seq->l, b->bwt = seq->s, b->n_walkers = n_walkers, b->walkers = walkers;
	seq->s = 0, seq->l = seq->m = 0; /* ownership moves to the batch */
	*out = b;
	return 0;
}

/* what to do with a freshly cut batch (raw text in *seq, ownership passes) or an end-of-file event */
typedef int (*submit_f)(void *data, rb3h_buf_t *seq, int64_t n_seq, int end_of_file);

/* read every input file, cutting batches as io.c:104-125 does */
/* rbeg / rend (NULL: whole files): the byte range of file i whose records this reader takes (`build --gpus N`: slices cut inside files) */
static int for_each_batch(const bopt_t *opt, int n_files, char **files, const int64_t *rbeg, const int64_t *rend, submit_f submit, void *data, int64_t *n_empty)
{
	rb3h_buf_t seq = {0, 0, 0};
	int64_t n_seq_acc = 0;
	int i, ret = 0;
	for (i = 0; i < n_files && ret == 0; ++i) {
		rb3h_seqio_t *fp = rbeg ? rb3h_seq_open_range(files[i], !!(opt->flag & BF_LINE), rbeg[i], rend[i]) : rb3h_seq_open(files[i], !!(opt->flag & BF_LINE));
		int64_t n_seq;
		if (fp == 0) {
			if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: failed to open file '%s'\n", files[i]);
			continue; /* build.c:208-211 */
		}
		for (;;) {
			const int64_t l0 = seq.l;
			n_seq = rb3h_seq_read(fp, &seq, batch_cut(opt), !(opt->flag & BF_NO_FOR), !(opt->flag & BF_NO_REV), n_empty);
			if (n_seq < 0) {
				if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: failed to read sequences from '%s' (code %ld)\n", files[i], (long)n_seq);
				ret = -1; /* (an I/O error in mid-file or no memory: indexing the prefix read so far would be a silently wrong index) */
				break;
			}
			if (rb3h_seq_error(fp) && seq.l != l0 && rb3h_verbose >= 1) /* the records before the error are indexed, as in io.c:121-124 */
				fprintf(stderr, "ERROR: FASTX parsing error (code %d)\n", rb3h_seq_error(fp));
			if (n_seq == 0 && seq.l == l0) break; /* EOF */
			n_seq_acc += n_seq;
			if (rb3h_verbose >= 3)
				fprintf(stderr, "[M::%s::%.3f*%.2f] read %ld symbols from file '%s'\n", "main_build", rb3h_realtime(), rb3h_percent_cpu(), (long)(seq.l - l0), files[i]);
			if (opt->rebatch && !(batch_cut(opt) > 0 && seq.l > batch_cut(opt))) break; /* keep filling from the next file */
			if ((ret = submit(data, &seq, n_seq_acc, 0)) != 0) break;
			n_seq_acc = 0;
		}
		rb3h_seq_close(fp);
		if (ret == 0 && !(opt->rebatch && seq.l > 0)) ret = submit(data, 0, 0, 1); /* end of file i */
	}
	if (ret == 0 && seq.l > 0) { /* the last, partly filled re-batched batch */
		if ((ret = submit(data, &seq, n_seq_acc, 0)) == 0) ret = submit(data, 0, 0, 1);
	}
	rb3h_batch_free(seq.s);
	return ret;
}

typedef struct {
	rb3gpu_t *h;
	const bopt_t *opt;
	int has_index;
	const char *fn_tmp;
	int device;
} consumer_t;

static int consume(consumer_t *c, batch_t *b, int end_of_file)
{
	if (b) {
		int r = process_batch(c->h, b, &c->has_index);
		rb3h_batch_free(b->bwt); walkers_free(b); free(b->sent); free(b);
		if (r < 0) return r;
	}
	if (end_of_file && c->fn_tmp && c->has_index) { /* build.c:232-238 */
		FILE *fp = fopen(c->fn_tmp, "wb");
		if (fp != 0) {
			dump_fmr(c->h, c->opt, fp);
			fclose(fp);
			if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] saved the current index to '%s'\n", "main_build", rb3h_realtime(), rb3h_percent_cpu(), c->fn_tmp);
		}
	}
	return 0;
}

/* serial mode: sort and merge on the calling thread */
static int submit_serial(void *data, rb3h_buf_t *seq, int64_t n_seq, int end_of_file)
{
	consumer_t *c = (consumer_t*)data;
	batch_t *b = 0;
	if (seq && sort_batch(c->opt, c->device, seq, n_seq, c->opt->n_threads, &b, 0) < 0) return -1;
	return consume(c, b, end_of_file);
}

/* pipelined mode: the reader thread queues raw batches */
static int submit_pool(void *data, rb3h_buf_t *seq, int64_t n_seq, int end_of_file)
{
	pool_t *q = (pool_t*)data;
	job_t *j;
	pthread_mutex_lock(&q->mtx);
	while (q->tail - q->head >= q->cap) pthread_cond_wait(&q->cv, &q->mtx);
	j = &q->ring[q->tail % q->cap];
	memset(j, 0, sizeof(*j));
	if (seq) j->seq = *seq, j->n_seq = n_seq, j->state = 1, seq->s = 0, seq->l = seq->m = 0;
	else j->state = 3, j->end_of_file = 1;
	(void)end_of_file;
	++q->tail;
	pthread_cond_broadcast(&q->cv);
	pthread_mutex_unlock(&q->mtx);
	return 0;
}

typedef struct { pool_t *q; int n_files; char **files; const int64_t *rbeg, *rend; int64_t n_empty; int err; } reader_t;

static void *reader_main(void *arg)
{
	reader_t *r = (reader_t*)arg;
	r->err = for_each_batch(r->q->opt, r->n_files, r->files, r->rbeg, r->rend, submit_pool, r->q, &r->n_empty);
	pthread_mutex_lock(&r->q->mtx);
	r->q->reader_done = 1;
	pthread_cond_broadcast(&r->q->cv);
	pthread_mutex_unlock(&r->q->mtx);
	return 0;
}

typedef struct { pool_t *q; rb3gpu_sorter_t *gs; } sorter_arg_t;

static void *sorter_main(void *arg)
{
	pool_t *q = ((sorter_arg_t*)arg)->q;
	rb3gpu_sorter_t *gs = ((sorter_arg_t*)arg)->gs;
	for (;;) {
		job_t *j = 0;
		pthread_mutex_lock(&q->mtx);
		for (;;) {
			while (q->next_sort < q->tail && q->ring[q->next_sort % q->cap].state != 1) ++q->next_sort; /* markers */
			if (q->next_sort < q->tail) { j = &q->ring[q->next_sort % q->cap]; j->state = 2; ++q->next_sort; break; }
			if (q->reader_done) break;
			pthread_cond_wait(&q->cv, &q->mtx);
		}
		pthread_mutex_unlock(&q->mtx);
		if (j == 0) return 0;
		{
			batch_t *b = 0;
			int err = sort_batch(q->opt, q->device, &j->seq, j->n_seq, 1, &b, gs);
			pthread_mutex_lock(&q->mtx);
			j->out = b, j->err = err, j->state = 3;
			pthread_cond_broadcast(&q->cv);
			pthread_mutex_unlock(&q->mtx);
		}
	}
}

/* one slice of the input on one GPU: reader thread -> sorter thread(s) -> merges, in input order (build.c:186-239).  A build on
 * one GPU is one slice; `--gpus N` runs N of them side by side, one per device, and merges their indexes afterwards. */
typedef struct {
	rb3gpu_t *h;
	const bopt_t *opt;
	int device, n_files, has_index, ret;
	char **files;
	const int64_t *rbeg, *rend; /* NULL: whole files; else the byte range of every file whose records belong to this slice */
	const char *fn_tmp;
	int64_t n_empty;
	rb3gpu_sorter_t *old_sorters[4];
	int n_old_sorters;
} slice_t;

static void *run_slice(void *arg)
{
	slice_t *sl = (slice_t*)arg;
	const bopt_t *opt = sl->opt;
	rb3gpu_t *h = sl->h;
	int ret = 0, has_index = sl->has_index;
	int64_t n_empty = 0;
	const char *fn_tmp = sl->fn_tmp;
	rb3gpu_sorter_t **old_sorters = sl->old_sorters;
	int n_old_sorters = 0;
	const int argc = sl->n_files, optind = 0;
	char **argv = sl->files;
	if (opt->sais_threads > 0 && argc - optind >= 1) { /* N suffix sorters ahead of the GPU merge */
		pool_t q;
		reader_t rd;
		pthread_t rt, *st;
		consumer_t cs = { h, opt, has_index, fn_tmp, sl->device };
		int k, n_sort = opt->sais_threads;
		sorter_arg_t *sa;
		if (opt->gpu_sort && n_sort > 3) n_sort = 3; /* GPU sorters: more than a few at once only compete for the same GPU */
		memset(&q, 0, sizeof(q));
		pthread_mutex_init(&q.mtx, 0);
		pthread_cond_init(&q.cv, 0);
		q.cap = n_sort + 2, q.ring = (job_t*)calloc((size_t)q.cap, sizeof(job_t)), q.opt = opt, q.device = sl->device;
		memset(&rd, 0, sizeof(rd));
		rd.q = &q, rd.n_files = argc - optind, rd.files = argv + optind, rd.rbeg = sl->rbeg, rd.rend = sl->rend;
		st = (pthread_t*)calloc((size_t)n_sort, sizeof(pthread_t));
		sa = (sorter_arg_t*)calloc((size_t)n_sort, sizeof(sorter_arg_t));
		pthread_create(&rt, 0, reader_main, &rd);
		for (k = 0; k < n_sort; ++k) {
			sa[k].q = &q, sa[k].gs = opt->gpu_sort ? rb3gpu_sorter_create(sl->device) : 0; /* NULL: the consumer's handle sorts */
			if (sa[k].gs && opt->so) rb3gpu_sorter_set_order(sa[k].gs, opt->so); /* every batch into the build's string order before it is sorted */
			pthread_create(&st[k], 0, sorter_main, &sa[k]);
		}
		for (;;) {
			job_t j;
			pthread_mutex_lock(&q.mtx);
			while (!(q.head < q.tail && q.ring[q.head % q.cap].state == 3) && !(q.reader_done && q.head == q.tail))
				pthread_cond_wait(&q.cv, &q.mtx);
			if (q.head == q.tail) { pthread_mutex_unlock(&q.mtx); break; }
			j = q.ring[q.head % q.cap];
			q.ring[q.head % q.cap].state = 0;
			++q.head;
			pthread_cond_broadcast(&q.cv);
			pthread_mutex_unlock(&q.mtx);
			if (j.err != 0) ret = -1;
			if (ret == 0) ret = consume(&cs, j.out, j.end_of_file);
			else if (j.out) {
				if (j.out->d_bwt) rb3gpu_sorter_release(j.out->gs, j.out->d_bwt);
				rb3h_batch_free(j.out->bwt); walkers_free(j.out); free(j.out->sent); free(j.out);
			}
		}
		pthread_join(rt, 0);
		for (k = 0; k < n_sort; ++k) pthread_join(st[k], 0);
		for (k = 0; k < n_sort; ++k) {
			double up = 0, so = 0, om = 0;
			if (sa[k].gs && rb3gpu_sorter_stats(sa[k].gs, &up, &so, 0, 0) == 0) {
				rb3gpu_sorter_order_stats(sa[k].gs, &om);
				pthread_mutex_lock(&g_sorted_mtx);
				g_sorted.ms_upload += up, g_sorted.ms_sort += so, g_sorted.ms_order += om;
				pthread_mutex_unlock(&g_sorted_mtx);
			}
			/* the sorters' scratch (tens of bytes per symbol of a batch) is given back AFTER the index has been written: freeing
			 * gigabytes here made the next device allocation -- the run list of the FMD export -- wait for up to 1.4 s */
			if (sa[k].gs && n_old_sorters < 4) old_sorters[n_old_sorters++] = sa[k].gs;
			else rb3gpu_sorter_destroy(sa[k].gs);
		}
		free(st); free(sa); free(q.ring);
		if (rd.err != 0) ret = -1;
		n_empty = rd.n_empty, has_index = cs.has_index;
	} else if (argc - optind >= 1) {
		consumer_t cs = { h, opt, has_index, fn_tmp, sl->device };
		ret = for_each_batch(opt, argc - optind, argv + optind, sl->rbeg, sl->rend, submit_serial, &cs, &n_empty);
		has_index = cs.has_index;
	}
	sl->ret = ret, sl->has_index = has_index, sl->n_empty = n_empty, sl->n_old_sorters = n_old_sorters;
	return 0;
}

static const struct option long_opts[] = {
	{ "gpu", required_argument, 0, 301 },
	{ "split", required_argument, 0, 302 },
	{ "rebatch", no_argument, 0, 303 },
	{ "gpu-sort", no_argument, 0, 304 },
	{ "host-sort", no_argument, 0, 305 },
	{ "gpu-batch", required_argument, 0, 306 },
	{ "gpu-sort-limit", required_argument, 0, 307 }, /* (tests: pretend the GPU sorter takes less than it does) */
	{ "host-fmd", no_argument, 0, 308 },
	{ "gpus", required_argument, 0, 309 },
	{ "interval", no_argument, 0, 310 },
	{ "bre-run-bytes", required_argument, 0, 311 },
	{ 0, 0, 0, 0 }
};

int main_build(int argc, char *argv[])
{
	bopt_t opt;
	int c, ret = 0, has_index = 0;
	char *fn_in = 0, *fn_tmp = 0;
	rb3gpu_t *h;
	rb3gpu_opt_t gopt;
	int64_t n_empty = 0;
	rb3gpu_sorter_t *old_sorters[4];
	int n_old_sorters = 0;

	bopt_init(&opt);
	optind = 1;
	while ((c = getopt_long(argc, argv, "l:n:m:t:2sri:LFRo:dbTS:p:e", long_opts, 0)) >= 0) {
		if (c == 'm') opt.batch_size = rb3h_parse_num(optarg);
		else if (c == 't') opt.n_threads = atoi(optarg);
		else if (c == 'p') opt.sais_threads = atoi(optarg);
		else if (c == 'l') opt.block_len = atoi(optarg);
		else if (c == 'n') opt.max_nodes = atoi(optarg);
		else if (c == 's') opt.so = RB3GPU_SO_RLO;
		else if (c == 'r') opt.so = RB3GPU_SO_RCLO;
		else if (c == '2') {
			fprintf(stderr, "ERROR: -%c selects the ropebwt2 insertion algorithm, which this build does not include; the default (suffix sorting + merge) gives the same BWT for -2\n", c);
			return 1;
		} else if (c == 'T') {
			fprintf(stderr, "ERROR: output format -%c is not available in this build; use -d (FMD), -b (FMR) or the default plain text\n", c);
			return 1;
		} else if (c == 'e') opt.fmt = FMT_BRE;
		else if (c == 311) g_bre_run_bytes = atoi(optarg);
		else if (c == 'i') fn_in = optarg;
		else if (c == 'L') opt.flag |= BF_LINE;
		else if (c == 'F') opt.flag |= BF_NO_FOR;
		else if (c == 'R') opt.flag |= BF_NO_REV;
		else if (c == 'o') { if (freopen(optarg, "wb", stdout) == 0) { fprintf(stderr, "ERROR: failed to write to '%s'\n", optarg); return 1; } }
		else if (c == 'd') opt.fmt = FMT_FMD;
		else if (c == 'b') opt.fmt = FMT_FMR;
		else if (c == 'S') fn_tmp = optarg;
		else if (c == 301) opt.device = atoi(optarg);
		else if (c == 302) opt.split_log2 = atoi(optarg);
		else if (c == 303) opt.rebatch = 1;
		else if (c == 304) opt.gpu_sort = 1;
		else if (c == 305) opt.gpu_sort = 0;
		else if (c == 306) opt.gpu_batch = rb3h_parse_num(optarg);
		else if (c == 307) opt.gpu_sort_limit = rb3h_parse_num(optarg);
		else if (c == 308) opt.host_fmd = g_host_fmd = 1;
		else if (c == 309) opt.n_gpus = atoi(optarg);
		else if (c == 310) opt.interval = 1;
		else if (c == '?') return 1;
	}
	if (opt.gpu_sort_limit > (int64_t)INT32_MAX - 16) opt.gpu_sort_limit = (int64_t)INT32_MAX - 16;
	if (opt.gpu_batch <= 0 || opt.gpu_batch > opt.gpu_sort_limit - 1) opt.gpu_batch = opt.gpu_sort_limit - 1;
	if (argc == optind && fn_in == 0) return usage_build(stderr, &opt);
	if (g_bre_run_bytes < 1 || g_bre_run_bytes > 4) {
		fprintf(stderr, "ERROR: --bre-run-bytes takes 1 to 4\n");
		return 1;
	}
	if ((opt.flag & BF_NO_FOR) && (opt.flag & BF_NO_REV)) {
		fprintf(stderr, "ERROR: -F and -R together leave nothing to index\n");
		return 1;
	}
	if (opt.so) { /* -s / -r: a sorted string order (build.c:146-219 decides which one the build really uses) */
		if (opt.n_gpus > 1 || opt.interval || !opt.gpu_sort) {
			fprintf(stderr, "ERROR: -%c is available with GPU suffix sorting on one GPU only (not with --gpus, --interval or --host-sort)\n", opt.so == RB3GPU_SO_RLO ? 's' : 'r');
			return 1;
		}
		if (fn_in && strcmp(fn_in, "-") == 0) { /* (the order of an index on stdin is in its header: not read twice here) */
			fprintf(stderr, "ERROR: -%c needs the index of -i in a file, not on stdin\n", opt.so == RB3GPU_SO_RLO ? 's' : 'r');
			return 1;
		}
		if (fn_in) opt.so = index_order(fn_in); /* -i: the order of that index (an FMR's header byte 3; an FMD is in input order) */
		if (argc - optind == 1 && opt.sais_threads > 0 && opt.n_threads - opt.sais_threads > 0) opt.so = RB3GPU_SO_IO; /* the reference's pipeline (build.c:178, 55-83) merges in input order */
	}
	g_order = opt.so;

	rb3gpu_opt_init(&gopt);
	gopt.device = opt.device, gopt.split_log2 = opt.split_log2, gopt.verbose = rb3h_verbose;
	h = rb3gpu_create(&gopt);
	if (h == 0) {
		fprintf(stderr, "ERROR: no usable MI355X/HIP device (device %d); the merge path has no CPU fallback\n", opt.device);
		return 1;
	}
	if (opt.so) rb3gpu_set_order(h, opt.so);

	if (getenv("RB3_PINNED_LIMIT")) g_pin_limit = atoll(getenv("RB3_PINNED_LIMIT"));
	if (!getenv("RB3_NO_PINNED")) g_pin_on = 1, rb3h_seq_set_batch_allocator(pin_alloc, pin_release); /* batch buffers in page-locked memory (one DMA per batch) */

	if (fn_in) { /* build.c:172-184 */
		const int r = load_index(h, fn_in);
		if (r == -1) {
			if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: failed to open index file '%s'\n", fn_in);
			rb3gpu_destroy(h);
			return 1;
		}
		if (r < 0) {
			fprintf(stderr, "ERROR: failed to load the index into HBM\n");
			rb3gpu_destroy(h);
			return 1;
		}
		has_index = 1;
		if (rb3h_verbose >= 3) {
			rb3gpu_stats_t st;
			rb3gpu_stats(h, &st);
			fprintf(stderr, "[M::%s::%.3f*%.2f] loaded the index from file '%s' (index %.1f MB in HBM, peak device memory while loading %.1f MB)\n", __func__, rb3h_realtime(), rb3h_percent_cpu(), fn_in, st.bytes_index / 1e6, st.bytes_peak / 1e6);
		}
	}

	if (opt.sais_threads < 0) opt.sais_threads = opt.gpu_sort ? 1 : 0; /* one batch sorted on the GPU while the one before is merged */
	if (opt.n_gpus < 1) opt.n_gpus = 1;
	/* Slices: contiguous pieces of the input in input order, equal in bytes, cut INSIDE files at record boundaries where every file
	 * can be read from an offset (regular files that are not gzip-compressed: a reads file of config 4 shards over all GPUs, each
	 * with its own reader and sorter, as kt_for spreads the chains of a batch, fm-index.c:217-224); with a pipe or a .gz among the
	 * inputs the slices are whole files. */
	int64_t *fsize = 0, total_bytes = 0;
	memset(&g_iv, 0, sizeof(g_iv));
	if (opt.interval && opt.n_gpus > 1) { /* ONE reader / sorter / consumer; the index is what is spread over the GPUs (north_star's split) */
		const int ndev = rb3gpu_device_count();
		if (!opt.gpu_sort || opt.n_gpus > RB3GPU_SH_MAXIV) { /* (-S works: the FMR writer takes the intervals where they are, see dump_fmr) */
			fprintf(stderr, "ERROR: --interval needs GPU suffix sorting and at most %d GPUs\n", RB3GPU_SH_MAXIV);
			rb3gpu_destroy(h);
			return 1;
		}
		g_iv.n = opt.n_gpus, g_iv.gopt = gopt;
		for (c = 0; c < g_iv.n; ++c) g_iv.devices[c] = (opt.device + c) % (ndev > 0 ? ndev : 1);
		opt.n_gpus = 1;
	}
	int by_bytes = opt.n_gpus > 1 && argc - optind >= 1;
	if (by_bytes) {
		fsize = (int64_t*)calloc((size_t)(argc - optind), sizeof(int64_t));
		for (c = 0; c < argc - optind && by_bytes; ++c) {
			if (!rb3h_seq_splittable(argv[optind + c], &fsize[c])) by_bytes = 0;
			else total_bytes += fsize[c];
		}
		if (total_bytes < (int64_t)opt.n_gpus * 64) by_bytes = 0; /* (nothing to cut) */
	}
	if (!by_bytes && opt.n_gpus > argc - optind) opt.n_gpus = argc - optind > 0 ? argc - optind : 1; /* slices are cut at file boundaries */
	if (opt.n_gpus > 1 && fn_tmp) { fprintf(stderr, "ERROR: -S (save after each file) is not available with --gpus\n"); rb3gpu_destroy(h); return 1; }
	if (opt.n_gpus == 1) {
		slice_t sl;
		memset(&sl, 0, sizeof(sl));
		sl.h = h, sl.opt = &opt, sl.device = opt.device, sl.rbeg = sl.rend = 0, sl.n_files = argc - optind, sl.files = argv + optind, sl.has_index = has_index, sl.fn_tmp = fn_tmp;
		run_slice(&sl);
		ret = sl.ret, has_index = sl.has_index, n_empty = sl.n_empty;
		for (c = 0; c < sl.n_old_sorters && n_old_sorters < 4; ++c) old_sorters[n_old_sorters++] = sl.old_sorters[c];
	} else { /* partitioned build: slice k of the files on device (--gpu + k) mod #devices, then a binary tree of whole-index merges */
		const int N = opt.n_gpus, ndev = rb3gpu_device_count(), nf = argc - optind;
		slice_t *sl = (slice_t*)calloc((size_t)N, sizeof(slice_t));
		pthread_t *th = (pthread_t*)calloc((size_t)N, sizeof(pthread_t));
		int k, stride;
		double t_tree;
		int64_t *rb = by_bytes ? (int64_t*)calloc((size_t)N * nf * 2, sizeof(int64_t)) : 0; /* per slice: begin and end offset in every file */
		for (k = 0; k < N && ret == 0; ++k) {
			int f0 = (int)((int64_t)nf * k / N), f1 = (int)((int64_t)nf * (k + 1) / N);
			if (by_bytes) { /* global byte range [lo, hi) of the concatenated inputs -> the files it touches and the range inside each */
				const int64_t lo = total_bytes / N * k, hi = k + 1 == N ? total_bytes : total_bytes / N * (k + 1);
				int64_t at = 0, *b = rb + (size_t)k * nf * 2, *e = b + nf;
				f0 = nf, f1 = 0;
				for (c = 0; c < nf; at += fsize[c], ++c) {
					const int64_t x0 = lo > at ? lo - at : 0, x1 = hi - at < fsize[c] ? hi - at : fsize[c];
					if (x1 <= x0 && !(fsize[c] == 0 && at >= lo && at < hi)) continue; /* (file c has nothing for this slice) */
					b[c] = x0, e[c] = x1 >= fsize[c] ? 0 : x1; /* (0: to the end of the file) */
					if (c < f0) f0 = c;
					f1 = c + 1;
				}
				if (f0 >= f1) f0 = f1 = 0;
				sl[k].rbeg = b + f0, sl[k].rend = e + f0;
			}
			sl[k].opt = &opt, sl[k].device = (opt.device + k) % (ndev > 0 ? ndev : 1), sl[k].n_files = f1 - f0, sl[k].files = argv + optind + f0;
			if (k == 0) sl[k].h = h, sl[k].has_index = has_index; /* (an index given with -i is the start of slice 0) */
			else {
				gopt.device = sl[k].device;
				sl[k].h = rb3gpu_create(&gopt);
				if (sl[k].h == 0) { fprintf(stderr, "ERROR: no usable HIP device %d for slice %d\n", sl[k].device, k); ret = -1; }
			}
		}
		if (ret == 0) {
			for (k = 0; k < N; ++k) pthread_create(&th[k], 0, run_slice, &sl[k]);
			for (k = 0; k < N; ++k) {
				pthread_join(th[k], 0);
				if (sl[k].ret != 0) ret = -1; /* (a slice whose files held nothing has no index: skipped below, as the reference skips such files, build.c:208-211) */
				n_empty += sl[k].n_empty;
				for (c = 0; c < sl[k].n_old_sorters; ++c) rb3gpu_sorter_destroy(sl[k].old_sorters[c]); /* (their scratch must not sit on the devices during the tree merge) */
			}
		}
		if (ret == 0 && rb3h_verbose >= 3)
			fprintf(stderr, "[M::%s::%.3f*%.2f] %d slices indexed on %d GPUs\n", __func__, rb3h_realtime(), rb3h_percent_cpu(), N, ndev < N ? ndev : N);
		t_tree = rb3h_realtime();
		{ /* the slices that hold an index, in input order (one whose files held nothing is skipped, as the single-GPU build and the reference skip such files) */
			int *live = (int*)calloc((size_t)N, sizeof(int)), nl = 0;
			for (k = 0; k < N; ++k) if (sl[k].has_index) live[nl++] = k;
			for (stride = 1; stride < nl && ret == 0; stride *= 2) /* merge(A, B) ranks the sentinels of B after those of A (fm-index.c:147): adjacent slices, left to right */
				for (k = 0; k + stride < nl && ret == 0; k += 2 * stride) { /* (the merges of one level are independent; they are short next to the slices and run in turn) */
					const int a = live[k], b = live[k + stride];
					const int r = rb3gpu_merge_index(sl[a].h, sl[b].h);
					if (r < 0) { fprintf(stderr, "ERROR: the GPU engine failed to merge the index of slice %d into slice %d: %s\n", b, a, rb3gpu_strerror(r)); ret = -1; }
					else {
						rb3gpu_stats_t so;
						if (rb3gpu_stats(sl[b].h, &so) == 0) g_other_slices.ms_path += so.ms_h2d + so.ms_lf + so.ms_rank + so.ms_build, g_other_slices.n_sym += so.n_symbols_merged;
						rb3gpu_destroy(sl[b].h), sl[b].h = 0;
						if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] merged the index of slice %d into slice %d\n", __func__, rb3h_realtime(), rb3h_percent_cpu(), b, a);
					}
				}
			if (ret == 0 && nl > 0 && live[0] != 0) { /* slice 0 held nothing: the result lives in another slice's handle */
				rb3gpu_destroy(h);
				h = sl[live[0]].h, sl[live[0]].h = 0, sl[0].h = h;
			}
			has_index = ret == 0 && nl > 0;
			free(live);
		}
		if (ret == 0 && rb3h_verbose >= 3) fprintf(stderr, "[M::%s] tree merge of %d slices: %.3f s\n", __func__, N, rb3h_realtime() - t_tree);
		for (k = 1; k < N; ++k) if (sl[k].h) rb3gpu_destroy(sl[k].h);
		free(sl); free(th); free(rb);
	}
	free(fsize);
	if (g_iv.batches > 0 && rb3h_verbose >= 3)
		fprintf(stderr, "[M::%s::%.3f*%.2f] %ld batches merged into %d intervals: %ld lock-step rounds, %.3f s\n", __func__, rb3h_realtime(), rb3h_percent_cpu(), (long)g_iv.batches, g_iv.n, (long)g_iv.rounds, g_iv.t_walk);
	if (n_empty > 0 && rb3h_verbose >= 2)
		fprintf(stderr, "WARNING: skipped %ld empty sequence(s)\n", (long)n_empty);

	if (ret != 0 || !has_index) {
		if (g_iv.s) rb3gpu_shard_destroy(g_iv.s), g_iv.s = 0;
		while (n_old_sorters > 0) rb3gpu_sorter_destroy(old_sorters[--n_old_sorters]);
		pin_drain();
		rb3gpu_destroy(h);
		return 1;
	}

	if (g_iv.s) { /* --interval: the writers take the intervals in rank order, where they are (the reference writes its ropes one after the other,
	                 fm-index.c:31-54, and rld_enc joins the runs that meet: rld0.c:153-161) -- the index is never put together on one device */
		int64_t acc[7];
		rb3gpu_shard_get_acc(g_iv.s, acc);
		if (opt.fmt == FMT_FMR) {
			ret = dump_fmr(h, &opt, stdout);
		} else if (opt.fmt == FMT_FMD) {
			rb3h_fmdw_t *w = rb3h_fmdw_init();
			ret = w ? rb3gpu_shard_export_run_words(g_iv.s, sink_fmd_words, w) : -1;
			if (ret == 0) ret = rb3h_fmdw_finish(w);
			if (ret == 0) ret = rb3h_fmdw_dump(w, stdout);
			if (w) rb3h_fmdw_destroy(w);
		} else if (opt.fmt == FMT_BRE) { /* the intervals' runs in rank order into the host's packer */
			ret = write_bre_host(h, g_iv.s, stdout);
		} else {
			ret = rb3gpu_shard_export_runs(g_iv.s, sink_plain, stdout);
			fputc('\n', stdout);
		}
		if (rb3h_verbose >= 3) { /* what each device held */
			int64_t bnd[RB3GPU_SH_MAXIV + 1];
			const int n = rb3gpu_shard_bounds(g_iv.s, bnd);
			for (c = 0; c < n; ++c) {
				rb3gpu_stats_t st;
				if (rb3gpu_stats(rb3gpu_shard_handle(g_iv.s, c), &st) == 0)
					fprintf(stderr, "[M::%s] interval %d on device %d: %ld symbols, index %.1f MB, peak device memory %.1f MB; merge path: rank %.3f + rebuild %.3f ms\n", __func__, c, g_iv.devices[c], (long)(bnd[c + 1] - bnd[c]), st.bytes_index / 1e6, st.bytes_peak / 1e6, st.ms_rank, st.ms_build);
			}
		}
		/* the writers are done: the rank threads, the handles of intervals 1 .. N-1 and the replicated buffers go BEFORE the caller's handle (interval 0),
		   which the object points at */
		rb3gpu_shard_destroy(g_iv.s), g_iv.s = 0;
	} else if (opt.fmt == FMT_FMR) { /* build.c:245-260 */
		ret = dump_fmr(h, &opt, stdout);
	} else if (opt.fmt == FMT_FMD) {
		ret = write_fmd(h, stdout);
	} else if (opt.fmt == FMT_BRE) {
		ret = write_bre(h, stdout);
	} else {
		ret = rb3gpu_export_runs(h, sink_plain, stdout);
		fputc('\n', stdout);
	}
	fflush(stdout);
	if (rb3h_verbose >= 3) {
		rb3gpu_stats_t st;
		rb3gpu_stats(h, &st);
		fprintf(stderr, "[M::%s] GPU merge path: %ld symbols merged in %.3f ms (H2D %.3f + LF %.3f + rank %.3f + rebuild %.3f); index %.1f MB in HBM\n", __func__,
				(long)st.n_symbols_merged, st.ms_h2d + st.ms_lf + st.ms_rank + st.ms_build, st.ms_h2d, st.ms_lf, st.ms_rank, st.ms_build, st.bytes_index / 1e6);
		if (g_other_slices.n_sym > 0)
			fprintf(stderr, "[M::%s] the other slices of this multi-GPU build (their own GPUs, side by side): %ld symbols merged in %.3f ms of merge path, summed over the slices\n", __func__, (long)g_other_slices.n_sym, g_other_slices.ms_path);
		if (st.ms_sort > 0)
			fprintf(stderr, "[M::%s] GPU suffix sorting: %.3f ms in all (%ld doubling rounds), text upload included\n", __func__, st.ms_sort, (long)st.n_sort_rounds);
		if (g_sorted.ms_sort > 0)
			fprintf(stderr, "[M::%s] GPU sorter threads: text upload %.3f ms, suffix sorting %.3f ms (overlapped with the merges)\n", __func__, g_sorted.ms_upload, g_sorted.ms_sort);
		if (g_sorted.ms_order > 0)
			fprintf(stderr, "[M::%s] GPU sorter threads: strings put into %s order in %.3f ms\n", __func__, opt.so == RB3GPU_SO_RLO ? "RLO" : "RCLO", g_sorted.ms_order);
		fprintf(stderr, "[M::%s] rebuild: %.3f ms for %ld algorithmic bytes (9 B x rows + old + new block array per round) = %.1f GB/s; LF walkers: k_chain %.3f ms in %ld launches, %ld steps\n", __func__,
				st.ms_build, (long)st.bytes_rebuild, st.ms_build > 0 ? st.bytes_rebuild / st.ms_build / 1e6 : 0.0, st.ms_chain, (long)st.n_rank_launches, (long)st.n_lf_steps);
		fprintf(stderr, "[M::%s] run-space rebuild: %ld groups, %ld of them handed on to the window kernels; %ld merges redone without tentative records, %ld needed the long settle pass; %ld rows LF-checked; %.1f ms in %ld device allocations\n", __func__,
				(long)st.n_reb_groups, (long)st.n_reb_groups_window, (long)st.n_fallbacks, (long)st.n_long_settles, (long)st.n_lf_checked, st.ms_alloc, (long)st.n_allocs);
		if (st.tent_mask_bits > 256)
			fprintf(stderr, "[M::%s] tentative records: drop-out masks of %ld bits (walkers met intervals of more than %ld matching suffixes)\n", __func__, (long)st.tent_mask_bits, (long)st.tent_mask_bits / 2 - 1);
		fprintf(stderr, "[M::%s] device memory of the index handle: peak %.1f MB, index %.1f MB\n", __func__, st.bytes_peak / 1e6, st.bytes_index / 1e6);
		fprintf(stderr, "[M::%s] batches: %ld (%ld symbols) suffix-sorted on the GPU, %ld (%ld symbols) on the host; -m %ld%s\n", __func__,
				(long)g_sorted.n_gpu, (long)g_sorted.sym_gpu, (long)g_sorted.n_host, (long)g_sorted.sym_host, (long)opt.batch_size,
				batch_cut(&opt) != opt.batch_size ? " cut into GPU sub-batches (--gpu-batch)" : "");
	}
	while (n_old_sorters > 0) rb3gpu_sorter_destroy(old_sorters[--n_old_sorters]);
	pin_drain();
	rb3gpu_destroy(h);
	if (ret != 0) { fprintf(stderr, "ERROR: failed to write the index (code %d)\n", ret); return 1; }
	return 0;
}

/* merge, main.c:84-133 (rb3_fmi_merge, fm-index.c:251-277): merge whole indexes into the first one.
 * The plain BWT of an index is itself a valid partial BWT whose sentinels all sort after those of
 * the base (fm-index.c:147), so every further index is decoded to plain symbols on the host and goes
 * through the same rb3gpu_merge_plain path as a batch. */
typedef struct { uint8_t *s; int64_t l, m; } plainvec_t;

static int sink_plainvec(void *data, int c, int64_t l)
{
	plainvec_t *v = (plainvec_t*)data;
	if (v->l + l > v->m) {
		v->m = (v->l + l) + ((v->l + l) >> 1) + 1024;
		v->s = (uint8_t*)realloc(v->s, (size_t)v->m);
		if (v->s == 0) return -1;
	}
	memset(v->s + v->l, c, (size_t)l);
	v->l += l;
	return 0;
}

/* One further index into the handle's.  The file is opened ONCE (it may be a pipe, or stdin) and goes by its magic: the words of an FMD file and the
 * records of a BRE file are decoded on the device and merged as one batch; an FMR file, anything with --host-fmd, an FMD on stdin and what the device
 * declined are decoded to plain symbols on the host.  0, 1 (not a loadable index file) or the engine's negative code */
static int merge_operand(rb3gpu_t *h, const char *fn)
{
	plainvec_t pv = {0, 0, 0};
	char magic[4];
	FILE *fp = rb3h_index_open(fn, magic);
	const int kind = fp ? rb3h_index_kind(magic) : RB3H_INDEX_NONE;
	int ret = 1, on_host = 0;
	if (fp == 0) return 1;
	if (!g_host_fmd && kind == RB3H_INDEX_FMD && fp != stdin) {
		uint64_t *z = 0;
		int64_t nw = 0, mc[6];
		if (rb3h_fmd_read_words_fp(fp, &z, &nw, mc) == 0) {
			ret = rb3gpu_merge_fmd_words(h, nw, z, mc);
			free(z);
			if (ret == RB3GPU_ESYMBOL || ret == RB3GPU_ENOMEM) { /* the device declined the stream: the host decoder reads the file again */
				fclose(fp), fp = 0;
				on_host = rb3h_index_read_runs(fn, sink_plainvec, &pv) == 0 && pv.l > 0;
				ret = 1;
			}
		}
	} else if (!g_host_fmd && kind == RB3H_INDEX_BRE) {
		rb3h_bre_t b;
		if (rb3h_bre_read_fp(fp, &b) == 0) {
			rb3gpu_bre_stats_t st;
			rb3gpu_tune(h, "verbose", 0); /* (the file may still be refused: see index_upload) */
			ret = rb3gpu_merge_bre(h, b.b_per_run, b.n_rec, b.rec, &st);
			rb3gpu_tune(h, "verbose", rb3h_verbose);
			if (ret == 0 && (st.n_sym != b.ftr[1] || st.n_run != b.ftr[2])) ret = 1; /* the footer disagrees with what the device counted */
			else if (ret == RB3GPU_ESYMBOL) ret = 1;
			else if (ret == RB3GPU_ENOMEM) { /* no room on the device: the host decoder takes the records */
				on_host = rb3h_bre_decode_runs(&b, sink_plainvec, &pv) == 0 && pv.l > 0;
				ret = 1;
			}
			rb3h_bre_free(&b);
		}
	} else on_host = rb3h_index_read_runs_fp(fp, magic, sink_plainvec, &pv) == 0 && pv.l > 0;
	if (fp && fp != stdin) fclose(fp);
	if (on_host) ret = rb3gpu_merge_plain(h, pv.l, pv.s);
	free(pv.s);
	return ret;
}

int main_merge(int argc, char *argv[])
{
	int c, i, ret = 0, fmt = FMT_FMR, device = 0;
	char *fn_tmp = 0;
	rb3gpu_t *h;
	rb3gpu_opt_t gopt;
	bopt_t opt;
	bopt_init(&opt);
	optind = 1;
	while ((c = getopt_long(argc, argv, "t:o:S:db", long_opts, 0)) >= 0) {
		if (c == 't') opt.n_threads = atoi(optarg);
		else if (c == 'o') { if (freopen(optarg, "wb", stdout) == 0) return 1; }
		else if (c == 'S') fn_tmp = optarg;
		else if (c == 'd') fmt = FMT_FMD;
		else if (c == 'b') fmt = FMT_FMR;
		else if (c == 301) device = atoi(optarg);
		else if (c == 308) g_host_fmd = 1;
		else if (c == '?') return 1;
	}
	if (argc - optind < 2) {
		fprintf(stdout, "Usage: ropebwt3-amd merge [options] <base.fmr|fmd> <other1.fmr|fmd> [...]\n");
		fprintf(stdout, "Options:\n");
		fprintf(stdout, "  -o FILE    output to FILE [stdout]\n");
		fprintf(stdout, "  -b / -d    output FMR (default, as the reference) / FMD\n");
		fprintf(stdout, "  -S FILE    save the current index to FILE after each input file []\n");
		fprintf(stdout, "  --gpu INT  HIP device ordinal [0]\n");
		return 1;
	}
	rb3gpu_opt_init(&gopt);
	gopt.device = device, gopt.verbose = rb3h_verbose;
	h = rb3gpu_create(&gopt);
	if (h == 0) { fprintf(stderr, "ERROR: no usable MI355X/HIP device; the merge path has no CPU fallback\n"); return 1; }
	if (load_index(h, argv[optind]) < 0) {
		fprintf(stderr, "ERROR: failed to load FMR/FMD file '%s'\n", argv[optind]);
		rb3gpu_destroy(h);
		return 1;
	}
	for (i = optind + 1; i < argc && ret == 0; ++i) {
		ret = merge_operand(h, argv[i]);
		if (ret > 0) { fprintf(stderr, "ERROR: failed to load FMR/FMD file '%s'\n", argv[i]); break; }
		if (ret < 0) { fprintf(stderr, "ERROR: the GPU engine failed to merge '%s': %s\n", argv[i], rb3gpu_strerror(ret)); break; }
		if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] merged '%s'\n", __func__, rb3h_realtime(), rb3h_percent_cpu(), argv[i]);
		if (fn_tmp) {
			FILE *fp = fopen(fn_tmp, "wb");
			if (fp) { dump_fmr(h, &opt, fp); fclose(fp); }
		}
	}
	if (ret == 0) {
		if (fmt == FMT_FMR) ret = dump_fmr(h, &opt, stdout);
		else {
			ret = write_fmd(h, stdout);
		}
		fflush(stdout);
	}
	rb3gpu_destroy(h);
	return ret == 0 ? 0 : 1;
}

/* `ssa`, ssa.c:246-279: sampled suffix array of an index, written as rb3_ssa_dump does (ssa.c:198-213) */
int main_ssa(int argc, char *argv[])
{
	int c, ret, ssa_shift = 8, device = 0, ms = 0;
	int64_t m = 0, n_ssa = 0;
	uint64_t *r2i = 0, *ssa = 0;
	char *fn = 0;
	FILE *fp;
	rb3gpu_t *h;
	rb3gpu_opt_t gopt;
	optind = 1;
	while ((c = getopt_long(argc, argv, "t:s:o:", long_opts, 0)) >= 0) {
		if (c == 't') {} /* threads of the reference's kt_for: nothing to size here */
		else if (c == 's') ssa_shift = atoi(optarg);
		else if (c == 'o') fn = optarg;
		else if (c == 301) device = atoi(optarg);
		else if (c == 308) g_host_fmd = 1;
		else if (c == '?') return 1;
	}
	if (argc == optind) {
		fprintf(stderr, "Usage: ropebwt3-amd ssa [options] <in.fmd|fmr>\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  -s INT     sample rate one SA per 2**INT bases [%d]\n", ssa_shift);
		fprintf(stderr, "  -o FILE    output to file [stdout]\n");
		fprintf(stderr, "  --gpu INT  HIP device ordinal [0]\n");
		return 1;
	}
	rb3gpu_opt_init(&gopt);
	gopt.device = device, gopt.verbose = rb3h_verbose;
	h = rb3gpu_create(&gopt);
	if (h == 0) { fprintf(stderr, "ERROR: no usable MI355X/HIP device; there is no CPU fallback\n"); return 1; }
	if (load_index(h, argv[optind]) < 0) {
		fprintf(stderr, "[E::%s] failed to load the FM-index\n", __func__);
		rb3gpu_destroy(h);
		return 1;
	}
	if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] loaded the index\n", __func__, rb3h_realtime(), rb3h_percent_cpu());
	ret = rb3gpu_ssa_dims(h, ssa_shift, &m, &n_ssa, &ms);
	if (ret == 0) {
		r2i = (uint64_t*)calloc((size_t)(m > 0 ? m : 1), 8);
		ssa = (uint64_t*)calloc((size_t)(n_ssa > 0 ? n_ssa : 1), 8);
		ret = r2i && ssa ? rb3gpu_ssa_gen(h, ssa_shift, r2i, ssa) : -1;
	}
	if (ret < 0) fprintf(stderr, "ERROR: the GPU engine failed to generate the sampled suffix array: %s\n", rb3gpu_strerror(ret));
	else {
		if (rb3h_verbose >= 3) {
			rb3gpu_stats_t st;
			rb3gpu_stats(h, &st);
			fprintf(stderr, "[M::%s::%.3f*%.2f] %lld samples of %lld strings in %.3f ms on the GPU (LF walk %.3f ms)\n", __func__, rb3h_realtime(), rb3h_percent_cpu(),
					(long long)n_ssa, (long long)m, st.ms_ssa, st.ms_ssa_walk);
		}
		fp = fn && strcmp(fn, "-") ? fopen(fn, "wb") : stdout;
		if (fp == 0) ret = -1;
		else {
			uint32_t y;
			fwrite("SSA\1", 1, 4, fp);
			y = (uint32_t)ssa_shift; fwrite(&y, 4, 1, fp);
			y = (uint32_t)ms; fwrite(&y, 4, 1, fp);
			fwrite(&m, 8, 1, fp);
			fwrite(&n_ssa, 8, 1, fp);
			fwrite(r2i, 8, (size_t)m, fp);
			fwrite(ssa, 8, (size_t)n_ssa, fp);
			if (fp != stdout) fclose(fp); else fflush(fp);
		}
	}
	free(r2i); free(ssa);
	rb3gpu_destroy(h);
	return ret == 0 ? 0 : 1;
}

/* kount: the k-mers that occur at least -m times in some index, with their count in every index (the reference's main_kount,
 * main.c:333-423), counted on the GPU (rb3gpu_kount).  The lines are formatted here, into a buffer written in large pieces.
 * One difference: -k below 1 is refused (the reference crashes on -k 0). */
typedef struct { FILE *fp; char *buf; size_t l, m; int err; double t_fmt; } kount_out_t;

static void kount_flush(kount_out_t *o)
{
	if (o->l > 0 && fwrite(o->buf, 1, o->l, o->fp) != o->l) o->err = 1;
	o->l = 0;
}

static int kount_sink(void *ud, int64_t n, int n_idx, int k, const uint8_t *kmers, const int64_t *counts)
{
	kount_out_t *o = (kount_out_t*)ud;
	const double t0 = rb3h_realtime();
	const size_t line_max = (size_t)k + (size_t)n_idx * 21 + 1;
	int64_t r;
	int i, p;
	for (r = 0; r < n; ++r) {
		const uint8_t *s = kmers + r * k;
		char *b;
		if (o->l + line_max > o->m) kount_flush(o);
		b = o->buf + o->l;
		for (p = 0; p < k; ++p) b[p] = "$ACGTN"[s[p] < 6 ? s[p] : 5];
		b += k;
		for (i = 0; i < n_idx; ++i) { /* "\t%ld" */
			int64_t x = counts[r * n_idx + i];
			char t[24];
			int nt = 0, neg = x < 0;
			uint64_t u = neg ? (uint64_t)0 - (uint64_t)x : (uint64_t)x;
			do t[nt++] = (char)('0' + u % 10), u /= 10; while (u);
			*b++ = '\t';
			if (neg) *b++ = '-';
			while (nt > 0) *b++ = t[--nt];
		}
		*b++ = '\n';
		o->l = (size_t)(b - o->buf);
	}
	o->t_fmt += rb3h_realtime() - t0;
	return o->err ? -1 : 0;
}

static int main_kount(int argc, char *argv[])
{
	int c, k = 51, min_occ = 100, device = 0, n, i, ret;
	rb3gpu_t **hs;
	rb3gpu_kount_stats_t st;
	kount_out_t o;
	optind = 1;
	while ((c = getopt_long(argc, argv, "k:m:", long_opts, 0)) >= 0) {
		if (c == 'k') k = (int)atol(optarg); /* (an int, as in the reference) */
		else if (c == 'm') min_occ = (int)atol(optarg);
		else if (c == 301) device = atoi(optarg);
		else if (c == 308) g_host_fmd = 1;
		else if (c == '?') return 1;
	}
	if (argc == optind) {
		fprintf(stderr, "Usage: ropebwt3-amd kount [options] <in1.fmd> [in2.fmd [...]]\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  -k INT     k-mer length [%d]\n", k);
		fprintf(stderr, "  -m INT     min k-mer occurrence [%d]\n", min_occ);
		fprintf(stderr, "  --gpu INT  HIP device ordinal [0]\n");
		return 1;
	}
	if (k < 1) {
		fprintf(stderr, "ERROR: the k-mer length (-k) must be at least 1\n");
		return 1;
	}
	n = argc - optind;
	hs = (rb3gpu_t**)calloc((size_t)n, sizeof(*hs));
	if (hs == 0) return 1;
	for (i = 0, ret = 0; i < n && ret == 0; ++i)
		if ((hs[i] = open_index(device, argv[optind + i], 0)) == 0) ret = 1;
	if (ret == 0) {
		if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] loaded %d index(es)\n", __func__, rb3h_realtime(), rb3h_percent_cpu(), n);
		o.fp = stdout, o.l = 0, o.err = 0, o.t_fmt = 0;
		o.m = (size_t)k + (size_t)n * 21 + 1;
		o.m = o.m < ((size_t)1 << 20) ? (size_t)1 << 20 : o.m * 2;
		o.buf = (char*)malloc(o.m);
		if (o.buf == 0) ret = 1;
		else {
			const int r = rb3gpu_kount(hs, n, k, min_occ, 0, kount_sink, &o, &st);
			kount_flush(&o);
			if (fflush(stdout) != 0) o.err = 1;
			if (r != 0 && !o.err) fprintf(stderr, "ERROR: the GPU engine failed to count the k-mers: %s\n", rb3gpu_strerror(r));
			else if (o.err) fprintf(stderr, "ERROR: failed to write the output\n");
			else if (rb3h_verbose >= 3)
				fprintf(stderr, "[M::%s::%.3f*%.2f] %lld k-mers; %lld nodes expanded in %lld slice(s): %.3f ms in the engine, of which %.3f ms formatting lines; expansion kernel %.3f ms\n",
						__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)st.n_out, (long long)st.n_nodes, (long long)st.n_slices, st.ms_total, o.t_fmt * 1e3, st.ms_expand);
			ret = r != 0 || o.err ? 1 : 0;
			free(o.buf);
		}
	}
	for (i = 0; i < n; ++i) if (hs[i]) rb3gpu_destroy(hs[i]);
	free(hs);
	return ret;
}

/* mem: the super-maximal exact matches of every query in the index (the reference's main_search for `mem`, search.c:443-582, with its
 * default algorithm), found on the GPU (rb3gpu_mem).  Queries are taken in batches of -K symbols; the lines of a batch are formatted
 * into one buffer (rb3h_mem_format) that is written in large pieces.  -p INT adds up to INT positions per match, located on the GPU
 * through <index>.ssa, named through <index>.len.gz (rb3gpu_mem_pos, rb3h_mem_format_pos).  Differences, each a refusal with exit status 1:
 * --old-mem, -l or -c below 1, the options of `sw` and `hapdiv`; and every refusal exits 1 (the reference exits 0 on some). */
typedef struct {
	rb3h_buf_t out;
	int mode, err;
	int64_t min_gap, id0, n_query, next_q, pend_q, n_pend, m_pend;
	rb3h_mem_rec_t *pend;       /* the matches of query pend_q so far (a query's matches may come in several pieces) */
	const int64_t *off;         /* the batch: offsets of the queries' symbols, of their names in `names` (-1: none) */
	const int64_t *name_off;
	const char *names;
	const rb3h_sid_t *sid;      /* not NULL: lines with positions; the positions of pend[i] are pend_pos[pend_off[i], pend_off[i + 1]) */
	int64_t *pend_off, m_pos;
	rb3h_pos_t *pend_pos;
} mem_out_t;

/* the lines of the queries [next_q, q) (the matches collected for pend_q among them) */
static void mem_advance(mem_out_t *o, int64_t q)
{
	for (; o->next_q < q; ++o->next_q) {
		const int64_t i = o->next_q, n = o->n_pend > 0 && o->pend_q == i ? o->n_pend : 0;
		if (n == 0 && o->mode != RB3H_MEM_GAP) continue; /* (only --gap has something to say about a query without matches) */
		if (o->sid) {
			if (rb3h_mem_format_pos(&o->out, o->name_off[i] >= 0 ? o->names + o->name_off[i] : 0, o->id0 + i, n, o->pend, o->pend_off, o->pend_pos, o->sid) < 0) o->err = 1;
		} else if (rb3h_mem_format(&o->out, o->mode, o->min_gap, o->name_off[i] >= 0 ? o->names + o->name_off[i] : 0, o->id0 + i, o->off[i + 1] - o->off[i], n, o->pend) < 0) o->err = 1;
		if (n > 0) o->n_pend = 0;
		if (out_flush(&o->out, 0) < 0) o->err = 1;
	}
}

static int mem_sink_pos(void *ud, int64_t n, const rb3gpu_mem_rec_t *recs, const int64_t *off, const rb3gpu_pos_t *pos)
{
	mem_out_t *o = (mem_out_t*)ud;
	int64_t i = 0;
	while (i < n && !o->err) {
		const int64_t q = recs[i].query;
		int64_t k = i + 1;
		while (k < n && recs[k].query == q) ++k;
		if (q < o->next_q || q >= o->n_query) { o->err = 2; break; }
		if (o->n_pend == 0 || o->pend_q != q) mem_advance(o, q), o->pend_q = q, o->n_pend = 0;
		if (o->n_pend + (k - i) > o->m_pend) {
			const int64_t m = (o->n_pend + (k - i)) * 2 + 256;
			rb3h_mem_rec_t *t = (rb3h_mem_rec_t*)realloc(o->pend, (size_t)m * sizeof(*t));
			int64_t *u;
			if (t == 0) { o->err = 1; break; }
			o->pend = t;
			u = (int64_t*)realloc(o->pend_off, (size_t)(m + 1) * 8);
			if (u == 0) { o->err = 1; break; }
			o->pend_off = u, o->m_pend = m;
		}
		memcpy(o->pend + o->n_pend, recs + i, (size_t)(k - i) * sizeof(*recs));
		if (o->n_pend == 0) o->pend_off[0] = 0;
		if (off) { /* the positions of these records behind those the query has already */
			const int64_t base = o->pend_off[o->n_pend], np = off[k] - off[i];
			int64_t x;
			if (base + np > o->m_pos) {
				const int64_t m = (base + np) * 2 + 1024;
				rb3h_pos_t *t = (rb3h_pos_t*)realloc(o->pend_pos, (size_t)m * sizeof(*t));
				if (t == 0) { o->err = 1; break; }
				o->pend_pos = t, o->m_pos = m;
			}
			if (np > 0) memcpy(o->pend_pos + base, pos + off[i], (size_t)np * sizeof(*pos));
			for (x = i; x < k; ++x) o->pend_off[o->n_pend + (x - i) + 1] = base + (off[x + 1] - off[i]);
		} else {
			int64_t x;
			for (x = 0; x < k - i; ++x) o->pend_off[o->n_pend + x + 1] = o->pend_off[o->n_pend];
		}
		o->n_pend += k - i, i = k;
	}
	return o->err ? -1 : 0;
}

static int mem_sink(void *ud, int64_t n, const rb3gpu_mem_rec_t *recs) { return mem_sink_pos(ud, n, recs, 0, 0); }

static const struct option mem_long_opts[] = {
	{ "gap", required_argument, 0, 403 },
	{ "cov", no_argument, 0, 404 },
	{ "old-mem", no_argument, 0, 405 },
	{ "no-ssa", no_argument, 0, 406 },
	{ "seq", no_argument, 0, 406 },
	{ "all-e2e", no_argument, 0, 406 },
	{ "gpu", required_argument, 0, 301 },
	{ "host-fmd", no_argument, 0, 308 },
	{ "chunk", required_argument, 0, 407 },
	{ 0, 0, 0, 0 }
};

static int main_mem(int argc, char *argv[])
{
	int c, is_line = 0, device = 0, mode = RB3H_MEM_LINES, ret = 0, j, max_pos = 0;
	rb3h_ssa_t *sa = 0;
	rb3h_sid_t *sid = 0;
	index_host_t ih;
	rb3gpu_locate_stats_t lsum;
	int64_t min_len = 19, min_occ = 1, batch_size = 100000000, min_gap = 0, chunk = 0, id = 0;
	int64_t n_steps = 0, n_walkers = 0, n_records = 0, n_slices = 0, n_batches = 0;
	double ms_walk = 0, ms_engine = 0;
	rb3gpu_t *h;
	int64_t acc[7];
	mem_out_t o;
	rb3h_qbatch_t b;
	_Static_assert(sizeof(rb3h_mem_rec_t) == sizeof(rb3gpu_mem_rec_t), "one record layout on both sides");
	_Static_assert(sizeof(rb3h_pos_t) == sizeof(rb3gpu_pos_t), "one position layout on both sides");
	optind = 1;
	while ((c = getopt_long(argc, argv, "Ll:c:t:K:MdN:A:B:O:E:C:m:k:uj:ey:a:w:p:bg:", mem_long_opts, 0)) >= 0) {
		if (c == 'L') is_line = 1;
		else if (c == 'l') min_len = atol(optarg);
		else if (c == 'c') min_occ = atol(optarg);
		else if (c == 't' || c == 'M') {} /* threads of the reference's kt_for, its mmap loader: nothing to size here */
		else if (c == 'K') batch_size = rb3h_parse_num(optarg);
		else if (c == 403) min_gap = (int32_t)rb3h_parse_num(optarg);
		else if (c == 404) mode = RB3H_MEM_COV;
		else if (c == 301) device = atoi(optarg);
		else if (c == 308) g_host_fmd = 1;
		else if (c == 407) chunk = rb3h_parse_num(optarg);
		else if (c == 'p') max_pos = atoi(optarg);
		else if (c == 405) { fprintf(stderr, "ERROR: --old-mem is not supported: mem runs the default algorithm only\n"); return 1; }
		else if (c == '?') return 1;
		else { fprintf(stderr, "ERROR: option not supported by mem (it belongs to sw or hapdiv)\n"); return 1; }
	}
	if (argc - optind < 2) {
		fprintf(stdout, "Usage: ropebwt3-amd mem [options] <idx.fmr> <seq.fa> [...]\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  -l INT      min MEM length [%ld]\n", (long)min_len);
		fprintf(stderr, "  -c INT      min interval size [%ld]\n", (long)min_occ);
		fprintf(stderr, "  --gap=NUM   output regions >=NUM that are not covered by MEMs [%d]\n", (int)min_gap);
		fprintf(stderr, "  --cov       output breadth of coverage\n");
		fprintf(stderr, "  -t INT      number of threads [4]\n");
		fprintf(stderr, "  -L          one sequence per line in the input\n");
		fprintf(stderr, "  -K NUM      query batch size [100m]\n");
		fprintf(stderr, "  -M          use mmap to load FMD\n");
		return 0;
	}
	if (min_len < 1) { fprintf(stderr, "ERROR: the min MEM length (-l) must be at least 1\n"); return 1; }
	if (min_occ < 1) { fprintf(stderr, "ERROR: the min interval size (-c) must be at least 1\n"); return 1; }
	if (min_gap > 0) mode = RB3H_MEM_GAP, max_pos = 0; /* (before --cov, search.c:271-279; no positions beside gaps, search.c:494) */
	memset(&lsum, 0, sizeof(lsum));
	memset(&ih, 0, sizeof(ih));
	if (max_pos > 0) { /* the two files beside the index (rb3_fmi_load_all, fm-index.c:606-640), read and held against the index before anything is asked of a
	                    * device: files of another index are no files (fm-index.c:615, 633), and the refusal is the only line (search.c:555-559: before the check for both strands) */
		int64_t m, n_sym;
		int ms;
		side_read(argv[optind], &sa, &sid);
		if (sa == 0 || sid == 0) goto no_side;
		if (index_host_read(argv[optind], &ih) < 0) {
			if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: failed to load index '%s'\n", argv[optind]);
			rb3h_ssa_destroy(sa); rb3h_sid_destroy(sid);
			return 1;
		}
		m = index_host_sentinels(&ih, &n_sym);
		for (ms = 1; (1LL << ms) < m; ++ms) {} /* ssa.c:63-64: what a sampled suffix array of THIS index looks like */
		if (sa->m != m || sid->n_seq * 2 != m || sa->ms != ms || sa->ss > 40 || sa->n_ssa != (n_sym - m + (1LL << sa->ss) - 1) >> sa->ss) goto no_side;
	}
	h = open_index(device, argv[optind], max_pos > 0 ? &ih : 0);
	if (h == 0) { rb3h_ssa_destroy(sa); rb3h_sid_destroy(sid); index_host_free(&ih); return 1; }
	rb3gpu_get_acc(h, acc);
	if (max_pos > 0) { /* (the sample rate and the width of the string field must be those of this index as well) */
		if (sa->m != acc[1] || sid->n_seq * 2 != acc[1] || rb3gpu_ssa_set(h, sa->ss, sa->ms, sa->m, sa->n_ssa, sa->r2i, sa->ssa) != 0) {
			rb3gpu_destroy(h);
			goto no_side;
		}
		rb3h_ssa_destroy(sa), sa = 0; /* (it lives on the device from here on) */
	}
	if (!both_strands(acc)) {
		rb3gpu_destroy(h);
		rb3h_sid_destroy(sid);
		return 1;
	}
	if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] loaded the index\n", __func__, rb3h_realtime(), rb3h_percent_cpu());
	memset(&o, 0, sizeof(o));
	memset(&b, 0, sizeof(b));
	o.mode = mode, o.min_gap = min_gap;
	if (max_pos > 0 && mode == RB3H_MEM_LINES) o.sid = sid; /* (--cov -p needs the files and prints no positions, search.c:279) */
	for (j = optind + 1; j < argc && ret == 0; ++j) {
		rb3h_seqio_t *fp = rb3h_seq_open(argv[j], is_line);
		if (fp == 0) {
			if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: failed to load the sequence file '%s'\n", argv[j]);
			ret = 1;
			break;
		}
		for (b.eof = 0; !b.eof && ret == 0;) { /* a batch: records until their symbols reach -K (search.c:366-378) */
			const int64_t n_q = rb3h_qbatch_read(fp, &b, batch_size, 0x7fffffffLL, 0x7fffffffLL);
			if (n_q == -1) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; }
			if (n_q == -2) { fprintf(stderr, "ERROR: a query of more than 2^31 - 1 symbols\n"); ret = 1; }
			if (rb3h_seq_error(fp) && rb3h_verbose >= 1 && b.eof) fprintf(stderr, "ERROR: FASTX parsing error (code %d)\n", rb3h_seq_error(fp));
			if (n_q > 0) {
				rb3gpu_mem_stats_t st;
				int r;
				o.off = b.off, o.name_off = b.name_off, o.names = (const char*)b.names.s, o.id0 = id, o.n_query = n_q, o.next_q = 0, o.n_pend = 0;
				if (o.sid) {
					rb3gpu_locate_stats_t ls;
					r = rb3gpu_mem_pos(h, n_q, b.off, b.sym.s, min_len, min_occ, chunk, max_pos, mem_sink_pos, &o, &st, &ls);
					lsum.ms_locate += ls.ms_locate, lsum.n_pops += ls.n_pops, lsum.n_intervals += ls.n_intervals, lsum.n_tier2 += ls.n_tier2, lsum.n_pairs += ls.n_pairs;
					lsum.max_heap = lsum.max_heap > ls.max_heap ? lsum.max_heap : ls.max_heap;
				} else r = rb3gpu_mem(h, n_q, b.off, b.sym.s, min_len, min_occ, chunk, mem_sink, &o, &st);
				if (r == 0 && !o.err) mem_advance(&o, n_q);
				if (out_flush(&o.out, 1) < 0) o.err = 1;
				if (r != 0 && !o.err) { fprintf(stderr, "ERROR: the GPU engine failed to find the matches: %s\n", rb3gpu_strerror(r)); ret = 1; }
				else if (o.err) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
				id += n_q, ++n_batches;
				n_steps += st.n_steps, n_walkers += st.n_walkers, n_records += st.n_records, n_slices += st.n_slices, ms_walk += st.ms_walk, ms_engine += st.ms_total;
				if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] processed %lld sequences\n", __func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)n_q);
			}
		}
		rb3h_seq_close(fp);
	}
	if (fflush(stdout) != 0 && ret == 0) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
	if (rb3h_verbose >= 3 && ret == 0)
		fprintf(stderr, "[M::%s::%.3f*%.2f] %lld queries in %lld batch(es): %lld matches from %lld walkers in %lld slice(s), %lld extensions; %.3f ms in the engine, walkers' kernel %.3f ms\n",
				__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)id, (long long)n_batches, (long long)n_records, (long long)n_walkers, (long long)n_slices, (long long)n_steps, ms_engine, ms_walk);
	if (rb3h_verbose >= 3 && ret == 0 && o.sid)
		fprintf(stderr, "[M::%s::%.3f*%.2f] %lld positions of %lld matches: %lld heap pops, %lld matches with a heap in global memory, largest heap %lld; locate kernels %.3f ms\n",
				__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)lsum.n_pairs, (long long)lsum.n_intervals, (long long)lsum.n_pops, (long long)lsum.n_tier2, (long long)lsum.max_heap, lsum.ms_locate);
	free(o.out.s); free(o.pend); free(o.pend_off); free(o.pend_pos);
	rb3h_qbatch_free(&b);
	rb3gpu_destroy(h);
	rb3h_sid_destroy(sid);
	return ret;
no_side:
	index_host_free(&ih);
	if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: failed to load suffix array samples or sequence names/lengths\n");
	rb3h_ssa_destroy(sa); rb3h_sid_destroy(sid);
	return 1;
}

/* suffix <idx> <seq.fa> [...] (main_suffix, main.c:167-217 of the reference): per query the longest suffix that occurs in the index -- where it starts,
 * the query's length, its occurrences --, found on the GPU (rb3gpu_suffix).  The queries come through the reader of `mem`, in batches of a fixed number
 * of symbols, and a line has the shape of a line of `mem`, so it goes through its formatter.  Any index serves, one strand or both.  Options the command
 * does not know are passed over, as the reference's option loop does.  Difference: a query file that cannot be opened is one line and exit status 1 behind
 * the answers of the files before it (the reference reads through a null pointer there). */
#define SUFFIX_BATCH 100000000 /* query symbols per call of the engine */

static const struct option walk_long_opts[] = {
	{ "gpu", required_argument, 0, 301 },
	{ "host-fmd", no_argument, 0, 308 },
	{ 0, 0, 0, 0 }
};

static int main_suffix(int argc, char *argv[])
{
	int c, is_line = 0, device = 0, ret = 0, j;
	int64_t id = 0, n_steps = 0, n_slices = 0, n_batches = 0, n_sym = 0;
	double ms_walk = 0, ms_engine = 0;
	rb3gpu_t *h;
	rb3h_buf_t out = {0, 0, 0};
	rb3h_qbatch_t b;
	int64_t m_rec = 0;
	rb3gpu_suffix_rec_t *rec = 0;
	optind = 1, opterr = 0;
	memset(&b, 0, sizeof(b));
	while ((c = getopt_long(argc, argv, "L", walk_long_opts, 0)) >= 0) {
		if (c == 'L') is_line = 1;
		else if (c == 301) device = atoi(optarg);
		else if (c == 308) g_host_fmd = 1;
	}
	if (argc - optind < 2) {
		fprintf(stdout, "Usage: ropebwt3-amd suffix [options] <idx.fmr> <seq.fa> [...]\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  -L        one sequence per line in the input\n");
		return 0;
	}
	if ((h = open_index(device, argv[optind], 0)) == 0) return 1;
	if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] loaded the index\n", __func__, rb3h_realtime(), rb3h_percent_cpu());
	for (j = optind + 1; j < argc && ret == 0; ++j) {
		rb3h_seqio_t *fp = rb3h_seq_open(argv[j], is_line);
		if (fp == 0) {
			if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: failed to load the sequence file '%s'\n", argv[j]);
			ret = 1;
			break;
		}
		for (b.eof = 0; !b.eof && ret == 0;) { /* a batch: records until their symbols reach SUFFIX_BATCH, as nt6 codes (main.c:200-202: anything from 128 on is 5) */
			const int64_t n_q = rb3h_qbatch_read(fp, &b, SUFFIX_BATCH, INT64_MAX, 0x7fffffffLL), *off = b.off, *name_off = b.name_off;
			int64_t i;
			if (n_q == -1) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; }
			if (n_q == -2) { fprintf(stderr, "ERROR: a query of more than 2^31 - 1 symbols\n"); ret = 1; }
			if (rb3h_seq_error(fp) && rb3h_verbose >= 1 && b.eof) fprintf(stderr, "ERROR: FASTX parsing error (code %d)\n", rb3h_seq_error(fp));
			if (n_q > 0) {
				rb3gpu_suffix_stats_t st;
				int r, werr = 0;
				if (n_q > m_rec) {
					m_rec = n_q + (n_q >> 1) + 256;
					rec = (rb3gpu_suffix_rec_t*)realloc(rec, (size_t)m_rec * sizeof(*rec));
					if (rec == 0) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; break; }
				}
				r = rb3gpu_suffix(h, n_q, off, b.sym.s, rec, &st);
				if (r != 0) { fprintf(stderr, "ERROR: the GPU engine failed to find the suffixes: %s\n", rb3gpu_strerror(r)); ret = 1; break; }
				for (i = 0; i < n_q && !werr; ++i) { /* name, start, length, occurrences: a line of `mem` (main.c:207-209; seq<N> counts every record) */
					rb3h_mem_rec_t t;
					t.query = i, t.x0 = 0, t.size = rec[i].size, t.st = (int32_t)rec[i].start, t.en = (int32_t)(off[i + 1] - off[i]);
					if (rb3h_mem_format(&out, RB3H_MEM_LINES, 0, name_off[i] >= 0 ? (const char*)b.names.s + name_off[i] : 0, id + i, off[i + 1] - off[i], 1, &t) < 0) werr = 1;
					if (out_flush(&out, i + 1 == n_q) < 0) werr = 1;
				}
				if (werr) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
				id += n_q, ++n_batches, n_sym += b.sym.l;
				n_steps += st.n_steps, n_slices += st.n_slices, ms_walk += st.ms_walk, ms_engine += st.ms_total;
				if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] processed %lld sequences\n", __func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)n_q);
			}
		}
		rb3h_seq_close(fp);
	}
	if (fflush(stdout) != 0 && ret == 0) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
	if (rb3h_verbose >= 3 && ret == 0)
		fprintf(stderr, "[M::%s::%.3f*%.2f] %lld queries of %lld symbols in %lld batch(es) and %lld slice(s): %lld extensions; %.3f ms in the engine, walk kernel %.3f ms\n",
				__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)id, (long long)n_sym, (long long)n_batches, (long long)n_slices, (long long)n_steps, ms_engine, ms_walk);
	free(out.s); free(rec);
	rb3h_qbatch_free(&b);
	rb3gpu_destroy(h);
	return ret;
}

/* get <idx> <int> [...] (main_get, main.c:135-165 of the reference): for every argument, read with atol, the string in front of the suffix of that row --
 * for a sentinel's row the whole indexed string -- as `>row end_row` and a line of $ACGTN letters; rows outside the index print nothing.  All rows of the
 * command line go through ONE call of rb3gpu_retrieve.  Arguments that begin with `-` are options nobody knows and are passed over, wherever they stand.
 * Two options of this command alone: --pieces sends the same rows through rb3gpu_retrieve_pieces (the whole index walked once in pieces: for long strings),
 * --all takes no rows and prints every string of the index, rows 0 .. acc[1] - 1, through the same call. */
typedef struct { const int64_t *rows; rb3h_buf_t out; int err; } get_out_t; /* rows == 0: row i is i (--all) */

static int get_sink(void *ud, int64_t i0, int64_t n, const int64_t *end_row, const int64_t *off, const uint8_t *symbols)
{
	get_out_t *o = (get_out_t*)ud;
	int64_t i, k;
	for (i = 0; i < n && !o->err; ++i) {
		const int64_t l = off[i + 1] - off[i], need = l + 64;
		uint8_t *p;
		if (end_row[i] < 0) continue; /* main.c:157: no such row */
		if (o->out.l + need > o->out.m) {
			const int64_t m = (o->out.l + need) * 2;
			uint8_t *t = (uint8_t*)realloc(o->out.s, (size_t)m);
			if (t == 0) { o->err = 1; break; }
			o->out.s = t, o->out.m = m;
		}
		p = o->out.s + o->out.l;
		p += sprintf((char*)p, ">%ld %ld\n", (long)(o->rows ? o->rows[i0 + i] : i0 + i), (long)end_row[i]);
		for (k = 0; k < l; ++k) *p++ = (uint8_t)"$ACGTN"[symbols[off[i] + k] < 6 ? symbols[off[i] + k] : 5];
		*p++ = '\n';
		o->out.l = p - o->out.s;
		if (out_flush(&o->out, 0) < 0) o->err = 1;
	}
	return o->err ? -1 : 0;
}

static const struct option get_long_opts[] = {
	{ "gpu", required_argument, 0, 301 },
	{ "host-fmd", no_argument, 0, 308 },
	{ "all", no_argument, 0, 501 },
	{ "pieces", no_argument, 0, 502 },
	{ 0, 0, 0, 0 }
};

static int main_get(int argc, char *argv[])
{
	int c, device = 0, ret = 0, i, all = 0, pieces = 0;
	int64_t *rows, n = 0;
	rb3gpu_t *h;
	rb3gpu_retrieve_stats_t st;
	rb3gpu_pieces_stats_t pst;
	get_out_t o;
	optind = 1, opterr = 0;
	while ((c = getopt_long(argc, argv, "", get_long_opts, 0)) >= 0) {
		if (c == 301) device = atoi(optarg);
		else if (c == 308) g_host_fmd = 1;
		else if (c == 501) all = 1;
		else if (c == 502) pieces = 1;
	}
	if (argc - optind < (all ? 1 : 2)) {
		fprintf(stdout, "Usage: ropebwt3-amd get <idx.fmr> <int> [...]\n");
		return 0;
	}
	if (all && argc - optind > 1) {
		fprintf(stderr, "ERROR: get --all prints every sequence of the index and takes no row\n");
		return 1;
	}
	if ((h = open_index(device, argv[optind], 0)) == 0) return 1;
	rows = (int64_t*)malloc((size_t)(argc - optind) * 8);
	if (rows == 0) { fprintf(stderr, "ERROR: out of memory\n"); rb3gpu_destroy(h); return 1; }
	for (i = optind + 1; i < argc; ++i) rows[n++] = atol(argv[i]); /* main.c:155: `abc` is row 0 */
	memset(&o, 0, sizeof(o));
	o.rows = all ? 0 : rows;
	if (all) c = rb3gpu_retrieve_pieces(h, -1, 0, get_sink, &o, &pst);
	else if (pieces) c = rb3gpu_retrieve_pieces(h, n, rows, get_sink, &o, &pst);
	else c = rb3gpu_retrieve(h, n, rows, get_sink, &o, &st);
	if (c == 0 && !o.err && out_flush(&o.out, 1) < 0) o.err = 1;
	if (c != 0 && !o.err) { fprintf(stderr, "ERROR: the GPU engine failed to retrieve the sequences: %s\n", rb3gpu_strerror(c)); ret = 1; }
	else if (o.err || fflush(stdout) != 0) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
	if (rb3h_verbose >= 3 && ret == 0 && (all || pieces))
		fprintf(stderr, "[M::%s::%.3f*%.2f] %lld rows, %lld symbols in %lld slice(s): %lld pieces, the longest of %lld steps, %lld LF steps; %.3f ms in the engine, pieces %.3f ms, join %.3f ms, sort %.3f ms, writing walk %.3f ms\n",
				__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)pst.n_rows, (long long)pst.n_symbols, (long long)pst.n_slices, (long long)pst.n_pieces, (long long)pst.max_piece_steps, (long long)pst.n_steps,
				pst.ms_total, pst.ms_pieces, pst.ms_join, pst.ms_sort, pst.ms_emit);
	else if (rb3h_verbose >= 3 && ret == 0)
		fprintf(stderr, "[M::%s::%.3f*%.2f] %lld rows, %lld symbols in %lld slice(s): %lld LF steps; %.3f ms in the engine, counting walk %.3f ms, writing walk %.3f ms\n",
				__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)st.n_rows, (long long)st.n_symbols, (long long)st.n_slices, (long long)st.n_steps, st.ms_total, st.ms_count, st.ms_emit);
	free(o.out.s); free(rows);
	rb3gpu_destroy(h);
	return ret;
}

/* remove [-d|-b|-e] [-o FILE] [--pieces] [--pair] [-f FILE] <idx> [<int>|<int>-<int> ...] (no counterpart in the reference): the index without the
 * sequences named, through ONE call of rb3gpu_remove, written like the output of `merge` (FMR unless -d or -e).  An argument is a string number (a row below acc[1])
 * or an inclusive range; -f adds one per line; --pair reads every number i as sequence i of an index of both strands, rows 2i and 2i + 1 (input order only: in a sorted order the strands of a
 * sequence stand where their order puts them, and --pair is refused).  Nothing is guessed: an
 * argument that is no number or range, a row outside the index, no row at all and a request that leaves no sequence are one line on stderr each, exit 1, nothing
 * written.  The index's .ssa and .len.gz do not fit the output and are not rewritten. */
typedef struct { int64_t *a; int64_t n, m; } rowvec_t;

static int rowvec_add(rowvec_t *v, const char *arg, int pair, int64_t n_str)
{
	int64_t a, b, i;
	if (rb3h_parse_rows(arg, &a, &b) < 0) { fprintf(stderr, "ERROR: remove: '%s' is neither a row number nor a range A-B\n", arg); return -1; }
	if (pair) { /* sequence i: rows 2i and 2i + 1 */
		if (b >= n_str / 2) { fprintf(stderr, "ERROR: remove: sequence %ld is outside the index (%ld sequences)\n", (long)b, (long)(n_str / 2)); return -1; }
		a *= 2, b = 2 * b + 1;
	} else if (b >= n_str) { fprintf(stderr, "ERROR: remove: row %ld is outside the index (%ld strings)\n", (long)b, (long)n_str); return -1; }
	if (v->n + (b - a + 1) > v->m) {
		int64_t *t;
		v->m = (v->n + (b - a + 1)) * 2;
		if ((t = (int64_t*)realloc(v->a, (size_t)v->m * 8)) == 0) { fprintf(stderr, "ERROR: out of memory\n"); return -1; }
		v->a = t;
	}
	for (i = a; i <= b; ++i) v->a[v->n++] = i;
	return 0;
}

static const struct option remove_long_opts[] = {
	{ "gpu", required_argument, 0, 301 },
	{ "host-fmd", no_argument, 0, 308 },
	{ "bre-run-bytes", required_argument, 0, 311 },
	{ "pieces", no_argument, 0, 502 },
	{ "pair", no_argument, 0, 503 },
	{ 0, 0, 0, 0 }
};

static int main_remove(int argc, char *argv[])
{
	int c, i, ret = 0, fmt = FMT_FMR, device = 0, pieces = 0, pair = 0;
	const char *fn_out = 0, *fn_rows = 0;
	int64_t acc[7];
	rowvec_t rv = { 0, 0, 0 };
	rb3gpu_remove_stats_t st;
	rb3gpu_t *h;
	bopt_t opt;
	bopt_init(&opt);
	optind = 1;
	while ((c = getopt_long(argc, argv, "dbeo:f:", remove_long_opts, 0)) >= 0) {
		if (c == 'd') fmt = FMT_FMD;
		else if (c == 'b') fmt = FMT_FMR;
		else if (c == 'e') fmt = FMT_BRE;
		else if (c == 'o') fn_out = optarg;
		else if (c == 'f') fn_rows = optarg;
		else if (c == 301) device = atoi(optarg);
		else if (c == 308) g_host_fmd = 1;
		else if (c == 311) g_bre_run_bytes = atoi(optarg);
		else if (c == 502) pieces = 1;
		else if (c == 503) pair = 1;
		else if (c == '?') return 1;
	}
	if (argc - optind < 1) {
		fprintf(stderr, "Usage: ropebwt3-amd remove [options] <idx.fmd|fmr|bre> [<int>|<int>-<int> ...]\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  -b / -d / -e   output FMR (default, as merge) / FMD / BRE\n");
		fprintf(stderr, "  --bre-run-bytes INT  bytes of a run length in a BRE record, 1..4 [2]\n");
		fprintf(stderr, "  -o FILE        output to FILE [stdout]\n");
		fprintf(stderr, "  -f FILE        read further rows or ranges from FILE, one per line\n");
		fprintf(stderr, "  --pair         a number i is sequence i of an index of both strands in input order: rows 2i and 2i+1\n");
		fprintf(stderr, "  --pieces       mark the rows through the walk in pieces (long sequences)\n");
		fprintf(stderr, "  --gpu INT      HIP device ordinal [0]\n");
		return 1;
	}
	if (fmt == FMT_BRE && (g_bre_run_bytes < 1 || g_bre_run_bytes > 4)) { fprintf(stderr, "ERROR: --bre-run-bytes takes 1 to 4\n"); return 1; }
	opt.so = index_order(argv[optind]); /* (an FMR output carries the order of its input) */
	c = rb3h_verbose;
	if (rb3h_verbose > 2) rb3h_verbose = 2; /* (the command may still refuse its rows with ONE line: the loading says nothing but errors and warnings until they are accepted) */
	h = open_index(device, argv[optind], 0);
	rb3h_verbose = c;
	if (h == 0) return 1;
	rb3gpu_tune(h, "verbose", rb3h_verbose);
	rb3gpu_get_acc(h, acc);
	if (pair && opt.so != RB3GPU_SO_IO) { fprintf(stderr, "ERROR: remove: --pair numbers the sequences in input order; the strings of this index are sorted (build -s / -r): name the rows\n"); ret = 1; }
	else if (pair && !both_strands(acc)) ret = 1;
	for (i = optind + 1; i < argc && ret == 0; ++i)
		if (rowvec_add(&rv, argv[i], pair, acc[1]) < 0) ret = 1;
	if (fn_rows && ret == 0) {
		FILE *fp = strcmp(fn_rows, "-") == 0 ? stdin : fopen(fn_rows, "r");
		char line[256];
		if (fp == 0) { fprintf(stderr, "ERROR: remove: failed to open '%s'\n", fn_rows); ret = 1; }
		while (ret == 0 && fgets(line, sizeof(line), fp)) {
			size_t l = strlen(line);
			while (l > 0 && (line[l - 1] == '\n' || line[l - 1] == '\r')) line[--l] = 0;
			if (l == 0) continue;
			if (rowvec_add(&rv, line, pair, acc[1]) < 0) ret = 1;
		}
		if (fp && fp != stdin) fclose(fp);
	}
	if (ret == 0 && rv.n == 0) { fprintf(stderr, "ERROR: remove: no row to remove\n"); ret = 1; }
	if (ret == 0) {
		c = rb3gpu_remove(h, rv.n, rv.a, pieces, &st);
		if (c == RB3GPU_EINVAL) { fprintf(stderr, "ERROR: remove: nothing would be left of the index\n"); ret = 1; } /* (rows outside the index never get here) */
		else if (c != 0) { fprintf(stderr, "ERROR: the GPU engine failed to remove the sequences: %s\n", rb3gpu_strerror(c)); ret = 1; }
	}
	if (ret == 0 && rb3h_verbose >= 3)
		fprintf(stderr, "[M::%s::%.3f*%.2f] removed %lld strings, %lld rows ($ACGTN: %lld %lld %lld %lld %lld %lld): %lld LF steps, %lld pieces, the longest of %lld steps; %.3f ms in the engine, marking %.3f ms, rebuild %.3f ms\n",
				__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)st.n_strings, (long long)st.n_rows, (long long)st.removed[0], (long long)st.removed[1], (long long)st.removed[2], (long long)st.removed[3],
				(long long)st.removed[4], (long long)st.removed[5], (long long)st.n_steps, (long long)st.n_pieces, (long long)st.max_piece_steps, st.ms_total, st.ms_mark, st.ms_build);
	if (ret == 0 && fn_out && freopen(fn_out, "wb", stdout) == 0) { fprintf(stderr, "ERROR: remove: failed to open '%s' for writing\n", fn_out); ret = 1; }
	if (ret == 0) {
		c = fmt == FMT_FMR ? dump_fmr(h, &opt, stdout) : fmt == FMT_FMD ? write_fmd(h, stdout) : write_bre(h, stdout);
		if (c != 0 || fflush(stdout) != 0) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
	}
	free(rv.a);
	rb3gpu_destroy(h);
	return ret;
}

/* dedup [--pair] [--dup-only] [--table] <idx> (no counterpart in the reference): the sequences that are exact copies of another one or lie wholly inside a
 * longer one, through ONE call of rb3gpu_dedup.  The output is the list `remove -f` reads: the units to drop, one bare number per line, ascending -- rows, or with
 * --pair sequences of an index of both strands in input order, where a copy of a reverse complement is a copy too.  --table: every unit with its kind (K kept,
 * D duplicate, C contained), the keeper of its class, occ and copies of its (forward) row.  Nothing to drop is no output and exit 0.  --pair on a sorted index or on
 * one strand, a further argument and a file that is no index are one line on stderr each, exit 1, nothing on stdout. */
static const struct option dedup_long_opts[] = {
	{ "gpu", required_argument, 0, 301 },
	{ "pair", no_argument, 0, 503 },
	{ "dup-only", no_argument, 0, 504 },
	{ "table", no_argument, 0, 505 },
	{ 0, 0, 0, 0 }
};

static int main_dedup(int argc, char *argv[])
{
	int c, ret = 0, device = 0, pair = 0, dup_only = 0, table = 0;
	int64_t acc[7], nu = 0, u;
	uint8_t *kind = 0;
	int64_t *keeper = 0;
	rb3gpu_dedup_rec_t *rec = 0;
	rb3gpu_dedup_stats_t st;
	rb3gpu_t *h;
	index_host_t ih;
	rb3h_buf_t out;
	optind = 1;
	while ((c = getopt_long(argc, argv, "", dedup_long_opts, 0)) >= 0) {
		if (c == 301) device = atoi(optarg);
		else if (c == 503) pair = 1;
		else if (c == 504) dup_only = 1;
		else if (c == 505) table = 1;
		else if (c == '?') return 1;
	}
	if (argc - optind < 1) {
		fprintf(stderr, "Usage: ropebwt3-amd dedup [options] <idx.fmd|fmr|bre>\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  --pair         a unit is sequence i of an index of both strands in input order: rows 2i and 2i+1\n");
		fprintf(stderr, "  --dup-only     exact copies only: a sequence inside a longer one stays\n");
		fprintf(stderr, "  --table        every unit: number, kind (K kept, D duplicate, C contained), keeper, occurrences, copies\n");
		fprintf(stderr, "  --gpu INT      HIP device ordinal [0]\n");
		fprintf(stderr, "Output: the units to drop, one per line: what `remove [--pair] -f -` reads\n");
		return 1;
	}
	if (argc - optind > 1) { fprintf(stderr, "ERROR: dedup: takes one index and nothing else ('%s')\n", argv[optind + 1]); return 1; }
	if (pair && index_order(argv[optind]) != RB3GPU_SO_IO) {
		fprintf(stderr, "ERROR: dedup: --pair numbers the sequences in input order; the strings of this index are sorted (build -s / -r): run it without --pair\n");
		return 1;
	}
	memset(&ih, 0, sizeof(ih));
	memset(&out, 0, sizeof(out));
	c = rb3h_verbose;
	rb3h_verbose = 0; /* (the command refuses with ONE line: the loading says nothing until the index is accepted) */
	if (index_host_read(argv[optind], &ih) < 0) {
		rb3h_verbose = c;
		fprintf(stderr, "ERROR: dedup: '%s' is not an index\n", argv[optind]);
		return 1;
	}
	rb3h_verbose = c > 2 ? 2 : c;
	h = open_index(device, argv[optind], &ih);
	rb3h_verbose = c;
	if (h == 0) return 1;
	rb3gpu_tune(h, "verbose", rb3h_verbose);
	rb3gpu_get_acc(h, acc);
	if (pair && !both_strands(acc)) ret = 1;
	if (ret == 0) {
		nu = pair ? acc[1] / 2 : acc[1];
		kind = (uint8_t*)malloc((size_t)nu + 1);
		keeper = (int64_t*)malloc((size_t)(nu + 1) * 8);
		if (table) rec = (rb3gpu_dedup_rec_t*)malloc((size_t)(acc[1] + 1) * sizeof(*rec));
		if (kind == 0 || keeper == 0 || (table && rec == 0)) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; }
	}
	if (ret == 0) {
		c = rb3gpu_dedup(h, pair, dup_only, kind, keeper, rec, &st);
		if (c == RB3GPU_EINVAL && pair) { fprintf(stderr, "ERROR: dedup: --pair: rows 2i and 2i+1 of this index are not the two strands of a sequence\n"); ret = 1; }
		else if (c != 0) { fprintf(stderr, "ERROR: the GPU engine failed to compare the sequences: %s\n", rb3gpu_strerror(c)); ret = 1; }
	}
	for (u = 0; u < nu && ret == 0; ++u) {
		if (!table && kind[u] == 'K') continue;
		if (out.l + 128 > out.m) {
			const int64_t m = (out.l + 128) * 2;
			uint8_t *t = (uint8_t*)realloc(out.s, (size_t)m);
			if (t == 0) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; break; }
			out.s = t, out.m = m;
		}
		if (table) out.l += sprintf((char*)out.s + out.l, "%ld\t%c\t%ld\t%ld\t%ld\n", (long)u, kind[u], (long)keeper[u], (long)rec[pair ? 2 * u : u].occ, (long)rec[pair ? 2 * u : u].copies);
		else out.l += sprintf((char*)out.s + out.l, "%ld\n", (long)u);
		if (out_flush(&out, 0) < 0) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
	}
	if (ret == 0 && (out_flush(&out, 1) < 0 || fflush(stdout) != 0)) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
	if (ret == 0 && rb3h_verbose >= 3)
		fprintf(stderr, "[M::%s::%.3f*%.2f] %lld strings: %lld duplicates, %lld contained, %lld classes of copies; %lld steps in %lld slice(s), %lld walks ended early; %.3f ms in the engine, walk %.3f ms\n",
				__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)st.n_strings, (long long)st.n_dup, (long long)st.n_contained, (long long)st.n_classes, (long long)st.n_steps,
				(long long)st.n_slices, (long long)st.n_early, st.ms_total, st.ms_walk);
	free(out.s); free(kind); free(keeper); free(rec);
	rb3gpu_destroy(h);
	return ret;
}

/* overlap [-l INT] [-c INT] [--pair] [--reduce] <idx> (no counterpart in the reference): the suffix-prefix overlaps of the indexed sequences, through
 * ONE call of rb3gpu_overlap -- with --reduce of rb3gpu_overlap_reduced: the same lines for the irreducible overlaps only; more overlaps than it may hold on the device and
 * more than the device's memory takes are one line on stderr each, exit 1, nothing on stdout.  One line per record: a, b, len, len_a, len_b -- the last len symbols of
 * row a are the first len of row b; by a, then longest first, then in the index's order of the partners.  --pair: i, strand_i, j, strand_j, len, len_i, len_j with sequence i = row >> 1 of an index of both strands in input order, + for an
 * even row and - for an odd one; both views of an overlap are printed.  -l below 1, -c below 0, --pair on a sorted index or on one strand, a further argument and a
 * file that is no index are one line on stderr each, exit 1, nothing on stdout. */
static const struct option overlap_long_opts[] = {
	{ "gpu", required_argument, 0, 301 },
	{ "pair", no_argument, 0, 503 },
	{ "reduce", no_argument, 0, 504 },
	{ 0, 0, 0, 0 }
};

typedef struct { const int64_t *len; rb3h_buf_t out; int pair, err; } overlap_out_t;

static int overlap_sink(void *ud, int64_t n, const rb3gpu_overlap_rec_t *recs)
{
	overlap_out_t *o = (overlap_out_t*)ud;
	int64_t i;
	for (i = 0; i < n && !o->err; ++i) {
		const rb3gpu_overlap_rec_t *r = &recs[i];
		if (o->out.l + 160 > o->out.m) {
			const int64_t m = (o->out.l + 160) * 2;
			uint8_t *t = (uint8_t*)realloc(o->out.s, (size_t)m);
			if (t == 0) { o->err = 1; break; }
			o->out.s = t, o->out.m = m;
		}
		if (o->pair) o->out.l += sprintf((char*)o->out.s + o->out.l, "%d\t%c\t%d\t%c\t%d\t%ld\t%d\n", r->a >> 1, "+-"[r->a & 1], r->b >> 1, "+-"[r->b & 1], r->len, (long)o->len[r->a], r->len_b);
		else o->out.l += sprintf((char*)o->out.s + o->out.l, "%d\t%d\t%d\t%ld\t%d\n", r->a, r->b, r->len, (long)o->len[r->a], r->len_b);
		if (out_flush(&o->out, 0) < 0) o->err = 2;
	}
	return o->err;
}

static int main_overlap(int argc, char *argv[])
{
	int c, ret = 0, device = 0, pair = 0, reduce = 0;
	int64_t acc[7], min_len = 31, max_hits = 0, *len = 0;
	rb3gpu_overlap_stats_t st;
	rb3gpu_reduce_stats_t rs;
	rb3gpu_t *h;
	index_host_t ih;
	overlap_out_t o;
	optind = 1;
	while ((c = getopt_long(argc, argv, "l:c:", overlap_long_opts, 0)) >= 0) {
		if (c == 301) device = atoi(optarg);
		else if (c == 503) pair = 1;
		else if (c == 504) reduce = 1;
		else if (c == 'l') min_len = atol(optarg);
		else if (c == 'c') max_hits = atol(optarg);
		else if (c == '?') return 1;
	}
	if (argc - optind < 1) {
		fprintf(stderr, "Usage: ropebwt3-amd overlap [options] <idx.fmd|fmr|bre>\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  -l INT         min overlap length [%ld]\n", (long)min_len);
		fprintf(stderr, "  -c INT         leave out an overlap shared with more than INT partners (0: none) [%ld]\n", (long)max_hits);
		fprintf(stderr, "  --pair         name sequence i of an index of both strands in input order and its strand: rows 2i (+) and 2i+1 (-)\n");
		fprintf(stderr, "  --reduce       only the irreducible overlaps: leave out a -> b where a longer a -> c and c -> b put b at the same place (after -c)\n");
		fprintf(stderr, "  --gpu INT      HIP device ordinal [0]\n");
		fprintf(stderr, "Output: a, b, len, len_a, len_b per overlap: the last len symbols of a are the first len of b (--pair: i, strand, j, strand, len, len_i, len_j)\n");
		return 1;
	}
	if (min_len < 1) { fprintf(stderr, "ERROR: overlap: -l takes a length of at least 1\n"); return 1; }
	if (max_hits < 0) { fprintf(stderr, "ERROR: overlap: -c takes a number of partners, 0 for no limit\n"); return 1; }
	if (argc - optind > 1) { fprintf(stderr, "ERROR: overlap: takes one index and nothing else ('%s')\n", argv[optind + 1]); return 1; }
	if (pair && index_order(argv[optind]) != RB3GPU_SO_IO) {
		fprintf(stderr, "ERROR: overlap: --pair numbers the sequences in input order; the strings of this index are sorted (build -s / -r): run it without --pair\n");
		return 1;
	}
	memset(&ih, 0, sizeof(ih));
	memset(&o, 0, sizeof(o));
	c = rb3h_verbose;
	rb3h_verbose = 0; /* (the command refuses with ONE line: the loading says nothing until the index is accepted) */
	if (index_host_read(argv[optind], &ih) < 0) {
		rb3h_verbose = c;
		fprintf(stderr, "ERROR: overlap: '%s' is not an index\n", argv[optind]);
		return 1;
	}
	rb3h_verbose = c > 2 ? 2 : c;
	h = open_index(device, argv[optind], &ih);
	rb3h_verbose = c;
	if (h == 0) return 1;
	rb3gpu_tune(h, "verbose", rb3h_verbose);
	rb3gpu_get_acc(h, acc);
	if (pair && !both_strands(acc)) ret = 1;
	if (ret == 0) {
		len = (int64_t*)malloc((size_t)(acc[1] + 1) * 8);
		if (len == 0) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; }
	}
	if (ret == 0) {
		o.len = len, o.pair = pair;
		if (reduce) c = rb3gpu_overlap_reduced(h, min_len, max_hits, len, overlap_sink, &o, &rs);
		else c = rb3gpu_overlap(h, min_len, max_hits, len, overlap_sink, &o, &st);
		if (o.err == 1) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; }
		else if (o.err == 2) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
		else if (reduce && c == RB3GPU_EUNSUP) { fprintf(stderr, "ERROR: overlap: --reduce holds all the overlaps on the device, and there are more than RB3GPU_OVL_RESIDENT allows: raise -l, set -c, or run it without --reduce\n"); ret = 1; }
		else if (reduce && c == RB3GPU_ENOMEM) { fprintf(stderr, "ERROR: overlap: --reduce holds all the overlaps on the device, and there are more than its memory takes: raise -l, set -c, or run it without --reduce\n"); ret = 1; }
		else if (c != 0) { fprintf(stderr, "ERROR: the GPU engine failed to find the overlaps: %s\n", rb3gpu_strerror(c)); ret = 1; }
	}
	if (ret == 0 && (out_flush(&o.out, 1) < 0 || fflush(stdout) != 0)) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
	if (ret == 0 && rb3h_verbose >= 3 && reduce)
		fprintf(stderr, "[M::%s::%.3f*%.2f] %lld strings: %lld overlaps in %lld groups of %lld strings, %lld kept by --reduce, %lld groups of %lld partners over -c; %lld slice(s), %lld bytes resident; %.3f ms in the engine: count %.3f, who %.3f, emit %.3f, reduce %.3f, compact %.3f ms\n",
				__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)rs.n_strings, (long long)rs.n_hits, (long long)rs.n_groups, (long long)rs.n_emitters, (long long)rs.n_kept, (long long)rs.n_capped_groups,
				(long long)rs.n_capped_hits, (long long)rs.n_slices, (long long)rs.resident_bytes, rs.ms_total, rs.ms_count, rs.ms_who, rs.ms_emit, rs.ms_reduce, rs.ms_compact);
	else if (ret == 0 && rb3h_verbose >= 3)
		fprintf(stderr, "[M::%s::%.3f*%.2f] %lld strings: %lld overlaps in %lld groups of %lld strings, %lld groups of %lld partners over -c; %lld + %lld steps, %lld walks ended early, %lld slice(s); %.3f ms in the engine: count %.3f, who %.3f, emit %.3f ms\n",
				__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)st.n_strings, (long long)st.n_hits, (long long)st.n_groups, (long long)st.n_emitters, (long long)st.n_capped_groups,
				(long long)st.n_capped_hits, (long long)st.n_steps_count, (long long)st.n_steps_emit, (long long)st.n_early, (long long)st.n_slices, st.ms_total, st.ms_count, st.ms_who, st.ms_emit);
	free(o.out.s); free(len);
	rb3gpu_destroy(h);
	return ret;
}

/* unitig [-l INT] [-c INT] [--pair] [--gfa | --table] <idx> (no counterpart in the reference): the unambiguous paths of the string graph of the irreducible
 * overlaps (those of `overlap --reduce` with the same -l and -c), each spelled as one sequence, through ONE call of rb3gpu_unitigs.  Per unitig `>utg<id>`, LN:i: its
 * length, RC:i: its members, CL:i: the closing overlap of a circular one, then its letters on one line.  --gfa: H, one S line per unitig, one L line per overlap between
 * unitigs and one per circular unitig onto itself.  --table: a line per member instead: utg, rank, string (--pair: sequence, strand), offset, overlap with the member in
 * front.  --pair: an index of both strands in input order; one of every two mirror-image unitigs is printed.  -l below 1, -c below 0, --gfa with --table, --pair on a
 * sorted index or on one strand, a graph whose strands differ, more overlaps than may be held on the device, a further argument and a file that is no index are one
 * line on stderr each, exit 1, nothing on stdout. */
static const struct option unitig_long_opts[] = {
	{ "gpu", required_argument, 0, 301 },
	{ "pair", no_argument, 0, 503 },
	{ "gfa", no_argument, 0, 504 },
	{ "table", no_argument, 0, 505 },
	{ 0, 0, 0, 0 }
};

typedef struct { rb3h_buf_t out; int pair, mode, err; int64_t n_circ, m_circ, *circ; } unitig_out_t; /* mode 0: sequences, 1: GFA, 2: the table; circ: (id, overlap) of the circular ones */

static int unitig_room(unitig_out_t *o, int64_t need)
{
	if (o->out.l + need > o->out.m) {
		const int64_t m = (o->out.l + need) * 2;
		uint8_t *t = (uint8_t*)realloc(o->out.s, (size_t)m);
		if (t == 0) { o->err = 1; return -1; }
		o->out.s = t, o->out.m = m;
	}
	return 0;
}

static int unitig_sink(void *ud, int64_t u0, int64_t n, const rb3gpu_unitig_t *utg, const rb3gpu_unitig_member_t *mem, const int64_t *off, const uint8_t *symbols)
{
	unitig_out_t *o = (unitig_out_t*)ud;
	int64_t i, j, at = 0;
	for (i = 0; i < n && !o->err; at += utg[i].members, ++i) {
		const rb3gpu_unitig_t *u = &utg[i];
		const int64_t len = off[i + 1] - off[i];
		char *p;
		if (o->mode == 2) {
			for (j = 0; j < u->members && !o->err; ++j) {
				const rb3gpu_unitig_member_t *v = &mem[at + j];
				if (unitig_room(o, 160) < 0) break;
				p = (char*)o->out.s + o->out.l;
				if (o->pair) o->out.l += sprintf(p, "utg%ld\t%ld\t%d\t%c\t%ld\t%d\n", (long)(u0 + i), (long)j, v->row >> 1, "+-"[v->row & 1], (long)v->off, v->o_in);
				else o->out.l += sprintf(p, "utg%ld\t%ld\t%d\t%ld\t%d\n", (long)(u0 + i), (long)j, v->row, (long)v->off, v->o_in);
				if (out_flush(&o->out, 0) < 0) o->err = 2;
			}
			continue;
		}
		if (unitig_room(o, len + 160) < 0) break;
		p = (char*)o->out.s + o->out.l;
		p += o->mode == 1 ? sprintf(p, "S\tutg%ld\t", (long)(u0 + i)) : sprintf(p, ">utg%ld\tLN:i:%ld\tRC:i:%d", (long)(u0 + i), (long)u->len, u->members);
		if (o->mode == 0 && u->circ) p += sprintf(p, "\tCL:i:%d", u->circ);
		if (o->mode == 0) *p++ = '\n';
		for (j = 0; j < len; ++j) *p++ = "$ACGTN"[symbols[off[i] + j] < 6 ? symbols[off[i] + j] : 5];
		if (o->mode == 1) p += sprintf(p, "\tLN:i:%ld\tRC:i:%d", (long)u->len, u->members);
		*p++ = '\n';
		o->out.l = (uint8_t*)p - o->out.s;
		if (o->mode == 1 && u->circ) {
			if (o->n_circ == o->m_circ) {
				const int64_t m = o->m_circ ? o->m_circ * 2 : 16;
				int64_t *t = (int64_t*)realloc(o->circ, (size_t)m * 16);
				if (t == 0) { o->err = 1; break; }
				o->circ = t, o->m_circ = m;
			}
			o->circ[2 * o->n_circ] = u0 + i, o->circ[2 * o->n_circ + 1] = u->circ, ++o->n_circ;
		}
		if (out_flush(&o->out, 0) < 0) o->err = 2;
	}
	return o->err;
}

static int unitig_link_sink(void *ud, int64_t n, const rb3gpu_unitig_link_t *links)
{
	unitig_out_t *o = (unitig_out_t*)ud;
	int64_t i;
	for (i = 0; i < n && !o->err; ++i) {
		const rb3gpu_unitig_link_t *l = &links[i];
		if (unitig_room(o, 160) < 0) break;
		o->out.l += sprintf((char*)o->out.s + o->out.l, "L\tutg%d\t%c\tutg%d\t%c\t%dM\n", l->from, "+-"[l->from_rev & 1], l->to, "+-"[l->to_rev & 1], l->len);
		if (out_flush(&o->out, 0) < 0) o->err = 2;
	}
	return o->err;
}

static int main_unitig(int argc, char *argv[])
{
	int c, ret = 0, device = 0, pair = 0, gfa = 0, table = 0;
	int64_t acc[7], min_len = 31, max_hits = 0, i;
	rb3gpu_unitig_stats_t st;
	rb3gpu_t *h;
	index_host_t ih;
	unitig_out_t o;
	optind = 1;
	while ((c = getopt_long(argc, argv, "l:c:", unitig_long_opts, 0)) >= 0) {
		if (c == 301) device = atoi(optarg);
		else if (c == 503) pair = 1;
		else if (c == 504) gfa = 1;
		else if (c == 505) table = 1;
		else if (c == 'l') min_len = atol(optarg);
		else if (c == 'c') max_hits = atol(optarg);
		else if (c == '?') return 1;
	}
	if (argc - optind < 1) {
		fprintf(stderr, "Usage: ropebwt3-amd unitig [options] <idx.fmd|fmr|bre>\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  -l INT         min overlap length [%ld]\n", (long)min_len);
		fprintf(stderr, "  -c INT         leave out an overlap shared with more than INT partners (0: none) [%ld]\n", (long)max_hits);
		fprintf(stderr, "  --pair         an index of both strands in input order: one of every two mirror-image unitigs, links with orientations\n");
		fprintf(stderr, "  --gfa          GFA 1.0: S lines, L lines for the overlaps between unitigs and for circular unitigs\n");
		fprintf(stderr, "  --table        a line per member instead of sequences: utg, rank, string (--pair: sequence, strand), offset, overlap\n");
		fprintf(stderr, "  --gpu INT      HIP device ordinal [0]\n");
		fprintf(stderr, "Output: >utg<id> LN:i:<length> RC:i:<members> [CL:i:<closing overlap of a circular one>], then the letters on one line\n");
		return 1;
	}
	if (min_len < 1) { fprintf(stderr, "ERROR: unitig: -l takes a length of at least 1\n"); return 1; }
	if (max_hits < 0) { fprintf(stderr, "ERROR: unitig: -c takes a number of partners, 0 for no limit\n"); return 1; }
	if (gfa && table) { fprintf(stderr, "ERROR: unitig: --gfa and --table are two outputs: name one\n"); return 1; }
	if (argc - optind > 1) { fprintf(stderr, "ERROR: unitig: takes one index and nothing else ('%s')\n", argv[optind + 1]); return 1; }
	if (pair && index_order(argv[optind]) != RB3GPU_SO_IO) {
		fprintf(stderr, "ERROR: overlap: --pair numbers the sequences in input order; the strings of this index are sorted (build -s / -r): run it without --pair\n");
		return 1;
	}
	memset(&ih, 0, sizeof(ih));
	memset(&o, 0, sizeof(o));
	memset(&st, 0, sizeof(st));
	c = rb3h_verbose;
	rb3h_verbose = 0; /* (the command refuses with ONE line: the loading says nothing until the index is accepted) */
	if (index_host_read(argv[optind], &ih) < 0) {
		rb3h_verbose = c;
		fprintf(stderr, "ERROR: unitig: '%s' is not an index\n", argv[optind]);
		return 1;
	}
	rb3h_verbose = c > 2 ? 2 : c;
	h = open_index(device, argv[optind], &ih);
	rb3h_verbose = c;
	if (h == 0) return 1;
	rb3gpu_tune(h, "verbose", rb3h_verbose);
	rb3gpu_get_acc(h, acc);
	if (pair && !both_strands(acc)) ret = 1;
	if (ret == 0) {
		o.pair = pair, o.mode = gfa ? 1 : table ? 2 : 0;
		if (gfa && unitig_room(&o, 160) == 0) o.out.l += sprintf((char*)o.out.s, "H\tVN:Z:1.0\n");
		c = o.err ? 0 : rb3gpu_unitigs(h, min_len, max_hits, pair, unitig_sink, &o, gfa ? unitig_link_sink : 0, &st);
		for (i = 0; i < o.n_circ && c == 0 && !o.err; ++i)
			if (unitig_room(&o, 160) == 0) o.out.l += sprintf((char*)o.out.s + o.out.l, "L\tutg%ld\t+\tutg%ld\t+\t%ldM\n", (long)o.circ[2 * i], (long)o.circ[2 * i], (long)o.circ[2 * i + 1]);
		if (o.err == 1) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; }
		else if (o.err == 2) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
		else if (c == RB3GPU_EUNSUP && st.n_asym > 0) { fprintf(stderr, "ERROR: unitig: --pair needs the same graph on both strands, and %ld overlaps have no mirror image (contained sequences or -c do that): run dedup --pair | remove --pair first, drop -c, or run it without --pair\n", (long)st.n_asym); ret = 1; }
		else if (c == RB3GPU_EUNSUP) { fprintf(stderr, "ERROR: overlap: --reduce holds all the overlaps on the device, and there are more than RB3GPU_OVL_RESIDENT allows: raise -l, set -c, or run it without --reduce\n"); ret = 1; }
		else if (c == RB3GPU_ENOMEM) { fprintf(stderr, "ERROR: overlap: --reduce holds all the overlaps on the device, and there are more than its memory takes: raise -l, set -c, or run it without --reduce\n"); ret = 1; }
		else if (c != 0) { fprintf(stderr, "ERROR: the GPU engine failed to build the unitigs: %s\n", rb3gpu_strerror(c)); ret = 1; }
	}
	if (ret == 0 && (out_flush(&o.out, 1) < 0 || fflush(stdout) != 0)) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
	if (ret == 0 && rb3h_verbose >= 3)
		fprintf(stderr, "[M::%s::%.3f*%.2f] %lld strings: %lld kept overlaps, %lld simple; %lld unitigs of %lld members and %lld symbols, %lld circular, longest %lld members, %lld links; %lld rounds, %lld steps, %lld slice(s), %lld bytes resident; %.3f ms in the engine: reduce %.3f, graph %.3f, rank %.3f, emit %.3f ms\n",
				__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)st.n_strings, (long long)st.n_kept, (long long)st.n_simple, (long long)st.n_unitigs, (long long)st.n_members, (long long)st.n_symbols,
				(long long)st.n_cycles, (long long)st.max_members, (long long)st.n_links, (long long)st.n_rounds, (long long)st.n_steps_emit, (long long)st.n_slices, (long long)st.resident_bytes,
				st.ms_total, st.ms_reduce, st.ms_graph, st.ms_rank, st.ms_emit);
	free(o.out.s); free(o.circ);
	rb3gpu_destroy(h);
	return ret;
}

/* fetch [-f FILE] [--row] [-s INT] <idx> [region ...] (no counterpart in the reference): regions of the indexed sequences through the sampled suffix array,
 * ONE call of rb3gpu_fetch.  A region is the word name:beg-end[:+|:-] (rb3h_region_parse: 0-based, end-exclusive, the name cut at the last colons); -f adds BED lines.
 * Named regions need <idx>.ssa and <idx>.len.gz and an index of both strands in input order: sequence i forward is row 2i, region as given; strand - is row 2i + 1,
 * region [len - end, len - beg), the reverse complement of the forward region read straight off the index.  --row: the name is a string number of `get`, only the .ssa
 * is needed and any index will do.  -s INT: where <idx>.ssa is absent the samples are made on the device at that rate.  Per region `>` and the region as it was asked
 * (a BED line as name:beg-end[:strand]), then a line of $ACGTN letters.  Nothing is guessed: a word that is no region, an unknown name, an end beyond the sequence and no
 * region at all are one line on stderr each, exit 1, nothing on stdout. */
typedef struct { char *label; int64_t name_len, beg, end; int strand; } fetch_req_t;
typedef struct { const fetch_req_t *q; rb3h_buf_t out; int err; } fetch_out_t;

static int fetch_sink(void *ud, int64_t i0, int64_t n, const int64_t *off, const uint8_t *symbols)
{
	fetch_out_t *o = (fetch_out_t*)ud;
	int64_t i, k;
	for (i = 0; i < n && !o->err; ++i) {
		const char *label = o->q[i0 + i].label;
		const int64_t l = off[i + 1] - off[i], ll = (int64_t)strlen(label), need = l + ll + 8;
		uint8_t *p;
		if (o->out.l + need > o->out.m) {
			const int64_t m = (o->out.l + need) * 2;
			uint8_t *t = (uint8_t*)realloc(o->out.s, (size_t)m);
			if (t == 0) { o->err = 1; break; }
			o->out.s = t, o->out.m = m;
		}
		p = o->out.s + o->out.l;
		*p++ = '>';
		memcpy(p, label, (size_t)ll), p += ll;
		*p++ = '\n';
		for (k = 0; k < l; ++k) *p++ = (uint8_t)"$ACGTN"[symbols[off[i] + k] < 6 ? symbols[off[i] + k] : 5];
		*p++ = '\n';
		o->out.l = p - o->out.s;
		if (out_flush(&o->out, 0) < 0) o->err = 1;
	}
	return o->err ? -1 : 0;
}

typedef struct { fetch_req_t *a; int64_t n, m; } fetch_vec_t;

static int fetch_add(fetch_vec_t *v, const char *str, int bed)
{
	rb3h_region_t r;
	fetch_req_t *q;
	if (rb3h_region_parse(str, bed, &r) < 0) {
		size_t l = strlen(str);
		while (l > 0 && (str[l - 1] == '\n' || str[l - 1] == '\r')) --l;
		fprintf(stderr, "ERROR: fetch: '%.*s' is no region%s\n", (int)l, str, bed ? " (BED: name, beg, end in columns 1-3, beg < end)" : " name:beg-end (0-based, beg < end)");
		return -1;
	}
	if (v->n == v->m) {
		fetch_req_t *t;
		v->m = v->m ? v->m * 2 : 64;
		if ((t = (fetch_req_t*)realloc(v->a, (size_t)v->m * sizeof(*t))) == 0) { fprintf(stderr, "ERROR: out of memory\n"); return -1; }
		v->a = t;
	}
	q = &v->a[v->n];
	q->name_len = r.name_len, q->beg = r.beg, q->end = r.end, q->strand = r.strand;
	if (bed) {
		if ((q->label = (char*)malloc((size_t)r.name_len + 64)) == 0) { fprintf(stderr, "ERROR: out of memory\n"); return -1; }
		memcpy(q->label, str, (size_t)r.name_len);
		sprintf(q->label + r.name_len, ":%ld-%ld%s", (long)r.beg, (long)r.end, !r.stranded ? "" : r.strand < 0 ? ":-" : ":+");
	} else if ((q->label = strdup(str)) == 0) { fprintf(stderr, "ERROR: out of memory\n"); return -1; }
	++v->n;
	return 0;
}

static const rb3h_sid_t *g_fetch_sid; /* (qsort and bsearch take no context) */

static int fetch_name_cmp(const void *a, const void *b) { return strcmp(g_fetch_sid->name[*(const int64_t*)a], g_fetch_sid->name[*(const int64_t*)b]); }

/* the sequence of that name, -1 if there is none (of several of one name: any) */
static int64_t fetch_lookup(const rb3h_sid_t *sid, const int64_t *by_name, const char *name, int64_t name_len)
{
	int64_t lo = 0, hi = sid->n_seq;
	while (lo < hi) {
		const int64_t mid = (lo + hi) >> 1;
		const char *s = sid->name[by_name[mid]];
		int c = strncmp(s, name, (size_t)name_len);
		if (c == 0 && s[name_len] != 0) c = 1;
		if (c == 0) return by_name[mid];
		if (c < 0) lo = mid + 1; else hi = mid;
	}
	return -1;
}

static const struct option fetch_long_opts[] = {
	{ "gpu", required_argument, 0, 301 },
	{ "host-fmd", no_argument, 0, 308 },
	{ "row", no_argument, 0, 504 },
	{ 0, 0, 0, 0 }
};

static int main_fetch(int argc, char *argv[])
{
	int c, i, ret = 0, device = 0, by_row = 0, ss = -1, ms;
	const char *fn_bed = 0;
	int64_t acc[7], m, n_sym, k, bad = -1, *by_name = 0;
	fetch_vec_t rv = { 0, 0, 0 };
	rb3gpu_region_t *reg = 0;
	rb3gpu_fetch_stats_t st;
	rb3h_ssa_t *sa = 0;
	rb3h_sid_t *sid = 0;
	index_host_t ih;
	rb3gpu_t *h = 0;
	fetch_out_t o;
	optind = 1;
	while ((c = getopt_long(argc, argv, "f:s:", fetch_long_opts, 0)) >= 0) {
		if (c == 'f') fn_bed = optarg;
		else if (c == 's') ss = atoi(optarg);
		else if (c == 301) device = atoi(optarg);
		else if (c == 308) g_host_fmd = 1;
		else if (c == 504) by_row = 1;
		else if (c == '?') return 1;
	}
	if (argc - optind < 1) {
		fprintf(stdout, "Usage: ropebwt3-amd fetch [options] <idx.fmd|fmr|bre> [name:beg-end[:+|:-] ...]\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  -f FILE     read further regions from the BED file FILE (columns 1-3, strand from column 6)\n");
		fprintf(stderr, "  --row       the name of a region is a string number of `get`; needs <idx>.ssa only\n");
		fprintf(stderr, "  -s INT      where <idx>.ssa is absent, sample the suffix array at rate 2^INT on the device\n");
		fprintf(stderr, "  --gpu INT   HIP device ordinal [0]\n");
		fprintf(stderr, "Regions are 0-based and end-exclusive; named regions need <idx>.ssa and <idx>.len.gz\n");
		return 0;
	}
	if (ss > 40) { fprintf(stderr, "ERROR: fetch: -s takes 0 to 40\n"); return 1; }
	memset(&ih, 0, sizeof(ih));
	memset(&o, 0, sizeof(o));
	/* 1. the regions as they are written: nothing else is looked at before every one of them is one */
	for (i = optind + 1; i < argc && ret == 0; ++i)
		if (fetch_add(&rv, argv[i], 0) < 0) ret = 1;
	if (fn_bed && ret == 0) {
		FILE *fp = strcmp(fn_bed, "-") == 0 ? stdin : fopen(fn_bed, "r");
		char *line = 0;
		size_t cap = 0;
		if (fp == 0) { fprintf(stderr, "ERROR: fetch: failed to open '%s'\n", fn_bed); ret = 1; }
		while (ret == 0 && getline(&line, &cap, fp) >= 0) {
			if (line[0] == '\n' || line[0] == '\r' || line[0] == 0 || line[0] == '#') continue;
			if (fetch_add(&rv, line, 1) < 0) ret = 1;
		}
		free(line);
		if (fp && fp != stdin) fclose(fp);
	}
	if (ret == 0 && rv.n == 0) { fprintf(stderr, "ERROR: fetch: no region to fetch\n"); ret = 1; }
	for (k = 0; k < rv.n && ret == 0 && by_row; ++k) { /* --row: the name is a number, and a string has no other strand */
		int64_t a, b;
		char t[32];
		if (rv.a[k].name_len > 20 || rv.a[k].strand < 0) a = -1;
		else {
			memcpy(t, rv.a[k].label, (size_t)rv.a[k].name_len), t[rv.a[k].name_len] = 0;
			if (rb3h_parse_rows(t, &a, &b) < 0 || a != b) a = -1;
		}
		if (a < 0) { fprintf(stderr, "ERROR: fetch: '%s' is no region row:beg-end of --row (a string number, no strand)\n", rv.a[k].label); ret = 1; }
	}
	if (ret) goto done;
	/* 2. the files beside the index, held against the index before anything is asked of a device (as mem -p does) */
	side_read(argv[optind], &sa, &sid);
	if ((sa == 0 && ss < 0) || (sid == 0 && !by_row)) goto no_side;
	if (index_host_read(argv[optind], &ih) < 0) {
		if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: failed to load index '%s'\n", argv[optind]);
		ret = 1;
		goto done;
	}
	m = index_host_sentinels(&ih, &n_sym);
	for (ms = 1; (1LL << ms) < m; ++ms) {}
	if (sa && (sa->m != m || sa->ms != ms || sa->ss > 40 || sa->n_ssa != (n_sym - m + (1LL << sa->ss) - 1) >> sa->ss)) goto no_side;
	if (!by_row && sid->n_seq * 2 != m) goto no_side;
	c = rb3h_verbose;
	if (rb3h_verbose > 2) rb3h_verbose = 2; /* (the command may still refuse its regions with ONE line: the loading says nothing but errors and warnings until they are accepted) */
	h = open_index(device, argv[optind], &ih);
	rb3h_verbose = c;
	if (h == 0) { index_host_free(&ih); ret = 1; goto done; }
	rb3gpu_get_acc(h, acc);
	if ((reg = (rb3gpu_region_t*)malloc((size_t)rv.n * sizeof(*reg))) == 0) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; goto done; }
	if (by_row) {
		for (k = 0; k < rv.n; ++k) reg[k].row = atol(rv.a[k].label), reg[k].beg = rv.a[k].beg, reg[k].end = rv.a[k].end;
	} else { /* 3. names to rows */
		if (index_order(argv[optind]) != RB3GPU_SO_IO) {
			fprintf(stderr, "ERROR: fetch: sequences are numbered in input order; the strings of this index are sorted (build -s / -r): use --row\n");
			ret = 1;
			goto done;
		}
		if (!both_strands(acc)) { ret = 1; goto done; }
		if ((by_name = (int64_t*)malloc((size_t)(sid->n_seq + 1) * 8)) == 0) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; goto done; }
		for (k = 0; k < sid->n_seq; ++k) by_name[k] = k;
		g_fetch_sid = sid;
		qsort(by_name, (size_t)sid->n_seq, 8, fetch_name_cmp);
		for (k = 0; k < rv.n; ++k) {
			const fetch_req_t *q = &rv.a[k];
			const int64_t s = fetch_lookup(sid, by_name, q->label, q->name_len);
			if (s < 0) { fprintf(stderr, "ERROR: fetch: no sequence '%.*s' in the index (region '%s')\n", (int)q->name_len, q->label, q->label); ret = 1; goto done; }
			if (q->end > sid->len[s]) { fprintf(stderr, "ERROR: fetch: region '%s' ends beyond its sequence of %ld symbols\n", q->label, (long)sid->len[s]); ret = 1; goto done; }
			if (q->strand > 0) reg[k].row = 2 * s, reg[k].beg = q->beg, reg[k].end = q->end;
			else reg[k].row = 2 * s + 1, reg[k].beg = sid->len[s] - q->end, reg[k].end = sid->len[s] - q->beg;
		}
	}
	/* 4. the samples: the file's, or made on the device */
	rb3gpu_tune(h, "verbose", rb3h_verbose > 2 ? 2 : rb3h_verbose);
	if (sa) {
		if (sa->m != acc[1] || rb3gpu_ssa_set(h, sa->ss, sa->ms, sa->m, sa->n_ssa, sa->r2i, sa->ssa) != 0) goto no_side;
	} else if ((c = rb3gpu_ssa_keep(h, ss)) != 0) {
		fprintf(stderr, "ERROR: the GPU engine failed to sample the suffix array: %s\n", rb3gpu_strerror(c));
		ret = 1;
		goto done;
	}
	o.q = rv.a;
	c = rb3gpu_fetch(h, rv.n, reg, &bad, fetch_sink, &o, &st);
	if (c == 0 && !o.err && out_flush(&o.out, 1) < 0) o.err = 1;
	if (c == RB3GPU_EINVAL && bad >= 0 && !o.err) { fprintf(stderr, "ERROR: fetch: region '%s' lies outside the index (no such string, or an end beyond it)\n", rv.a[bad].label); ret = 1; }
	else if (c == RB3GPU_EINTERNAL && !o.err) { fprintf(stderr, "ERROR: fetch: the suffix array samples do not belong to this index\n"); ret = 1; }
	else if (c != 0 && !o.err) { fprintf(stderr, "ERROR: the GPU engine failed to fetch the regions: %s\n", rb3gpu_strerror(c)); ret = 1; }
	else if (o.err || fflush(stdout) != 0) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
	if (rb3h_verbose >= 3 && ret == 0)
		fprintf(stderr, "[M::%s::%.3f*%.2f] %lld regions, %lld symbols in %lld slice(s): %lld walkers, %lld regions measured, %lld LF steps, the longest walk of %lld; %.3f ms in the engine, table %.3f ms, plan %.3f ms, walk %.3f ms\n",
				__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)st.n_regions, (long long)st.n_symbols, (long long)st.n_slices, (long long)st.n_walkers, (long long)st.n_measured, (long long)st.n_steps,
				(long long)st.max_walk_steps, st.ms_total, st.ms_table, st.ms_plan, st.ms_walk);
done:
	for (k = 0; k < rv.n; ++k) free(rv.a[k].label);
	free(rv.a); free(reg); free(by_name); free(o.out.s);
	if (h) rb3gpu_destroy(h);
	rb3h_ssa_destroy(sa); rb3h_sid_destroy(sid);
	return ret;
no_side:
	index_host_free(&ih);
	if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: failed to load suffix array samples or sequence names/lengths\n");
	ret = 1;
	goto done;
}

/* hapdiv: the windows of every query (k symbols every w, search.c:384-393) through rb3gpu_hapdiv, batch by batch; the lines of write_hapdiv */
typedef struct { int32_t *r; int64_t n; } hapdiv_out_t;

static int hapdiv_sink(void *ud, int64_t i0, int64_t n, const rb3gpu_hapdiv_rec_t *recs)
{
	hapdiv_out_t *o = (hapdiv_out_t*)ud;
	if (i0 < 0 || i0 + n > o->n) return -1;
	memcpy(o->r + 9 * i0, recs, (size_t)n * 36);
	return 0;
}

static const struct option hapdiv_long_opts[] = {
	{ "gap", required_argument, 0, 403 },
	{ "cov", no_argument, 0, 403 },
	{ "old-mem", no_argument, 0, 403 },
	{ "all-e2e", no_argument, 0, 403 },
	{ "no-ssa", no_argument, 0, 406 },
	{ "seq", no_argument, 0, 406 },
	{ "gpu", required_argument, 0, 301 },
	{ "host-fmd", no_argument, 0, 308 },
	{ 0, 0, 0, 0 }
};

static int main_hapdiv(int argc, char *argv[])
{
	int c, is_line = 0, device = 0, ret = 0, j;
	int64_t k = 101, w = 50, batch_size = 100000000, id = 0, n_win_all = 0, n_ext = 0, n_tier2 = 0, n_slices = 0, n_batches = 0;
	double ms_dp = 0, ms_engine = 0;
	rb3gpu_hapdiv_opt_t ho = { 25, 30, 1, 3, 5, 2, -1 };
	rb3gpu_t *h;
	int64_t acc[7];
	rb3h_buf_t out = {0, 0, 0};
	rb3h_qbatch_t b;
	int64_t *win = 0, m_win = 0;
	hapdiv_out_t o = { 0, 0 };
	_Static_assert(sizeof(rb3gpu_hapdiv_rec_t) == 36, "nine numbers per window");
	optind = 1;
	memset(&b, 0, sizeof(b));
	while ((c = getopt_long(argc, argv, "Ll:c:t:K:MdN:A:B:O:E:C:m:k:uj:ey:a:w:p:bg:", hapdiv_long_opts, 0)) >= 0) {
		if (c == 'L') is_line = 1;
		else if (c == 'a') k = atoi(optarg);
		else if (c == 'w') w = atoi(optarg);
		else if (c == 'N') ho.n_best = atoi(optarg);
		else if (c == 'm') ho.min_sc = atoi(optarg);
		else if (c == 'A') ho.match = atoi(optarg);
		else if (c == 'B') ho.mis = atoi(optarg);
		else if (c == 'O') ho.gap_open = atoi(optarg);
		else if (c == 'E') ho.gap_ext = atoi(optarg);
		else if (c == 'y') ho.e2e_drop = atoi(optarg);
		else if (c == 'K') batch_size = rb3h_parse_num(optarg);
		else if (c == 't' || c == 'C' || c == 'M') {} /* threads, the rank cache, the mmap loader: nothing to size here, and none changes an answer */
		else if (c == 'e' || c == 'k' || c == 'b' || c == 'u' || c == 'j' || c == 'l' || c == 'c' || c == 406) {} /* hapdiv is end to end with end_len 1 whatever these say (search.c:498-505) */
		else if (c == 301) device = atoi(optarg);
		else if (c == 308) g_host_fmd = 1;
		else if (c == '?') return 1;
		else { fprintf(stderr, "ERROR: option not supported by hapdiv (it belongs to sw or mem)\n"); return 1; }
	}
	if (argc - optind < 2) {
		fprintf(stdout, "Usage: ropebwt3-amd hapdiv [options] <idx.fmr> <seq.fa> [...]\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  -a INT      annotate sliding INT-mers [%ld]\n", (long)k);
		fprintf(stderr, "  -w INT      k-mer step size for annotation [%ld]\n", (long)w);
		fprintf(stderr, "  -N INT      keep up to INT hits per DAG node [%d]\n", ho.n_best);
		fprintf(stderr, "  -A INT      match score [%d]\n", ho.match);
		fprintf(stderr, "  -B INT      mismatch penalty [%d]\n", ho.mis);
		fprintf(stderr, "  -O INT      gap open penalty [%d]\n", ho.gap_open);
		fprintf(stderr, "  -E INT      gap extension penalty; a k-long gap costs O+k*E [%d]\n", ho.gap_ext);
		fprintf(stderr, "  -m INT      min alignment score [%d]\n", ho.min_sc);
		fprintf(stderr, "  -y INT      report alignments within INT of the best score (-1: all) [%d]\n", ho.e2e_drop);
		fprintf(stderr, "  -L          one sequence per line in the input\n");
		fprintf(stderr, "  -K NUM      query batch size [100m]\n");
		return 0;
	}
	if (k < 1) { fprintf(stderr, "ERROR: the k-mer length (-a) must be at least 1\n"); return 1; }
	if (w < 1) { fprintf(stderr, "ERROR: the step size (-w) must be at least 1\n"); return 1; }
	if (ho.n_best < 1) { fprintf(stderr, "ERROR: the number of hits kept per row (-N) must be at least 1\n"); return 1; }
	if (k > 0x7ffffffeLL || (k + 1) * (int64_t)ho.n_best >= 0xFFFFFFFFLL || ho.n_best >= (1 << 24)) { fprintf(stderr, "ERROR: -a times -N is too large\n"); return 1; }
	if ((h = open_index(device, argv[optind], 0)) == 0) return 1;
	rb3gpu_get_acc(h, acc);
	if (!both_strands(acc)) {
		rb3gpu_destroy(h);
		return 1;
	}
	for (j = optind + 1; j < argc && ret == 0; ++j) {
		rb3h_seqio_t *fp = rb3h_seq_open(argv[j], is_line);
		if (fp == 0) {
			if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: failed to load the sequence file '%s'\n", argv[j]);
			ret = 1;
			break;
		}
		for (b.eof = 0; !b.eof && ret == 0;) { /* a batch: whole records until their symbols reach -K (search.c:366-378) */
			const int64_t n_q = rb3h_qbatch_read(fp, &b, batch_size, 0x7fffffffLL, INT64_MAX), *off = b.off, *name_off = b.name_off;
			int64_t n_win = 0, q, x;
			if (n_q < 0) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; }
			if (rb3h_seq_error(fp) && rb3h_verbose >= 1 && b.eof) fprintf(stderr, "ERROR: FASTX parsing error (code %d)\n", rb3h_seq_error(fp));
			if (n_q <= 0) continue;
			for (q = 0; q < n_q; ++q) {
				const int64_t len = off[q + 1] - off[q];
				n_win += len < k ? 0 : (len - k) / w + 1;
			}
			if (n_win > m_win) {
				m_win = n_win + (n_win >> 1) + 64;
				win = (int64_t*)realloc(win, (size_t)m_win * 8), o.r = (int32_t*)realloc(o.r, (size_t)m_win * 36);
				if (win == 0 || o.r == 0) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; break; }
			}
			for (q = 0, n_win = 0; q < n_q; ++q)
				for (x = 0; x + k <= off[q + 1] - off[q]; x += w) win[n_win++] = off[q] + x;
			o.n = n_win;
			if (n_win > 0) {
				rb3gpu_hapdiv_stats_t st;
				int64_t at = 0;
				const int r = rb3gpu_hapdiv(h, n_win, win, b.sym.s, (int32_t)k, &ho, hapdiv_sink, &o, &st);
				if (r != 0) { fprintf(stderr, "ERROR: the GPU engine failed to align the windows: %s\n", rb3gpu_strerror(r)); ret = 1; break; }
				for (q = 0; q < n_q && ret == 0; ++q) {
					const int64_t len = off[q + 1] - off[q], nw = len < k ? 0 : (len - k) / w + 1;
					if (nw > 0 && rb3h_hapdiv_format(&out, name_off[q] >= 0 ? (const char*)b.names.s + name_off[q] : 0, id + q, k, w, nw, o.r + 9 * at) < 0) ret = 1;
					at += nw;
					if (out_flush(&out, q == n_q - 1) < 0) ret = 1;
				}
				if (ret) { fprintf(stderr, "ERROR: failed to write the output\n"); break; }
				n_win_all += n_win, n_ext += st.n_ext, n_tier2 += st.n_tier2, n_slices += st.n_slices, ms_dp += st.ms_dp, ms_engine += st.ms_total;
			}
			id += n_q, ++n_batches;
			if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] processed %lld sequences\n", __func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)n_q);
		}
		rb3h_seq_close(fp);
	}
	if (fflush(stdout) != 0 && ret == 0) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
	if (rb3h_verbose >= 3 && ret == 0)
		fprintf(stderr, "[M::%s::%.3f*%.2f] %lld queries in %lld batch(es): %lld windows in %lld slice(s), %lld extensions, %lld windows with a table in global memory; %.3f ms in the engine, the DP kernel %.3f ms\n",
				__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)id, (long long)n_batches, (long long)n_win_all, (long long)n_slices, (long long)n_ext, (long long)n_tier2, ms_engine, ms_dp);
	free(out.s); free(o.r); free(win);
	rb3h_qbatch_free(&b);
	rb3gpu_destroy(h);
	return ret;
}

/* sw: the end-to-end alignments of every query (the reference's main_search for `sw` with -e, --all-e2e or -g, search.c:443-582) through rb3gpu_sw_e2e, batch by
 * batch; the PAF of write_paf or the blocks of write_all_hits (swfmt.c).  <index>.ssa and <index>.len.gz are loaded when they are there and belong to the index
 * (rb3_fmi_load_all, fm-index.c:606-640) unless --no-ssa, --all-e2e or -g says otherwise; with the first a hit gets positions, with the second they get names.
 * --local: the reference's default mode, the one best local hit of every query over the query's DAWG (host/dawg.c, rb3gpu_sw_local), written by the same write_paf
 * with the hit's place on the query.  It is opt-in: without --local and without -e the command is refused as before.
 * --prefilter: with -j above the end length, the reference's MEM pre-filter (rb3_sw, bwa-sw.c:536-539): rb3gpu_seed_present runs first on every batch, only the
 * queries with a seed of -j symbols go to the alignment, as a compacted batch, and the others are written as queries without a hit.  Opt-in as well.
 * Differences, each a refusal with exit status 1 and nothing on stdout: no mode given (neither --local nor -e), --local with -e, --all-e2e or -g, -j above the end length without --prefilter,
 * -N or -k below 1, and the options of `mem` and `hapdiv`. */
typedef struct {
	int64_t n, *off, *map, m_q; /* the compacted batch: n queries, query i is the batch's query map[i] */
	rb3h_buf_t sym;
	uint8_t *present;
} sw_seed_t;

/* the queries of the batch that hold a seed of min_len symbols, as a batch of their own; 1: out of memory, < 0: the engine's error */
static int sw_seed_filter(rb3gpu_t *h, int64_t n_q, const int64_t *off, const uint8_t *sym, int min_len, sw_seed_t *f, rb3gpu_seed_stats_t *st)
{
	int64_t q, total = 0;
	int r;
	if (n_q + 1 > f->m_q) {
		f->m_q = n_q + (n_q >> 1) + 1024;
		f->off = (int64_t*)realloc(f->off, (size_t)f->m_q * 8), f->map = (int64_t*)realloc(f->map, (size_t)f->m_q * 8), f->present = (uint8_t*)realloc(f->present, (size_t)f->m_q);
		if (f->off == 0 || f->map == 0 || f->present == 0) return 1;
	}
	if ((r = rb3gpu_seed_present(h, n_q, off, sym, min_len, 0, f->present, st)) != 0) return r;
	for (q = 0; q < n_q; ++q) if (f->present[q]) total += off[q + 1] - off[q];
	if (f->sym.m < total + 1) {
		f->sym.m = total + 1, f->sym.s = (uint8_t*)realloc(f->sym.s, (size_t)f->sym.m);
		if (f->sym.s == 0) return 1;
	}
	for (q = 0, f->n = 0, f->off[0] = 0; q < n_q; ++q)
		if (f->present[q]) {
			memcpy(f->sym.s + f->off[f->n], sym + off[q], (size_t)(off[q + 1] - off[q]));
			f->map[f->n] = q, f->off[f->n + 1] = f->off[f->n] + (off[q + 1] - off[q]), ++f->n;
		}
	f->sym.l = total;
	return 0;
}

/* the hits of a compacted batch, as counted per query by sw_sink, spread back over the n_q queries of the whole batch (the hits themselves stay in order) */
static void sw_seed_spread(const sw_seed_t *f, int64_t n_q, int32_t *n_hit, int32_t *hit_node)
{
	int64_t i, q;
	for (i = f->n - 1, q = n_q - 1; q >= 0; --q) { /* map[i] >= i: from the back, nothing is overwritten before it is read */
		if (i >= 0 && f->map[i] == q) {
			n_hit[q] = n_hit[i];
			if (hit_node) hit_node[q] = hit_node[i];
			--i;
		} else {
			n_hit[q] = 0;
			if (hit_node) hit_node[q] = 0;
		}
	}
}

typedef struct {
	int32_t *n_hit; int64_t m_q;
	rb3h_sw_hit_t *hits; int64_t n_hits, m_hits;
	uint8_t *steps; int64_t n_steps, m_steps;
	rb3h_pos_t *pos; int64_t n_pos, m_pos;
	int err;
} sw_out_t;

static int sw_sink(void *ud, int64_t q0, int64_t nq, const int32_t *n_hit, const rb3gpu_sw_hit_t *hits, const uint8_t *steps, const rb3gpu_pos_t *pos)
{
	sw_out_t *o = (sw_out_t*)ud;
	int64_t i, nh = 0, ns = 0, np = 0;
	if (q0 < 0 || q0 + nq > o->m_q) return o->err = 2, -1;
	for (i = 0; i < nq; ++i) o->n_hit[q0 + i] = n_hit[i], nh += n_hit[i];
	for (i = 0; i < nh; ++i) {
		if (hits[i].step_off + hits[i].n_steps > ns) ns = hits[i].step_off + hits[i].n_steps;
		if (hits[i].n_pos > 0 && hits[i].pos_off + hits[i].n_pos > np) np = hits[i].pos_off + hits[i].n_pos;
	}
	if (o->hits == 0 || o->n_hits + nh > o->m_hits) {
		o->m_hits = (o->n_hits + nh) * 2 + 256;
		o->hits = (rb3h_sw_hit_t*)realloc(o->hits, (size_t)o->m_hits * sizeof(*o->hits));
	}
	if (o->steps == 0 || o->n_steps + ns > o->m_steps) o->m_steps = (o->n_steps + ns) * 2 + 4096, o->steps = (uint8_t*)realloc(o->steps, (size_t)o->m_steps);
	if (o->pos == 0 || o->n_pos + np > o->m_pos) o->m_pos = (o->n_pos + np) * 2 + 256, o->pos = (rb3h_pos_t*)realloc(o->pos, (size_t)o->m_pos * sizeof(*o->pos));
	if (o->hits == 0 || o->steps == 0 || o->pos == 0) return o->err = 1, -1;
	if (ns > 0) memcpy(o->steps + o->n_steps, steps, (size_t)ns);
	if (np > 0) memcpy(o->pos + o->n_pos, pos, (size_t)np * sizeof(*pos));
	for (i = 0; i < nh; ++i) {
		rb3h_sw_hit_t *d = o->hits + o->n_hits + i;
		memcpy(d, hits + i, sizeof(*d));
		d->step_off += o->n_steps, d->pos_off += o->n_pos;
	}
	o->n_hits += nh, o->n_steps += ns, o->n_pos += np;
	return 0;
}

static const struct option sw_long_opts[] = {
	{ "gap", required_argument, 0, 403 },
	{ "cov", no_argument, 0, 403 },
	{ "old-mem", no_argument, 0, 403 },
	{ "no-ssa", no_argument, 0, 401 },
	{ "seq", no_argument, 0, 402 },
	{ "all-e2e", no_argument, 0, 406 },
	{ "local", no_argument, 0, 407 },
	{ "prefilter", no_argument, 0, 408 },
	{ "gpu", required_argument, 0, 301 },
	{ "host-fmd", no_argument, 0, 308 },
	{ 0, 0, 0, 0 }
};

static int main_sw(int argc, char *argv[])
{
	int c, is_line = 0, device = 0, ret = 0, j, e2e = 0, local = 0, no_ssa = 0, write_all = 0, both = 0, unmapped = 0, with_rs = 0, max_pos = 0, min_mem_len = 0, prefilter = 0, seeded;
	int64_t batch_size = 100000000, id = 0, max_all_out = 0, n_ext = 0, n_hits = 0, n_tier2 = 0, n_slices = 0, n_batches = 0, n_filtered = 0, n_seed_walkers = 0, n_seed_steps = 0;
	double ms_dp = 0, ms_bt = 0, ms_engine = 0, ms_locate = 0, ms_dawg = 0, ms_seed = 0;
	int64_t n_nodes = 0, n_edges = 0, *node_off = 0, m_node_off = 0, m_hit = 0, max_len;
	int32_t *hit_node = 0;
	rb3gpu_sw_opt_t so = { 25, 30, 1, 3, 5, 2, -1, 11, 0 };
	rb3gpu_t *h;
	rb3h_ssa_t *sa = 0;
	rb3h_sid_t *sid = 0;
	int have_ssa = 0;
	int64_t acc[7];
	rb3h_buf_t rev = {0, 0, 0}, out = {0, 0, 0};
	rb3h_qbatch_t b;
	sw_out_t o[2];
	sw_seed_t sf[2];
	_Static_assert(sizeof(rb3h_sw_hit_t) == sizeof(rb3gpu_sw_hit_t), "one hit layout on both sides");
	_Static_assert(sizeof(rb3h_pos_t) == sizeof(rb3gpu_pos_t), "one position layout on both sides");
	memset(o, 0, sizeof(o));
	memset(&b, 0, sizeof(b));
	memset(sf, 0, sizeof(sf));
	optind = 1;
	while ((c = getopt_long(argc, argv, "Ll:c:t:K:MdN:A:B:O:E:C:m:k:uj:ey:a:w:p:bg:", sw_long_opts, 0)) >= 0) { /* the order of -e, -k, -g matters as in search.c:452-492 */
		if (c == 'L') is_line = 1;
		else if (c == 'g') max_all_out = atol(optarg), write_all = 1, e2e = 1, so.end_len = 1, no_ssa = 1;
		else if (c == 406) write_all = 1, e2e = 1, so.end_len = 1, no_ssa = 1;
		else if (c == 407) local = 1;
		else if (c == 408) prefilter = 1;
		else if (c == 'e') e2e = 1, so.end_len = 1;
		else if (c == 'k') so.end_len = atoi(optarg);
		else if (c == 'j') min_mem_len = atoi(optarg);
		else if (c == 'N') so.n_best = atoi(optarg);
		else if (c == 'm') so.min_sc = atoi(optarg);
		else if (c == 'A') so.match = atoi(optarg);
		else if (c == 'B') so.mis = atoi(optarg);
		else if (c == 'O') so.gap_open = atoi(optarg);
		else if (c == 'E') so.gap_ext = atoi(optarg);
		else if (c == 'y') so.e2e_drop = atoi(optarg);
		else if (c == 'p') max_pos = atoi(optarg);
		else if (c == 'K') batch_size = rb3h_parse_num(optarg);
		else if (c == 'u') unmapped = 1;
		else if (c == 'b') both = 1;
		else if (c == 401) no_ssa = 1;
		else if (c == 402) with_rs = 1;
		else if (c == 't' || c == 'C' || c == 'M') {} /* threads, the rank cache, the mmap loader: nothing to size here, and none changes an answer */
		else if (c == 301) device = atoi(optarg);
		else if (c == 308) g_host_fmd = 1;
		else if (c == '?') return 1;
		else { fprintf(stderr, "ERROR: option not supported by sw (it belongs to mem or hapdiv)\n"); return 1; }
	}
	if (argc - optind < 2) {
		fprintf(stdout, "Usage: ropebwt3-amd sw [options] <idx.fmr> <seq.fa> [...]\n");
		fprintf(stderr, "Options:\n");
		fprintf(stderr, "  --local     local mode: the best local hit of every query (BWA-SW over the query's DAWG)\n");
		fprintf(stderr, "  -e          end-to-end mode (forcing -k to 1); one of --local and -e is required\n");
		fprintf(stderr, "  -N INT      keep up to INT hits per row [%d]\n", so.n_best);
		fprintf(stderr, "  -m INT      min alignment score [%d]\n", so.min_sc);
		fprintf(stderr, "  -A INT      match score [%d]\n", so.match);
		fprintf(stderr, "  -B INT      mismatch penalty [%d]\n", so.mis);
		fprintf(stderr, "  -O INT      gap open penalty [%d]\n", so.gap_open);
		fprintf(stderr, "  -E INT      gap extension penalty; a k-long gap costs O+k*E [%d]\n", so.gap_ext);
		fprintf(stderr, "  -y INT      ignore secondary hits scored INT lower than the best [%d]\n", so.e2e_drop);
		fprintf(stderr, "  -k INT      require INT-mer match at the end of alignment [%d]\n", so.end_len);
		fprintf(stderr, "  -j INT      min MEM length to initiate alignment (with --prefilter) [%d]\n", min_mem_len);
		fprintf(stderr, "  --prefilter with -j above the end length: align only the queries that hold an exact match of -j symbols\n");
		fprintf(stderr, "  -b          align both strands (effective with --all-e2e)\n");
		fprintf(stderr, "  -u          write unmapped queries to PAF\n");
		fprintf(stderr, "  --seq       write reference sequence to the rs tag\n");
		fprintf(stderr, "  --all-e2e   write all end-to-end hits in a compact format (forcing -e)\n");
		fprintf(stderr, "  -g INT      cap the number of --all-e2e output to INT (forcing --all-e2e)\n");
		fprintf(stderr, "  --no-ssa    ignore the sampled suffix array\n");
		fprintf(stderr, "  -p INT      output up to INT positions [%d]\n", max_pos);
		fprintf(stderr, "  -L          one sequence per line in the input\n");
		fprintf(stderr, "  -K NUM      query batch size [100m]\n");
		return 0;
	}
	if (local && e2e) { fprintf(stderr, "ERROR: --local does not go with -e, --all-e2e or -g\n"); return 1; }
	if (!e2e && !local) { fprintf(stderr, "ERROR: local mode is not implemented: use -e\n"); return 1; }
	if (so.n_best < 1) { fprintf(stderr, "ERROR: the number of hits kept per row (-N) must be at least 1\n"); return 1; }
	if (so.end_len < 1) { fprintf(stderr, "ERROR: the end length (-k) must be at least 1\n"); return 1; }
	if (so.n_best >= (1 << 24)) { fprintf(stderr, "ERROR: -N is too large\n"); return 1; }
	seeded = min_mem_len > 0 && min_mem_len > so.end_len; /* bwa-sw.c:536 */
	if (seeded && !prefilter) { fprintf(stderr, "ERROR: -j above the end length asks for the MEM pre-filter: add --prefilter\n"); return 1; }
	if ((h = open_index(device, argv[optind], 0)) == 0) return 1;
	rb3gpu_get_acc(h, acc);
	if (!no_ssa) { /* the two files beside the index, each only if it is there and belongs to this index */
		side_read(argv[optind], &sa, &sid);
		if (sa && (sa->m != acc[1] || rb3gpu_ssa_set(h, sa->ss, sa->ms, sa->m, sa->n_ssa, sa->r2i, sa->ssa) != 0)) {
			if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: number of sequences do not match between BWT and sampled suffix array\n");
		} else if (sa) have_ssa = 1;
		rb3h_ssa_destroy(sa), sa = 0; /* (it lives on the device from here on) */
		if (sid && sid->n_seq * 2 != acc[1]) {
			if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: number of sequences do not match between BWT and the sequence list\n");
			rb3h_sid_destroy(sid), sid = 0;
		}
	}
	if (max_pos > 0 && (!have_ssa || sid == 0)) { /* search.c:555-559 */
		if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: failed to load suffix array samples or sequence names/lengths\n");
		rb3gpu_destroy(h);
		rb3h_sid_destroy(sid);
		return 1;
	}
	if (!both_strands(acc)) {
		rb3gpu_destroy(h);
		rb3h_sid_destroy(sid);
		return 1;
	}
	so.max_pos = have_ssa ? max_pos : -1;
	/* the longest query: a cell of the backtrack matrix is named by row * n_best + column in 32 bits (two rows a symbol with --local), so with c = n_best * (local ? 2 : 1),
	 * 1 <= c < 2^25, a query of l symbols is refused when l > 0x7ffffffe or (l + 1) * c >= 0xFFFFFFFF.  (l + 1) * c < 0xFFFFFFFF is (l + 1) * c <= 0xFFFFFFFE,
	 * which for integers is l + 1 <= 0xFFFFFFFE / c rounded down: the largest l that passes is the smaller of 0x7ffffffe and 0xFFFFFFFE / c - 1 (127 at least) */
	max_len = 0xFFFFFFFELL / (so.n_best * (local ? 2 : 1)) - 1;
	if (max_len > 0x7ffffffeLL) max_len = 0x7ffffffeLL;
	if (write_all) fputs("CC\tQS  queryName  queryLen  numHap\nCC\tQH  refCount   score     editDist   cs   strand   nOut   totAln\nCC\n", stdout);
	for (j = optind + 1; j < argc && ret == 0; ++j) {
		rb3h_seqio_t *fp = rb3h_seq_open(argv[j], is_line);
		if (fp == 0) {
			if (rb3h_verbose >= 1) fprintf(stderr, "ERROR: failed to load the sequence file '%s'\n", argv[j]);
			break; /* (the reference stops here and exits 0, search.c:570-576) */
		}
		for (b.eof = 0; !b.eof && ret == 0;) { /* a batch: whole records until their symbols reach -K (search.c:366-378) */
			const int64_t n_q = rb3h_qbatch_read(fp, &b, batch_size, 0x7fffffffLL, max_len), *off = b.off, *name_off = b.name_off;
			const rb3h_buf_t sym = b.sym, names = b.names;
			int64_t q, at[2] = { 0, 0 };
			int pass;
			if (n_q > m_hit) {
				m_hit = n_q + (n_q >> 1) + 1024;
				o[0].n_hit = (int32_t*)realloc(o[0].n_hit, (size_t)m_hit * 4), o[1].n_hit = (int32_t*)realloc(o[1].n_hit, (size_t)m_hit * 4);
			}
			if (n_q == -1 || (n_q > 0 && (o[0].n_hit == 0 || o[1].n_hit == 0))) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; }
			if (n_q == -2) { fprintf(stderr, "ERROR: a query times -N is too large\n"); ret = 1; }
			if (rb3h_seq_error(fp) && rb3h_verbose >= 1 && b.eof) fprintf(stderr, "ERROR: FASTX parsing error (code %d)\n", rb3h_seq_error(fp));
			if (n_q <= 0 || ret != 0) continue;
			if (seeded) { /* only the queries with a seed are aligned (bwa-sw.c:536-539): the batch without the others */
				rb3gpu_seed_stats_t ss;
				const int r = sw_seed_filter(h, n_q, off, sym.s, min_mem_len, &sf[0], &ss);
				if (r > 0) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; continue; }
				if (r < 0) { fprintf(stderr, "ERROR: the GPU engine failed to look for seeds: %s\n", rb3gpu_strerror(r)); ret = 1; continue; }
				n_filtered += n_q - ss.n_present, n_seed_walkers += ss.n_walkers, n_seed_steps += ss.n_steps, ms_seed += ss.ms_walk, ms_engine += ss.ms_total;
			}
			if (local) { /* the graphs of the batch on the host, the nodes as rows on the device, one hit per query at most with its place on the query */
				rb3h_dawg_t dg;
				rb3gpu_swl_stats_t st;
				rb3gpu_locate_stats_t ls;
				const double t_dg = rb3h_realtime();
				const int64_t a_n = seeded ? sf[0].n : n_q, *a_off = seeded ? sf[0].off : off; /* what is aligned: the graphs are built for these queries only */
				const uint8_t *a_sym = seeded ? sf[0].sym.s : sym.s;
				int64_t a; /* the query's number among the aligned ones */
				int r;
				if (n_q + 1 > m_node_off) {
					m_node_off = n_q + 1;
					node_off = (int64_t*)realloc(node_off, (size_t)m_node_off * 8), hit_node = (int32_t*)realloc(hit_node, (size_t)m_node_off * 4);
				}
				if (node_off == 0 || hit_node == 0 || (r = rb3h_dawg_batch(a_n, a_off, a_sym, &dg, node_off)) < 0) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; continue; }
				ms_dawg += (rb3h_realtime() - t_dg) * 1e3;
				o[0].m_q = n_q, o[0].n_hits = o[0].n_steps = o[0].n_pos = 0, o[0].err = 0;
				r = rb3gpu_sw_local(h, a_n, a_off, a_sym, node_off, dg.sym, dg.pre_off, dg.pre, &so, sw_sink, &o[0], hit_node, &st, &ls);
				if (r != 0 && o[0].err == 1) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; }
				else if (r != 0) { fprintf(stderr, "ERROR: the GPU engine failed to align the queries: %s\n", rb3gpu_strerror(r)); ret = 1; }
				n_ext += st.sw.n_ext, n_hits += st.sw.n_hits, n_tier2 += st.sw.n_tier2, n_slices += st.sw.n_slices, ms_dp += st.sw.ms_dp, ms_bt += st.sw.ms_backtrack, ms_engine += st.sw.ms_total;
				ms_locate += ls.ms_locate, n_nodes += st.n_nodes, n_edges += st.n_edges;
				if (seeded && ret == 0) sw_seed_spread(&sf[0], n_q, o[0].n_hit, hit_node);
				for (q = 0, a = 0; q < n_q && ret == 0; ++q) {
					const char *nm = name_off[q] >= 0 ? (const char*)names.s + name_off[q] : 0;
					const int64_t g = o[0].n_hit[q] > 0 ? node_off[a] + hit_node[q] : 0;
					if (o[0].n_hit[q] > 1 || (o[0].n_hit[q] == 1 && (hit_node[q] < 0 || g >= node_off[a + 1]))) r = -3;
					else r = rb3h_sw_format_paf_at(&out, nm, id + q, off[q + 1] - off[q], sym.s + off[q], o[0].n_hit[q], o[0].hits + at[0], o[0].steps, o[0].pos, sid, unmapped, with_rs,
							dg.qoff0 + g, dg.n_qoff + g);
					at[0] += o[0].n_hit[q];
					if (!seeded || sf[0].present[q]) ++a;
					if (r == -2) { fprintf(stderr, "ERROR: a position names a sequence that the name list does not have\n"); ret = 1; break; }
					if (r == -3) { fprintf(stderr, "ERROR: the GPU engine returned a hit that is not on the query\n"); ret = 1; break; }
					if (r < 0) ret = 1;
					if (out_flush(&out, q == n_q - 1) < 0) ret = 1;
					if (ret) fprintf(stderr, "ERROR: failed to write the output\n");
				}
				rb3h_dawg_free(&dg);
				id += n_q, ++n_batches;
				if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] processed %lld sequences\n", __func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)n_q);
				continue;
			}
			for (pass = 0; pass < (write_all && both ? 2 : 1) && ret == 0; ++pass) { /* the second pass: every query reverse-complemented in place (search.c:94-98) */
				rb3gpu_sw_stats_t st;
				rb3gpu_locate_stats_t ls;
				const uint8_t *codes = sym.s;
				int r;
				if (pass == 1) {
					if (rev.m < sym.l + 1) rev.m = sym.l + 1, rev.s = (uint8_t*)realloc(rev.s, (size_t)rev.m);
					if (rev.s == 0) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; break; }
					memcpy(rev.s, sym.s, (size_t)sym.l);
					for (q = 0; q < n_q; ++q) rb3h_revcomp6(off[q + 1] - off[q], rev.s + off[q]);
					codes = rev.s;
					if (seeded) { /* the reference's second rb3_sw call sees the reverse-complemented query (search.c:94-98) */
						rb3gpu_seed_stats_t ss;
						r = sw_seed_filter(h, n_q, off, codes, min_mem_len, &sf[1], &ss);
						if (r > 0) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; break; }
						if (r < 0) { fprintf(stderr, "ERROR: the GPU engine failed to look for seeds: %s\n", rb3gpu_strerror(r)); ret = 1; break; }
						n_filtered += n_q - ss.n_present, n_seed_walkers += ss.n_walkers, n_seed_steps += ss.n_steps, ms_seed += ss.ms_walk, ms_engine += ss.ms_total;
					}
				}
				o[pass].m_q = n_q, o[pass].n_hits = o[pass].n_steps = o[pass].n_pos = 0, o[pass].err = 0;
				if (seeded) r = rb3gpu_sw_e2e(h, sf[pass].n, sf[pass].off, sf[pass].sym.s, &so, sw_sink, &o[pass], &st, &ls);
				else r = rb3gpu_sw_e2e(h, n_q, off, codes, &so, sw_sink, &o[pass], &st, &ls);
				if (r != 0 && o[pass].err == 1) { fprintf(stderr, "ERROR: out of memory\n"); ret = 1; }
				else if (r != 0) { fprintf(stderr, "ERROR: the GPU engine failed to align the queries: %s\n", rb3gpu_strerror(r)); ret = 1; }
				n_ext += st.n_ext, n_hits += st.n_hits, n_tier2 += st.n_tier2, n_slices += st.n_slices, ms_dp += st.ms_dp, ms_bt += st.ms_backtrack, ms_engine += st.ms_total, ms_locate += ls.ms_locate;
				if (seeded && ret == 0) sw_seed_spread(&sf[pass], n_q, o[pass].n_hit, 0);
			}
			for (q = 0; q < n_q && ret == 0; ++q) {
				const char *nm = name_off[q] >= 0 ? (const char*)names.s + name_off[q] : 0;
				const int64_t len = off[q + 1] - off[q];
				int r;
				if (write_all) {
					r = rb3h_sw_format_all(&out, nm, id + q, len, sym.s + off[q], o[0].n_hit[q], o[0].hits + at[0], o[0].steps, '+', max_all_out);
					if (r == 0 && both) r = rb3h_sw_format_all(&out, nm, id + q, len, rev.s + off[q], o[1].n_hit[q], o[1].hits + at[1], o[1].steps, '-', max_all_out), at[1] += o[1].n_hit[q];
				} else r = rb3h_sw_format_paf(&out, nm, id + q, len, sym.s + off[q], o[0].n_hit[q], o[0].hits + at[0], o[0].steps, o[0].pos, sid, unmapped, with_rs);
				at[0] += o[0].n_hit[q];
				if (r == -2) { fprintf(stderr, "ERROR: a position names a sequence that the name list does not have\n"); ret = 1; break; }
				if (r < 0) ret = 1;
				if (out_flush(&out, q == n_q - 1) < 0) ret = 1;
				if (ret) fprintf(stderr, "ERROR: failed to write the output\n");
			}
			id += n_q, ++n_batches;
			if (rb3h_verbose >= 3) fprintf(stderr, "[M::%s::%.3f*%.2f] processed %lld sequences\n", __func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)n_q);
		}
		rb3h_seq_close(fp);
	}
	if (fflush(stdout) != 0 && ret == 0) { fprintf(stderr, "ERROR: failed to write the output\n"); ret = 1; }
	if (rb3h_verbose >= 3 && ret == 0) {
		char pre[256] = "";
		if (seeded) snprintf(pre, sizeof(pre), "; the pre-filter: %lld queries without a seed of %d symbols were not aligned; %lld walkers, %lld extension steps, the seed kernel %.3f ms",
				(long long)n_filtered, min_mem_len, (long long)n_seed_walkers, (long long)n_seed_steps, ms_seed);
		fprintf(stderr, "[M::%s::%.3f*%.2f] %lld queries in %lld batch(es): %lld hits in %lld slice(s), %lld extensions, %lld queries with a table in global memory; %.3f ms in the engine, the DP kernel %.3f ms, the backtrack %.3f ms, the locate kernels %.3f ms%s\n",
				__func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)id, (long long)n_batches, (long long)n_hits, (long long)n_slices, (long long)n_ext, (long long)n_tier2, ms_engine, ms_dp, ms_bt, ms_locate, pre);
	}
	if (rb3h_verbose >= 3 && ret == 0 && local)
		fprintf(stderr, "[M::%s::%.3f*%.2f] the graphs: %lld nodes, %lld edges, %.3f ms on the host\n", __func__, rb3h_realtime(), rb3h_percent_cpu(), (long long)n_nodes, (long long)n_edges, ms_dawg);
	for (j = 0; j < 2; ++j) { free(o[j].n_hit); free(o[j].hits); free(o[j].steps); free(o[j].pos); free(sf[j].off); free(sf[j].map); free(sf[j].present); free(sf[j].sym.s); }
	free(out.s); free(rev.s); free(node_off); free(hit_node);
	rb3h_qbatch_free(&b);
	rb3gpu_destroy(h);
	rb3h_sid_destroy(sid);
	return ret;
}

/* recode: decode an FMD/FMR file on the host and write it back as plain text (default), FMD (-d)
 * or FMR (-b).  Host-only utility; also the CPU-side test bench of the two codecs. */
typedef struct { int64_t cnt[6]; runvec_t rv; } recode_t;

static int sink_recode(void *data, int c, int64_t l)
{
	recode_t *r = (recode_t*)data;
	r->cnt[c] += l;
	return sink_runvec(&r->rv, c, l);
}

static const struct option recode_opts[] = {
	{ "bre-run-bytes", required_argument, 0, 311 },
	{ 0, 0, 0, 0 }
};

static int main_recode(int argc, char *argv[])
{
	int c, fmt = FMT_PLAIN, ret = 0, block_len = 0, max_nodes = 0;
	int64_t i;
	recode_t rc;
	optind = 1;
	while ((c = getopt_long(argc, argv, "dbeo:l:n:", recode_opts, 0)) >= 0) {
		if (c == 'd') fmt = FMT_FMD;
		else if (c == 'b') fmt = FMT_FMR;
		else if (c == 'e') fmt = FMT_BRE;
		else if (c == 311) g_bre_run_bytes = atoi(optarg);
		else if (c == 'l') block_len = atoi(optarg);
		else if (c == 'n') max_nodes = atoi(optarg);
		else if (c == 'o' && freopen(optarg, "wb", stdout) == 0) return 1;
	}
	if (argc - optind < 1 || g_bre_run_bytes < 1 || g_bre_run_bytes > 8) { fprintf(stderr, "Usage: ropebwt3-amd recode [-d|-b|-e [--bre-run-bytes 1..8]] [-o out] <in.fmd|in.fmr|in.bre>\n"); return 1; }
	memset(&rc, 0, sizeof(rc));
	if (rb3h_index_read_runs(argv[optind], sink_recode, &rc) < 0) { fprintf(stderr, "ERROR: failed to read '%s'\n", argv[optind]); free(rc.rv.a); return 1; }
	if (fmt == FMT_FMD) {
		rb3h_fmdw_t *w = rb3h_fmdw_init();
		for (i = 0; i < rc.rv.n && ret == 0; ++i) ret = rb3h_fmdw_enc(w, (int64_t)(rc.rv.a[i] >> 3), (int)(rc.rv.a[i] & 7));
		if (ret == 0) ret = rb3h_fmdw_finish(w);
		if (ret == 0) ret = rb3h_fmdw_dump(w, stdout);
		rb3h_fmdw_destroy(w);
	} else if (fmt == FMT_FMR) {
		int64_t acc[7];
		rb3h_fmrw_t *w;
		for (acc[0] = 0, c = 0; c < 6; ++c) acc[c + 1] = acc[c] + rc.cnt[c];
		w = rb3h_fmrw_init(acc, max_nodes, block_len);
		for (i = 0; i < rc.rv.n && ret == 0; ++i) ret = rb3h_fmrw_enc(w, (int64_t)(rc.rv.a[i] >> 3), (int)(rc.rv.a[i] & 7));
		if (ret == 0) ret = rb3h_fmrw_dump(w, stdout);
		rb3h_fmrw_destroy(w);
	} else if (fmt == FMT_BRE) {
		rb3h_brew_t *w = rb3h_brew_init(stdout, g_bre_run_bytes);
		if (w == 0) ret = -1;
		for (i = 0; i < rc.rv.n && ret == 0; ++i) ret = rb3h_brew_enc(w, (int64_t)(rc.rv.a[i] >> 3), (int)(rc.rv.a[i] & 7));
		if (ret == 0) ret = rb3h_brew_finish(w);
		rb3h_brew_destroy(w);
	} else {
		for (i = 0; i < rc.rv.n && ret == 0; ++i) ret = sink_plain(stdout, (int)(rc.rv.a[i] & 7), (int64_t)(rc.rv.a[i] >> 3));
		fputc('\n', stdout);
	}
	free(rc.rv.a);
	return ret == 0 ? 0 : 1;
}

/* plain2fmd (the reference's main.c:299-331): every byte of the input is one BWT symbol, '\n' and '$' are sentinels; host only.
 * The symbols go to the FMD writer a run at a time, not one by one. */
static int main_plain2fmd(int argc, char *argv[])
{
	int c, j, ret = 0, cur = -1;
	int64_t run = 0;
	rb3h_fmdw_t *w;
	uint8_t *buf, tab[256];
	optind = 1;
	while ((c = getopt(argc, argv, "o:")) >= 0)
		if (c == 'o' && freopen(optarg, "wb", stdout) == 0) { fprintf(stderr, "ERROR: failed to open '%s' for writing\n", optarg); return 1; }
	if (argc - optind < 1) {
		fprintf(stdout, "Usage: ropebwt3-amd plain2fmd [-o output.fmd] <in.txt>\n");
		return 0;
	}
	buf = (uint8_t*)malloc(1 << 20);
	for (c = 0; c < 256; ++c) tab[c] = (uint8_t)c;
	rb3h_char2nt6(256, tab);
	tab['\n'] = tab['$'] = 0;
	w = rb3h_fmdw_init();
	for (j = optind; j < argc && ret == 0; ++j) {
		FILE *fp = strcmp(argv[j], "-") == 0 ? stdin : fopen(argv[j], "r");
		size_t i, len;
		if (fp == 0) { fprintf(stderr, "ERROR: failed to open '%s'\n", argv[j]); ret = -1; break; }
		while (ret == 0 && (len = fread(buf, 1, 1 << 20, fp)) > 0) {
			for (i = 0; i < len && ret == 0; ++i) {
				const int x = tab[buf[i]];
				if (x == cur) { ++run; continue; }
				if (run > 0) ret = rb3h_fmdw_enc(w, run, cur);
				cur = x, run = 1;
			}
		}
		if (fp != stdin) fclose(fp);
	}
	if (ret == 0 && run > 0) ret = rb3h_fmdw_enc(w, run, cur);
	if (ret == 0) ret = rb3h_fmdw_finish(w);
	if (ret == 0) ret = rb3h_fmdw_dump(w, stdout);
	rb3h_fmdw_destroy(w);
	free(buf);
	return ret == 0 ? 0 : 1;
}

static int usage(FILE *fp)
{
	fprintf(fp, "Usage: ropebwt3-amd <command> <arguments>\n");
	fprintf(fp, "Commands:\n");
	fprintf(fp, "    build      construct a BWT (merge path on an MI355X)\n");
	fprintf(fp, "    merge      merge BWTs (on an MI355X)\n");
	fprintf(fp, "    ssa        generate sampled suffix array (on an MI355X)\n");
	fprintf(fp, "    kount      count k-mers in one or more FM-indexes (on an MI355X)\n");
	fprintf(fp, "    mem        find super-maximal exact matches of queries (on an MI355X)\n");
	fprintf(fp, "    suffix     find the longest matching suffix of queries (on an MI355X)\n");
	fprintf(fp, "    get        retrieve the i-th sequence from a BWT (on an MI355X)\n");
	fprintf(fp, "    remove     take sequences out of a BWT (on an MI355X)\n");
	fprintf(fp, "    dedup      list sequences that are copies of, or lie inside, another one (on an MI355X)\n");
	fprintf(fp, "    overlap    list the suffix-prefix overlaps of the sequences (on an MI355X)\n");
	fprintf(fp, "    unitig     spell the unambiguous paths of the overlap graph (on an MI355X)\n");
	fprintf(fp, "    fetch      retrieve regions of sequences through the sampled suffix array (on an MI355X)\n");
	fprintf(fp, "    hapdiv     haplotype diversity with sliding k-mers (on an MI355X)\n");
	fprintf(fp, "    sw         align queries end to end with CIGAR and positions (on an MI355X)\n");
	fprintf(fp, "    recode     convert an FMD/FMR file to plain text, FMD (-d) or FMR (-b) (host only)\n");
	fprintf(fp, "    plain2fmd  convert BWT in plain text to FMD (host only)\n");
	fprintf(fp, "    version    print the version number\n");
	return fp == stdout ? 0 : 1;
}

int main(int argc, char *argv[])
{
	int ret = 0;
	rb3h_init();
	if (getenv("RB3_VERBOSE")) rb3h_verbose = atoi(getenv("RB3_VERBOSE")); /* (diagnostics: 4 makes the engine print every merge's phases from its HIP events; the reference's level is 3) */
	if (argc == 1) return usage(stdout);
	else if (strcmp(argv[1], "build") == 0) ret = main_build(argc - 1, argv + 1);
	else if (strcmp(argv[1], "merge") == 0) ret = main_merge(argc - 1, argv + 1);
	else if (strcmp(argv[1], "ssa") == 0) ret = main_ssa(argc - 1, argv + 1);
	else if (strcmp(argv[1], "kount") == 0) ret = main_kount(argc - 1, argv + 1);
	else if (strcmp(argv[1], "mem") == 0) ret = main_mem(argc - 1, argv + 1);
	else if (strcmp(argv[1], "suffix") == 0) ret = main_suffix(argc - 1, argv + 1);
	else if (strcmp(argv[1], "get") == 0) ret = main_get(argc - 1, argv + 1);
	else if (strcmp(argv[1], "remove") == 0) ret = main_remove(argc - 1, argv + 1);
	else if (strcmp(argv[1], "dedup") == 0) ret = main_dedup(argc - 1, argv + 1);
	else if (strcmp(argv[1], "overlap") == 0) ret = main_overlap(argc - 1, argv + 1);
	else if (strcmp(argv[1], "unitig") == 0) ret = main_unitig(argc - 1, argv + 1);
	else if (strcmp(argv[1], "fetch") == 0) ret = main_fetch(argc - 1, argv + 1);
	else if (strcmp(argv[1], "hapdiv") == 0) ret = main_hapdiv(argc - 1, argv + 1);
	else if (strcmp(argv[1], "sw") == 0) ret = main_sw(argc - 1, argv + 1);
	else if (strcmp(argv[1], "recode") == 0) ret = main_recode(argc - 1, argv + 1);
	else if (strcmp(argv[1], "plain2fmd") == 0) ret = main_plain2fmd(argc - 1, argv + 1);
	else if (strcmp(argv[1], "version") == 0) { printf("%s\n", RB3H_VERSION); return 0; }
	else { fprintf(stderr, "ERROR: unknown command '%s'\n", argv[1]); return 1; }
	if (rb3h_verbose >= 3 && argc > 2 && ret == 0) { /* main.c:73-80 */
		int i;
		fprintf(stderr, "[M::%s] Version: %s\n", __func__, RB3H_VERSION);
		fprintf(stderr, "[M::%s] CMD:", __func__);
		for (i = 0; i < argc; ++i) fprintf(stderr, " %s", argv[i]);
		fprintf(stderr, "\n[M::%s] Real time: %.3f sec; CPU: %.3f sec; Peak RSS: %.3f GB\n", __func__, rb3h_realtime(), rb3h_cputime(), rb3h_peakrss() / 1024.0 / 1024.0 / 1024.0);
	}
	return ret;
}
