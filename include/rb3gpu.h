/*
 * rb3gpu.h -- C ABI of the MI355X-native BWT-merge engine (librb3gpu.so).
 *
 * This is the drop-in boundary for the hot path of `ropebwt3 build`: every entry
 * point replaces one call the reference's build.c makes on an `mrope_t*` -- and,
 * further down, the calls on either side of it: the suffix sorting of a batch, the
 * run export / FMD packing, the sampled suffix array (citations are file:line in
 * the reference tree).  The opaque `rb3gpu_t`
 * stands where `mrope_t*` stood; it owns a flat run/bit-plane block array in
 * HBM instead of the reference's B+-tree of RLE leaves.  Plain C types only:
 * no HIP, torch or C++ types cross this boundary.  All functions return 0 on
 * success or a negative RB3GPU_E* code (the reference asserts/aborts instead,
 * fm-index.c:125,246); nothing here ever falls back to a CPU implementation.
 */
#ifndef RB3GPU_H
#define RB3GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RB3GPU_ASIZE 6           /* $ACGTN = 0..5, fm-index.h:15 (RB3_ASIZE) */

#define RB3GPU_OK         0
#define RB3GPU_ENODEV    -1      /* no usable HIP device / HIP runtime error */
#define RB3GPU_ENOMEM    -2      /* device or host allocation failed */
#define RB3GPU_EINVAL    -3      /* bad argument (NULL, negative length, ...) */
#define RB3GPU_ESYMBOL   -4      /* a BWT byte is outside 0..5 (fm-index.c:124-125) */
#define RB3GPU_ESTATE    -5      /* call not valid in this state (e.g. merge into an empty index) */
#define RB3GPU_EINTERNAL -6      /* invariant violated on the device (fm-index.c:246 analogue) */
#define RB3GPU_EUNSUP    -7      /* this call cannot serve this index; use the alternative named in its description */

typedef struct rb3gpu_s rb3gpu_t;

typedef struct {
	int32_t device;              /* HIP device ordinal */
	int32_t split_log2;          /* long-chain splitting: start an extra LF walker at every row whose
	                                hashed id is 0 mod 2^split_log2; 0 = automatic, <0 = never split */
	int32_t verbose;             /* >=3: per-phase "[M::...]" lines on stderr like the reference */
	int32_t reserved;
} rb3gpu_opt_t;

/* per-handle counters, all cumulative since rb3gpu_create()/rb3gpu_stats_reset() */
typedef struct {
	double  ms_h2d;              /* host->device copies of partial BWTs */
	double  ms_lf;               /* LF-array construction of B2 (fm-index.c:206-216) */
	double  ms_rank;             /* LF-chain / rank kernels (fm-index.c:160-175, 217-224) */
	double  ms_build;            /* interleave + block-array rebuild (fm-index.c:237-249, 294-299) */
	double  ms_export;           /* run / symbol export kernels + D2H */
	double  ms_chain;            /* k_chain alone (HIP events on the launch stream): the dominant kernel */
	int64_t n_rank_launches;     /* launches of the chain kernel */
	int64_t n_lf_steps;          /* LF steps executed by the chain kernel (incl. speculative ones) */
	int64_t n_symbols_merged;    /* sum of `len` over merge calls */
	int64_t n_rounds;            /* chain-kernel launches incl. fallbacks */
	int64_t n_fallbacks;         /* merges whose optimistic (tentative-record) rank phase had to be redone */
	int64_t bytes_index;         /* current size of the block array + group directory in HBM */
	int64_t bytes_peak;          /* high-water mark of device memory owned by the handle */
	double  ms_ssa;              /* rb3gpu_ssa_gen: kernels + copy-back */
	double  ms_ssa_walk;         /* k_ssa_walk alone (one LF step per row of the index) */
	double  ms_sort;             /* rb3gpu_bwt_from_text: upload + suffix sorting + BWT */
	int64_t n_sort_rounds;       /* prefix-doubling rounds of those calls */
	int64_t n_reb_groups;        /* groups (8192 symbols) of the merges whose rebuild went through the run-space kernel ... */
	int64_t n_reb_groups_window; /* ... and how many of them it handed on to the symbol path (the plane or per-window kernels); counted by the
	                                single-sync merges and by rb3gpu_sh_finish */
	int64_t n_lf_checked;        /* batch rows whose LF relation was verified against the index after the rank phase (approximate) */
	int64_t n_long_settles;      /* merges whose tentative records needed the pointer-jumping settle pass (paths over > 64 walkers) */
	double  ms_alloc;            /* host time inside hipMalloc / hipFree for the handle's buffers (they grow with the index; replaced ones are freed in bulk) */
	int64_t n_allocs;
	int64_t n_reb_again;         /* rebuilds done twice because a buffer sized by an estimate did not take the result */
	int64_t bytes_rebuild;       /* algorithmic bytes of the rebuilds: per merge 9 B x rows + old block array + new block array */
	int64_t n_thinned;           /* merges done again with fewer, longer walkers because the table of tentative stretches was full */
	int64_t tent_mask_bits;      /* width of the drop-out masks the last single-sync merge settled its tentative records with: 256, or 512 / 1024 /
	                                2048 once walkers have met intervals of more matching suffixes than that (an index of > 255 relatives) */
	int64_t n_junctions_checked; /* junctions of the speculative walk (a walker meeting somebody's record; a drop-out event) whose LF relation was
	                                verified after the rank phase: all of them, on every merge with text-order words */
	int64_t n_peer_rounds;       /* lock-step rounds of the interval-sharded merge that ran as PEER ROUNDS (one kernel per rank, states written straight
	                                into the owner's receive buffer; rb3gpu_comm_t.stream_barrier): 0 where the host drove the rounds */
	int64_t n_reb_groups_tier2;  /* groups of n_reb_groups that the small tier of the run-space kernel handed to the medium one (0 for a rebuild that
	                                starts with the medium tier); n_reb_groups_window of them went on to the symbol path */
} rb3gpu_stats_t;

void rb3gpu_opt_init(rb3gpu_opt_t *opt);
const char *rb3gpu_strerror(int err);

/* mr_init (mrope.c:15-26) / mr_destroy (mrope.c:28-34) */
rb3gpu_t *rb3gpu_create(const rb3gpu_opt_t *opt);
void rb3gpu_destroy(rb3gpu_t *h);

/* rb3_enc_plain2fmr(len, bwt, max_nodes, block_len, n_threads), fm-index.c:114-137,
 * called at build.c:77,223 -- index the first batch.  `bwt` is caller-owned host memory,
 * read-only during the call.  Any previous content of the handle is dropped. */
int rb3gpu_from_plain(rb3gpu_t *h, int64_t len, const uint8_t *bwt);

/* rb3_fmi_merge_plain(r, len, seq, n_threads), fm-index.c:279-303, called at
 * build.c:78,226 -- merge the partial BWT of a later batch in place. */
int rb3gpu_merge_plain(rb3gpu_t *h, int64_t len, const uint8_t *bwt);

/* Same two operations with the partial BWT already resident in HBM on the handle's
 * device (`d_bwt` is a device pointer).  Used by the pipelined build and by bench.py,
 * whose timed region starts with inputs in HBM.  commit=0 computes the merged block
 * array and then discards it, leaving the index unchanged (repeatable benchmark step). */
int rb3gpu_from_plain_dev(rb3gpu_t *h, int64_t len, const uint8_t *d_bwt);
int rb3gpu_merge_plain_dev(rb3gpu_t *h, int64_t len, const uint8_t *d_bwt, int commit);

/* An LF WALKER follows one string of the batch right to left (the loop of rb3_mg_rank1_plain,
 * fm-index.c:160-175).  The reference starts one per string; this engine can also start walkers in
 * the middle of long strings (see rb3gpu_kernels.h).  Callers that still hold the suffix array of
 * the batch (sais-ss.c:23-26 has it when the BWT is written) can say where: */
typedef struct {
	int64_t row;                 /* row of B2 (rank of the suffix in the batch) where the walker starts */
	int64_t ka0;                 /* exact insertion point of that suffix in B1 if known (sentinel rows:
	                                acc[1] of the index, fm-index.c:164), else -1 */
	int64_t nsteps;              /* LF steps to the end of the walker's segment: the text distance to the walker on its left, plus the steps the
	                                walker starts outside its segment (flags >> 8) */
	int64_t flags;               /* RB3GPU_WK_* in the low byte; flags >> 8 & 255: a walker given by text position may start that many positions
	                                to the RIGHT of its segment (rb3h_walkers_text does: 32, the age from which a walker records), on rows its
	                                right neighbour owns and records; flags >> 16 & 255: if not 0, the walker does not start at all when the
	                                row that many positions further right already carries a record (it comes too late: rb3h_walkers_text, RB3H_PROBE = 64) */
} rb3gpu_walker_t;
#define RB3GPU_KA_SENTINEL (-2)  /* ka0 of a sentinel row: the engine substitutes acc[1] of the index (in a sorted order: p0 of the string, rb3gpu_set_order) */
#define RB3GPU_WK_CHECK 2        /* the rows ahead may already be recorded: check each before recording */

/* rb3gpu_merge_plain with an explicit walker list (host memory); same result, more parallelism
 * and no dependence on how the suffix array scatters the strings.  An entry that is not a walker of this batch (row outside it, no
 * steps) makes the call return RB3GPU_EINVAL with nothing installed; the list is checked on the device, by the kernel that walks it. */
int rb3gpu_merge_plain_walkers(rb3gpu_t *h, int64_t len, const uint8_t *bwt, int64_t n_walkers, const rb3gpu_walker_t *walkers);
/* (device BWT) walkers == NULL: one walker per string, made on the device; n_walkers = the number of strings of the batch */
int rb3gpu_merge_plain_dev_walkers(rb3gpu_t *h, int64_t len, const uint8_t *d_bwt, int64_t n_walkers, const rb3gpu_walker_t *walkers, int commit);

/* The same merge in three stages, for a multi-GPU build with the index replicated and the batch's
 * walkers sharded by text range: every rank calls begin (LF array of the whole batch), walk on ITS
 * walkers (several calls allowed: hand-off values arriving from the neighbour rank start fix-up
 * walkers), then the ranks combine pos[] (RCCL all-reduce MAX over the device buffer returned by
 * rb3gpu_mg_pos_ptr: rows not yet recorded hold negative words, identical on every rank) and every rank calls finish.  d_pos_ext, if not NULL, is a
 * caller-owned device buffer of len int64 to use for pos[].  stop_row >= 0 names the row where the
 * territory of the next rank begins (the start row of its top walker): any walker reaching it stops,
 * and *arrive (host, optional) receives the exact value a walker arrived there with, or -1 if none did. */
int rb3gpu_mg_begin(rb3gpu_t *h, int64_t len, const uint8_t *d_bwt, void *d_pos_ext, int64_t acc2[RB3GPU_ASIZE+1]);
int rb3gpu_mg_walk(rb3gpu_t *h, int64_t n_walkers, const rb3gpu_walker_t *walkers, int64_t stop_row, int64_t *arrive);
int rb3gpu_mg_pos_ptr(rb3gpu_t *h, void **d_pos, int64_t *len);
int rb3gpu_mg_finish(rb3gpu_t *h, int commit);

/* rb3_mg_rank_plain(fa, len, seq, rb, acc, n_threads), fm-index.c:202-225 -- the rank phase
 * alone, for parity tests against the reference's rb[] array: on return pos[kb] = ka[kb]+kb,
 * the merged position of row kb of B2 (= rb[kb]>>6 in the reference), and acc2[7] the C array
 * of B2.  The index is not modified.  `pos` is host memory of `len` int64. */
int rb3gpu_mg_rank_plain(rb3gpu_t *h, int64_t len, const uint8_t *bwt, int64_t *pos, int64_t acc2[RB3GPU_ASIZE+1]);

/* the same through the walker-list entry point (tests: pos[] of the single-synchronisation path) */
int rb3gpu_mg_rank_plain_walkers(rb3gpu_t *h, int64_t len, const uint8_t *bwt, int64_t n_walkers, const rb3gpu_walker_t *walkers, int64_t *pos, int64_t acc2[RB3GPU_ASIZE+1]);

/* rb3_fmi_rank1a(f, k, ok), fm-index.h:109-112 -> mr_rank2a, mrope.c:71-121: for each of the
 * n query offsets k[i] in [0, total], ok[6*i+c] = #{j < k[i] : B[j] = c}.  Host arrays. */
int rb3gpu_rank1a_batch(rb3gpu_t *h, int64_t n, const int64_t *k, int64_t *ok);

/* rb3_fmi_get_acc (fm-index.c:544-550) -> mr_get_ac (mrope.h:113-120): acc[a] = #symbols < a */
int rb3gpu_get_acc(const rb3gpu_t *h, int64_t acc[RB3GPU_ASIZE+1]);
int64_t rb3gpu_get_tot(const rb3gpu_t *h);          /* mr_get_tot, mrope.h:122-130 */

/* Ordered export of the index as runs, replacing the leaf-block iteration of
 * rb3_enc_fmr2fmd (fm-index.c:31-54) / mr_print_bwt (mrope.c:201-214): emit(c, l, data) is
 * called on the host for consecutive runs, in BWT order; adjacent calls may carry the same
 * symbol (the FMD writer coalesces, rld0.c:153-161).  A non-zero return from emit aborts. */
typedef int (*rb3gpu_emit_f)(void *data, int c, int64_t l);
int rb3gpu_export_runs(rb3gpu_t *h, rb3gpu_emit_f emit, void *data);

/* The same runs in bulk, for writers that want a tight loop instead of a call per run: emit receives arrays of
 * words start << 3 | sym, one per MAXIMAL run in BWT order (adjacent runs differ in symbol); run i ends where
 * run i+1 starts -- possibly in the next call -- and the last call is (n = 0, words = NULL, end = total length),
 * which closes the last run.  In the other calls end is -1. */
typedef int (*rb3gpu_emit_words_f)(void *data, int64_t n, const uint64_t *words, int64_t end);
int rb3gpu_export_run_words(rb3gpu_t *h, rb3gpu_emit_words_f emit, void *data);

/* The data section of the .fmd packed on the GPU (rb3_enc_fmr2fmd + rld_enc + rld_enc_finish, fm-index.c:31-52,
 * rld0.c:107-216): *words receives a malloc'ed array (free it with rb3gpu_host_free) of *n_words 64-bit words, the
 * blocks incl. the trailing header-only block, exactly what rld_dump writes between the file header and the rank
 * index (rld0.c:237-239; n_bytes = 8 * *n_words).  Blocks with 16-bit and with 32-bit headers (rld0.c:116-128: the
 * block before holds fewer than 0x4000 / 0x40000000 symbols) are packed on the device; an index with a block of 2^30
 * symbols or more (64-bit header) returns RB3GPU_EUNSUP and the caller packs the runs of rb3gpu_export_run_words on
 * the host. */
int rb3gpu_export_fmd_words(rb3gpu_t *h, uint64_t **words, int64_t *n_words);
void rb3gpu_host_free(void *p);

/* Page-locked host memory (hipHostMalloc) for batch buffers: a text or BWT that the caller builds in such a buffer is copied
 * to HBM by one DMA at PCIe speed (rb3gpu_from_plain, rb3gpu_merge_plain*, rb3gpu_sort_text, rb3gpu_sorter_*); any other host
 * pointer is staged through pinned buffers chunk by chunk, which a single host thread feeds at memcpy speed.  The reference's
 * counterpart is the malloc of the batch buffer (build.c:205, io.c:92).  NULL: no such memory to be had (use malloc). */
void *rb3gpu_pinned_alloc(int64_t n_bytes);
void rb3gpu_pinned_free(void *p);

/* The text distance between the LF walkers of a batch of n_strings long strings, `len` symbols in all (the `step` of
 * rb3h_walkers_text / rb3h_build_bwt_walkers; the reference has one chain per string, fm-index.c:217-224): as many walkers as the
 * walker kernel keeps resident on `device` -- one per group of eight lanes, compute units x 160 -- because a wave lasts as long as
 * its longest walker and walkers beyond the resident ones only start when others have finished; never closer than 192 positions
 * (a walker must be 16 steps old before it records -- RB3_TENT_MIN_AGE --, and segments shorter than 128 are not split).  < 0: no such device. */
int64_t rb3gpu_walker_step(int device, int64_t len, int64_t n_strings);

/* The whole BWT as one symbol per byte (0..5) into host memory of rb3gpu_get_tot() bytes;
 * small indexes / tests only. */
int rb3gpu_export_plain(rb3gpu_t *h, uint8_t *out);

/* same into device memory of the handle's GPU (rb3gpu_get_tot() bytes): the plain BWT of an index
 * is itself a valid partial BWT, so a whole index can be merged into another one with
 * rb3gpu_merge_plain_dev -- the tree-shaped multi-GPU build (rb3_fmi_merge, fm-index.c:251-277) */
int rb3gpu_export_plain_dev(rb3gpu_t *h, uint8_t *d_out);
int rb3gpu_export_plain_range_dev(rb3gpu_t *h, int64_t beg, int64_t end, uint8_t *d_out); /* symbols [beg, end) only */
/* bounds[0..n] of n intervals of positions that hold about equal BYTES of the block array (cut at group boundaries) */
int rb3gpu_balanced_bounds(rb3gpu_t *h, int n, int64_t *bounds);

/* Sampled suffix array of the index, `ropebwt3 ssa` (rb3_ssa_gen ssa.c:54-81; the words are those of
 * rb3_ssa_t fm-index.h:28-36 as written by rb3_ssa_dump ssa.c:198-213):
 *   r2i[k], k in [0, m): the string whose first suffix is reached from sentinel row k (ssa.c:36);
 *   ssa[x], x in [0, n_ssa): for row m + (x << ssa_shift), (offset of its suffix in its string) << ms | string.
 * rb3gpu_ssa_dims gives the sizes (m = acc[1], n_ssa = ceil((n - m) / 2^ssa_shift), ms = bits of m as in
 * ssa.c:62-64); rb3gpu_ssa_gen fills caller-owned host arrays of m and n_ssa words. */
int rb3gpu_ssa_dims(const rb3gpu_t *h, int ssa_shift, int64_t *m, int64_t *n_ssa, int *ms);
int rb3gpu_ssa_gen(rb3gpu_t *h, int ssa_shift, uint64_t *r2i, uint64_t *ssa);

/* The merge of a batch that comes with its TEXT-ORDER WORDS: d_tw[t] = row of the suffix at text position t << 3 |
 * the symbol before it (0 at the start of a string), i.e. the inverse suffix array of the batch next to its BWT
 * (rb3gpu_sort_text / rb3gpu_sorter_sort produce both; a host sorter has the suffix array and inverts it).
 * walkers[i].row is then the TEXT POSITION a walker starts at (a sentinel's walker: the position of the sentinel),
 * everything else as in rb3gpu_merge_plain_dev_walkers.  walkers == NULL: one walker per string, made on the device
 * (n_walkers = the number of strings of the batch; short strings, i.e. reads).  Same result as rb3_fmi_merge_plain (fm-index.c:279-303);
 * the LF walkers read their batch-side state as a stream instead of one random row word per step.
 * d_bwt: len bytes, d_tw: len 64-bit words, both device memory.  rb3gpu_mg_rank_text_dev: the rank phase alone
 * (pos[] as in rb3gpu_mg_rank_plain), for parity tests. */
int rb3gpu_merge_text_dev(rb3gpu_t *h, int64_t len, const uint8_t *d_bwt, const uint64_t *d_tw, int64_t n_walkers, const rb3gpu_walker_t *walkers, int commit);
/* the same for a caller that also has the batch's suffix array (d_sa[i] = text position of the suffix of row i, len x u32 of device
 * memory: the GPU sorter's rb3gpu_sorter_sort[_uploaded]_sa / rb3gpu_sort_text_sa leave it behind the text-order words).  The
 * walkers may then leave their records in text order -- eight consecutive words per store instead of eight random rows -- and the
 * validation pass gathers them into row order through d_sa: what an index that lives in HBM wants (a batch of reads into a large
 * index: the record stores are two thirds of the walk).  d_sa == NULL: rb3gpu_merge_text_dev.  Same result either way. */
int rb3gpu_merge_text_sa_dev(rb3gpu_t *h, int64_t len, const uint8_t *d_bwt, const uint64_t *d_tw, const uint32_t *d_sa, int64_t n_walkers, const rb3gpu_walker_t *walkers, int commit);
/* The same with the walker list made ON THE DEVICE: the caller passes the number of strings of the batch and a spacing (rb3gpu_walker_step), the
 * engine puts a walker at every sentinel and at every multiple of `step` strictly inside a string -- the list rb3h_walkers_text makes on the host
 * (70 ms of one core per 152-genome build), by two small kernels in front of the walk.  d_sa may be NULL.  A wrong string count: RB3GPU_EINVAL. */
int rb3gpu_merge_text_step_dev(rb3gpu_t *h, int64_t len, const uint8_t *d_bwt, const uint64_t *d_tw, const uint32_t *d_sa, int64_t n_strings, int64_t step, int commit);
/* that list on the host, without its empty slots (tests): *walkers is malloc'ed, free it with rb3gpu_host_free */
int rb3gpu_walkers_step_dev(rb3gpu_t *h, int64_t len, const uint64_t *d_tw, int64_t n_strings, int64_t step, int64_t *n_walkers, rb3gpu_walker_t **walkers);
int rb3gpu_mg_rank_text_dev(rb3gpu_t *h, int64_t len, const uint8_t *d_bwt, const uint64_t *d_tw, int64_t n_walkers, const rb3gpu_walker_t *walkers, int64_t *pos, int64_t acc2[RB3GPU_ASIZE+1]);

/* Partial BWT of one batch on the GPU, instead of rb3_build_sais on the host (sais-ss.c:10-56; libsais in GSA
 * mode: the i-th sentinel sorts before the (i+1)-th, sais-ss.c:16-21).  text: len symbols 0..5 in host memory,
 * every string terminated by 0 (so text[len-1] == 0), exactly what rb3_seq_read leaves in seq->s (io.c:104-125);
 * it is not modified.  d_bwt: len bytes of device memory (rb3gpu_dev_alloc) that receive the BWT, ready for
 * rb3gpu_from_plain_dev / rb3gpu_merge_plain_dev[_walkers].  If step > 0 and ckrow != NULL, ckrow[i] (host,
 * ceil(len / step) entries) receives the row of the suffix that starts at text position i * step -- the sampled
 * inverse suffix array a walker list is made from.  len < 2^31. */
int rb3gpu_bwt_from_text(rb3gpu_t *h, int64_t len, const uint8_t *text, uint8_t *d_bwt, int64_t step, int64_t *ckrow);
/* the same, with the text-order words of the batch (len 64-bit words of device memory) for rb3gpu_merge_text_dev */
int rb3gpu_sort_text(rb3gpu_t *h, int64_t len, const uint8_t *text, uint8_t *d_bwt, uint64_t *d_tw);
/* ... and the suffix array (len x u32 of device memory) for rb3gpu_merge_text_sa_dev */
int rb3gpu_sort_text_sa(rb3gpu_t *h, int64_t len, const uint8_t *text, uint8_t *d_bwt, uint64_t *d_tw, uint32_t *d_sa);

/* The same sorter as an object of its own (own HIP stream and scratch, independent of any index handle), so that a
 * host thread can sort batch i+1 while another merges batch i -- the pipeline of build.c:55-83, 186-201 with both
 * stages on the GPU.  rb3gpu_sorter_bwt blocks until the BWT is complete and returns it in one of the sorter's two
 * output buffers (*d_bwt, device memory, len bytes, valid until rb3gpu_sorter_release; it waits while both are out).
 * A sorter is used by one thread at a time; release may come from any thread. */
typedef struct rb3gpu_sorter_s rb3gpu_sorter_t;
rb3gpu_sorter_t *rb3gpu_sorter_create(int device);
void rb3gpu_sorter_destroy(rb3gpu_sorter_t *s);
int rb3gpu_sorter_bwt(rb3gpu_sorter_t *s, int64_t len, const uint8_t *text, void **d_bwt, int64_t step, int64_t *ckrow);
/* BWT + text-order words (*d_tw: len 64-bit words in the same output buffer; released together with *d_bwt) */
int rb3gpu_sorter_sort(rb3gpu_sorter_t *s, int64_t len, const uint8_t *text, void **d_bwt, void **d_tw);
int rb3gpu_sorter_release(rb3gpu_sorter_t *s, void *d_bwt);
/* rb3gpu_sorter_sort in its two stages, for callers that time or overlap them: the upload of the text (the H2D copy of the
 * merge path, SURVEY 8(d): one DMA if `text` lies in memory from rb3gpu_pinned_alloc, else through pinned staging buffers),
 * then the suffix sorting of the text uploaded last (len must be the same). */
int rb3gpu_sorter_upload(rb3gpu_sorter_t *s, int64_t len, const uint8_t *text);
/* the same for a batch of at most 32 records on both strands (rb3_seq_read with is_for and is_rev: per record l symbols, 0, the l
 * symbols of the reverse complement, 0; io.c:84-102): only the forward strands are copied, the reverse complements (io.c:30-40) are
 * written on the device.  pair_start[i] = offset of record i in `text` (pair_start[0] = 0; record n_pairs - 1 ends at len).
 * RB3GPU_EINVAL if the text does not have that layout (use rb3gpu_sorter_upload). */
int rb3gpu_sorter_upload_fwd(rb3gpu_sorter_t *s, int64_t len, const uint8_t *text, int64_t n_pairs, const int64_t *pair_start);
/* rb3gpu_sorter_upload_fwd in two halves, so that the copy of the NEXT batch runs beside the merge of the current one on the copy
 * engine (what the CLI gets from its sorter thread; build.c:203-239 reads the next batch while the current one is inserted):
 * _begin queues the copies and the strand kernel on the sorter's stream and returns at once if `text` is page-locked
 * (rb3gpu_pinned_alloc; otherwise it is rb3gpu_sorter_upload_fwd), and `text` must stay untouched until _end -- or the sort, which
 * the stream orders behind the copies anyway -- has returned.  _end waits for whatever the sorter's stream still holds. */
int rb3gpu_sorter_upload_fwd_begin(rb3gpu_sorter_t *s, int64_t len, const uint8_t *text, int64_t n_pairs, const int64_t *pair_start);
int rb3gpu_sorter_upload_end(rb3gpu_sorter_t *s);
int rb3gpu_sorter_sort_uploaded(rb3gpu_sorter_t *s, int64_t len, void **d_bwt, void **d_tw);
/* the same with the suffix array (*d_sa: len x u32 behind the text-order words in the same output buffer, released with *d_bwt) */
int rb3gpu_sorter_sort_uploaded_sa(rb3gpu_sorter_t *s, int64_t len, void **d_bwt, void **d_tw, void **d_sa);
int rb3gpu_sorter_sort_sa(rb3gpu_sorter_t *s, int64_t len, const uint8_t *text, void **d_bwt, void **d_tw, void **d_sa);
/* cumulative times of a sorter: text upload (host -> HBM, through its pinned staging buffer) and suffix sorting proper */
int rb3gpu_sorter_stats(const rb3gpu_sorter_t *s, double *ms_upload, double *ms_sort, int64_t *n_batches, int64_t *n_symbols);

/* Sorted string orders (build -s / -r; mrope.h MR_SO_*).  The reference's ropebwt2 insertion (mr_insert_multi) builds the BWT of a
 * collection in reverse lexicographic order (RLO: the strings sorted by their reversed contents, $ < A < C < G < T < N, a string that is
 * a suffix of another first) or reverse-complement lexicographic order (RCLO: the same with $ < T < G < C < A < N).  That BWT is the
 * input-order BWT of the collection reordered that way, so the engine builds it through its own merge: every batch is put into the order
 * on the device before it is suffix-sorted, and the sentinels of a merged batch go to their places among the index's strings (p0, below)
 * instead of behind them all.  The default is RB3GPU_SO_IO: nothing changes.
 *   rb3gpu_set_order: the order of the index in the handle (set it before the first merge into an index built that way).  Honoured by
 *     rb3gpu_merge_plain[_dev][_walkers], rb3gpu_merge_plain_dev_walkers, rb3gpu_merge_text_dev, rb3gpu_merge_text_sa_dev,
 *     rb3gpu_merge_text_step_dev, rb3gpu_mg_rank_plain[_walkers], rb3gpu_mg_rank_text_dev -- the batch given to them must already be in the
 *     order --, and by rb3gpu_bwt_from_text / rb3gpu_sort_text[_sa], which order the text first.  RB3GPU_EUNSUP from rb3gpu_mg_begin,
 *     rb3gpu_merge_index, rb3gpu_merge_fmd_words and the interval-sharded merge (rb3gpu_sh_*; rb3gpu_shard_split returns NULL).
 *   rb3gpu_sorter_set_order: a sorter orders every batch before it sorts it (after the reverse strands of rb3gpu_sorter_upload_fwd).
 *   rb3gpu_order_strings_dev: d_text (len symbols of device memory, strings ending in 0) reordered in place, in order so (RLO or RCLO).
 *   rb3gpu_sentinel_ranks_dev: p0 of the next merge of a batch (already in order) into the handle's index, into host memory (n_strings
 *     entries): p0[i] = the index strings that sort before string i in the handle's order.  d_tw may be NULL (the strings are then read
 *     through the batch's BWT).  RB3GPU_EINVAL if n_strings is not the batch's count, RB3GPU_EINTERNAL if p0 decreases anywhere (a batch
 *     not in the order), RB3GPU_ESTATE for an empty index or the input order. */
#define RB3GPU_SO_IO   0
#define RB3GPU_SO_RLO  1
#define RB3GPU_SO_RCLO 2
int rb3gpu_set_order(rb3gpu_t *h, int so);
int rb3gpu_get_order(const rb3gpu_t *h);
int rb3gpu_sorter_set_order(rb3gpu_sorter_t *s, int so);
int rb3gpu_sorter_order_stats(const rb3gpu_sorter_t *s, double *ms_order); /* cumulative time of the ordering (not in ms_sort of rb3gpu_sorter_stats) */
int rb3gpu_order_strings_dev(rb3gpu_t *h, int64_t len, uint8_t *d_text, int so);
int rb3gpu_sentinel_ranks_dev(rb3gpu_t *h, int64_t len, const uint8_t *d_bwt, const uint64_t *d_tw, int64_t n_strings, int64_t *p0);

/* Import for `build -i` (rb3_enc_fmd2fmr fm-index.c:56-85, mr_restore mrope.c:161-177):
 * runs[i] = len<<3 | sym in BWT order (host memory). */
int rb3gpu_from_runs(rb3gpu_t *h, int64_t n_runs, const uint64_t *runs);

/* rb3_enc_fmd2fmr (fm-index.c:56-85: rld_dec over the whole file + rope inserts) with the decoding on the device:
 * `words` (host) is the word stream of an FMD file -- what follows the 80-byte header, n_words = n_bytes / 8
 * (rld0.c:218-243) --, mcnt[6] the symbol counts of the header (NULL: not checked).  One thread decodes one 64-byte
 * block (blocks are self-contained, rld0.h:85-122); the symbols are built into the block array as by
 * rb3gpu_from_plain_dev.  RB3GPU_ESYMBOL: not a valid stream. */
int rb3gpu_from_fmd_words(rb3gpu_t *h, int64_t n_words, const uint64_t *words, const int64_t mcnt[RB3GPU_ASIZE]);
/* the same stream decoded on the device and merged into the index the handle holds as one batch, like rb3gpu_merge_plain
 * (`ropebwt3 merge`, main.c:84-133, with the right-hand index taken as its BWT) */
int rb3gpu_merge_fmd_words(rb3gpu_t *h, int64_t n_words, const uint64_t *words, const int64_t mcnt[RB3GPU_ASIZE]);

/* BRE, the run-length interchange format of the reference (bre.c / bre.h; `build -e`: mr_print_bre, build.c:85-106; read wherever an index is read:
 * rld_restore, rld0.c:245-283).  A RECORD is one symbol byte followed by b_per_run length bytes, little-endian; a run longer than 2^(8 b_per_run) - 1 is
 * split into records of that length and a remainder, and a reader joins consecutive records of one symbol.  These calls handle the records; the file's
 * header and footer are the host's (rb3h_bre_*).
 *   rb3gpu_export_bre  the records of the index in order, packed on the device a piece of the runs at a time (rb3gpu_tune "bre_piece": runs per piece,
 *                      default 64 M; a piece ends with a whole group of 8192 symbols) and handed to emit in consecutive slabs of bytes (host memory valid
 *                      during the call only; a nonzero return stops the export: RB3GPU_EINVAL).  b_per_run 1..4.  st (may be NULL): n_rec records written,
 *                      n_sym symbols, n_run maximal runs -- the footer's three counts --, n_pieces, ms_scan (record counts + scan) and ms_pack (the kernel
 *                      that writes the records).
 *   rb3gpu_from_bre    the index of n_rec records (host memory, n_rec * (1 + b_per_run) bytes), decoded on the device; b_per_run 1..8.  st: the counts the
 *                      DEVICE found -- the caller holds them against the file's footer --, ms_scan, ms_fill (symbols written, where the index is built in
 *                      one piece), n_pieces (chunks of the two-pass builder above rb3gpu_tune "load_chunk" groups, as for an FMD stream).
 *   rb3gpu_merge_bre   the same records merged into the handle's index as one batch, like rb3gpu_merge_fmd_words.
 * RB3GPU_ESYMBOL: a record with a symbol above 5, of no symbols or of 2^56 and more; RB3GPU_EINVAL: NULL, n_rec <= 0, b_per_run out of range.
 * A caller that may still refuse the file for its footer can keep the handle quiet meanwhile: rb3gpu_tune "verbose" sets the level of rb3gpu_opt_t. */
typedef struct { int64_t n_rec, n_sym, n_run, n_pieces; double ms_scan, ms_pack, ms_fill; } rb3gpu_bre_stats_t;
typedef int (*rb3gpu_emit_bytes_f)(void *data, int64_t n, const uint8_t *bytes);
int rb3gpu_export_bre(rb3gpu_t *h, int b_per_run, rb3gpu_emit_bytes_f emit, void *data, rb3gpu_bre_stats_t *st); /* records only, in order */
int rb3gpu_from_bre(rb3gpu_t *h, int b_per_run, int64_t n_rec, const uint8_t *records, rb3gpu_bre_stats_t *st);
int rb3gpu_merge_bre(rb3gpu_t *h, int b_per_run, int64_t n_rec, const uint8_t *records, rb3gpu_bre_stats_t *st);

/* rb3_fmi_merge(fa, fb), fm-index.c:251-277 (`ropebwt3 merge`, main.c:84-133) between two handles: every string of the index in
 * `src` is merged into `h` as one batch (its sentinels rank after those of `h`, fm-index.c:147).  The two may sit on different
 * GPUs: the plain BWT of `src` goes device to device (xGMI).  This is the tree step of a partitioned multi-GPU build
 * (`ropebwt3-amd build --gpus N`): slices of the input indexed on N devices, then merged pairwise in input order. */
int rb3gpu_merge_index(rb3gpu_t *h, rb3gpu_t *src);

/* INTERVAL-SHARDED INDEX over several GPUs (one process and one handle per GPU; no reference analogue beyond the walk over
 * the per-rope totals in mr_rank2a, mrope.c:76-88, and the kt_for over strings, fm-index.c:217-224).  The accumulated BWT is
 * cut into n_iv contiguous intervals of positions, iv_bounds[i] .. iv_bounds[i+1]; the handle of rank i holds the block array
 * of interval i only (build it with rb3gpu_from_plain[_dev] from that slice of the BWT).  A chain STATE is the text position
 * of the current suffix of a string of the batch and its insertion point ka in the whole BWT; it lives on the rank whose
 * interval contains ka.  The batch (its text-order words d_tw, rb3gpu_sort_text) is replicated on every rank.
 *   rb3gpu_sh_step   one LF step (fm-index.c:166-173) for the n_states states resident here: ka is recorded for the suffix's
 *                    row in d_ka (len of the batch int64, -1 = not recorded), the next states are written to d_send GROUPED
 *                    BY THE INTERVAL THAT OWNS THEM, counts[d] of them for interval d (the split sizes of the all-to-all),
 *                    counts[n_iv] = chains that reached the start of their string.  adj[c] = C[c] of the whole BWT + symbols c
 *                    in the intervals before this one - C[c] of this interval (rb3gpu_get_acc of every rank, all-gathered).
 *   rb3gpu_sh_finish the rows jlo .. jlo + n_rows - 1 of the batch are the ones whose insertion points lie in this interval
 *                    (ka is monotone in the row number, so they are contiguous, and this rank recorded every one of them):
 *                    interleave them into the interval (worker_mgins, fm-index.c:237-249) and rebuild its block array. */
#define RB3GPU_SH_MAXIV 64
typedef struct { int64_t tp, ka; } rb3gpu_state_t;
int rb3gpu_sh_step(rb3gpu_t *h, int64_t n_states, const rb3gpu_state_t *d_in, const uint64_t *d_tw, int64_t *d_ka, const int64_t adj[RB3GPU_ASIZE],
		int n_iv, const int64_t *iv_bounds, int my_iv, rb3gpu_state_t *d_send, int64_t *counts);
int rb3gpu_sh_finish(rb3gpu_t *h, int64_t jlo, int64_t n_rows, const uint8_t *d_bwt, const int64_t *d_ka, int64_t iv_start, int commit);

/* The whole merge of one batch into the interval-sharded index, DRIVEN FROM THE LIBRARY (rb3_mg_rank_plain + worker_mgins,
 * fm-index.c:202-249, with the kt_for over strings of 217-224 cut by interval instead of by thread): every rank calls
 * rb3gpu_sh_merge with the same batch and bounds; per lock-step round there is ONE kernel (k_sh_round: LF step, record, next
 * states written straight into per-destination send regions), one read-back of the split sizes, one all-gather of them and one
 * all-to-all of 16-byte states -- or, over a communicator with stream_barrier (below), ONE kernel per round and nothing else.  The rows that land in an interval are kept as (row, insertion point) pairs -- 16 bytes per
 * landed row, nothing of the size of the whole batch -- and placed when the walk is over; then the interval is rebuilt.
 * What connects the ranks is a COMMUNICATOR of two collectives (host vectors of int64; device buffers of states):
 *   all_gather  every rank contributes n int64, recv gets world * n of them in rank order
 *   all_to_all  region d of this rank's send buffer (d_send + d * stride states, send_cnt[d] states) goes to rank d; d_recv
 *               receives recv_cnt[s] states from every rank s, packed in rank order.  `stream` is the HIP stream the engine's
 *               kernels run on: the send regions are complete on it, and d_recv must be usable on it when the call returns.
 * Both return 0 or a negative RB3GPU_E* code; a rank that fails must make the others fail too (abort), not leave them waiting.
 * Three communicators ship with the library: ranks as THREADS of one process with one device each (rb3gpu_group_*: barriers +
 * peer copies over xGMI -- what `ropebwt3-amd build --gpus N --interval` uses), one PROCESS per GPU over RCCL (rb3gpu_rccl_*:
 * grouped ncclSend/ncclRecv on the engine's stream, librccl loaded at run time), and any pair of callbacks (tests: gloo).
 *   iv_bounds  world + 1 positions, the same on every rank; updated to the bounds after the merge when commit != 0
 *   chain_tp   text positions of the batch's sentinels (host, n_chains of them, the same on every rank): where the chains start
 *   n_rounds   (may be NULL) lock-step rounds this merge took = longest string + 1 */
typedef struct rb3gpu_comm_s {
	void *ctx;
	int rank, world;
	int (*all_gather)(void *ctx, const int64_t *send, int n, int64_t *recv);
	int (*all_to_all)(void *ctx, const rb3gpu_state_t *d_send, int64_t stride, const int64_t *send_cnt, rb3gpu_state_t *d_recv, const int64_t *recv_cnt, void *stream);
	void (*abort)(void *ctx);   /* may be NULL: called by a rank whose merge failed locally, so that the others do not wait for it */
	/* may be NULL.  Not NULL says two things: (1) the ranks can address each other's device memory (one process, peer access: a pointer that
	 * all_gather carried from another rank can be given to a kernel here), and (2) stream_barrier(ctx, stream) makes everything this rank queues
	 * on `stream` AFTER the call wait for everything EVERY rank queued on its stream BEFORE its call -- without waiting for the devices (events the
	 * streams wait for, not a host synchronisation).  With it the lock-step rounds of rb3gpu_sh_merge[_text] run as PEER ROUNDS: one kernel per
	 * rank and round that writes the next states straight into the owner's receive buffer over xGMI, no read-back, no all-gather, no all-to-all. */
	int (*stream_barrier)(void *ctx, void *stream);
	/* may be NULL (then a device pointer means the same on every rank: threads of one process).  Ranks that are PROCESSES name a device buffer to each other
	 * by a handle of 8 words (peer_export: 0 or a negative code) which all_gather carries and the other side turns into a pointer of its own address space
	 * (peer_import: NULL if it cannot; with handle == NULL: the rank named is about to replace its buffers -- whatever is mapped of them here is given up, NULL is
	 * returned) -- HIP IPC memory handles in rb3gpu_ipc_peer_enable below. */
	int (*peer_export)(void *ctx, void *d_ptr, int64_t handle[8]);
	void *(*peer_import)(void *ctx, int rank, const int64_t handle[8]);
} rb3gpu_comm_t;
int rb3gpu_sh_merge(rb3gpu_t *h, const rb3gpu_comm_t *comm, int64_t *iv_bounds, int64_t len, const uint8_t *d_bwt, const uint64_t *d_tw,
		int64_t n_chains, const int64_t *chain_tp, int commit, int64_t *n_rounds);
/* The same with the BATCH sharded as well (what rb3gpu_shard_merge runs): every rank holds d_tprev -- the symbol before every text position,
 * one byte each, the only thing a step needs of the batch (rb3gpu_tprev_from_tw makes it from the text-order words) -- and d_tw_slice, the
 * text-order words of ITS text range [len * rank / world, len * (rank + 1) / world) only.  A record is (text position, insertion point); when
 * the chains have ended, one all-to-all takes the records to the owners of their text positions and one brings row << 3 | symbol back (the same
 * 16-byte collective as the rounds'): replicated 1 byte per batch symbol instead of 9, and 16 bytes per symbol cross the links once instead of
 * 8 (world - 1) out of one device. */
int rb3gpu_sh_merge_text(rb3gpu_t *h, const rb3gpu_comm_t *comm, int64_t *iv_bounds, int64_t len, const uint8_t *d_tprev, const uint64_t *d_tw_slice,
		int64_t n_chains, const int64_t *chain_tp, int commit, int64_t *n_rounds);
int rb3gpu_tprev_from_tw(rb3gpu_t *h, int64_t len, const uint64_t *d_tw, uint8_t *d_out);

/* ranks = threads of ONE process, one handle (device) each.  rb3gpu_group_create(world) once, rb3gpu_group_comm(g, rank, h, &comm)
 * by each rank's thread; rb3gpu_group_abort wakes every rank waiting in a collective (they return RB3GPU_ESTATE). */
typedef struct rb3gpu_group_s rb3gpu_group_t;
rb3gpu_group_t *rb3gpu_group_create(int world);
int rb3gpu_group_comm(rb3gpu_group_t *g, int rank, rb3gpu_t *h, rb3gpu_comm_t *comm);
void rb3gpu_group_abort(rb3gpu_group_t *g);
void rb3gpu_group_destroy(rb3gpu_group_t *g);

/* one PROCESS per GPU over RCCL.  Rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the others by whatever means the
 * launcher has (bench.py: torch.distributed broadcast; MPI; a file); every rank then creates its communicator on its handle's
 * device.  RB3GPU_EUNSUP: librccl.so could not be loaded. */
#define RB3GPU_RCCL_ID_BYTES 128
int rb3gpu_rccl_unique_id(char id[RB3GPU_RCCL_ID_BYTES]);
int rb3gpu_rccl_comm_create(rb3gpu_t *h, int rank, int world, const char id[RB3GPU_RCCL_ID_BYTES], rb3gpu_comm_t *comm);
void rb3gpu_rccl_comm_destroy(rb3gpu_comm_t *comm);

/* PEER ROUNDS for ranks that are PROCESSES of one node (bench.py --gpus N, torchrun: one process per GPU): wraps a communicator of world > 1 -- any of the above --
 * so that it offers stream_barrier / peer_export / peer_import: the receive buffers and counter tables are shared through HIP IPC memory handles
 * (hipIpcGetMemHandle / hipIpcOpenMemHandle, opened once per buffer); between two rounds every rank waits for its own stream and the processes meet at a spin
 * barrier in POSIX shared memory (streams of different processes cannot wait for each other on this runtime: hipStreamWaitEvent refuses events that came through
 * hipIpcOpenEventHandle) -- one host synchronisation per lock-step round, but no collective, no read-back, no copy.  COLLECTIVE: every rank calls it with its
 * handle and its communicator; it returns 0 on every rank (enabled everywhere) or RB3GPU_EUNSUP on every rank (some rank could not: the communicator is
 * left as it was).  rb3gpu_ipc_peer_disable undoes it (before the wrapped communicator is destroyed). */
int rb3gpu_ipc_peer_enable(rb3gpu_t *h, rb3gpu_comm_t *comm);
void rb3gpu_ipc_peer_disable(rb3gpu_comm_t *comm);

/* The interval-sharded index as ONE object for a single-process host program (`ropebwt3-amd build --gpus N --interval`): N handles,
 * one per device, a thread per handle (they live as long as the object), the thread-group communicator above between them.  Nothing of
 * the index, and of a batch nothing but one byte per symbol, is ever whole on one device:
 *   rb3gpu_shard_split   h0 holds a whole index (the first batch): it is cut into n intervals that hold about equal BYTES of the block array
 *                        (rb3gpu_balanced_bounds), an interval at a time (its symbols, 1 byte each, device to device); h0 keeps the first,
 *                        n - 1 new handles (options *opt, devices[1..n-1]; devices[0] must be h0's) get the others.  NULL: fewer symbols
 *                        than intervals, or a device / memory error.
 *   rb3gpu_shard_merge   one batch (text-order words on h0's device -- d_bwt is not read --, sentinel positions on the host): every rank
 *                        pulls the symbol-before array (1 byte per symbol) and ITS text range of the text-order words (8 bytes per symbol / n)
 *                        over its own xGMI link, all at once; then n threads run rb3gpu_sh_merge_text.
 *   rb3gpu_shard_export_runs / _run_words   the runs of the intervals in rank order, joined where they meet at a seam (the reference writes
 *                        its ropes one after the other and rld_enc joins them, fm-index.c:31-54, rld0.c:153-161): what the FMD / FMR /
 *                        plain writers take -- no gather.  rb3gpu_shard_get_acc: the cumulative symbol counts of the whole index.
 *   rb3gpu_shard_destroy the other handles destroyed, the object freed; h0 still holds interval 0.
 *   rb3gpu_shard_gather  the intervals put back together in h0 (plain symbols, the WHOLE index on h0's device: only for a caller that must
 *                        merge a batch the ordinary way), the other handles destroyed and the object freed.
 *   rb3gpu_shard_handle  the handle of interval i (statistics, tests); rb3gpu_shard_bounds copies the n + 1 bounds, returns n. */
typedef struct rb3gpu_shard_s rb3gpu_shard_t;
rb3gpu_shard_t *rb3gpu_shard_split(rb3gpu_t *h0, int n, const int *devices, const rb3gpu_opt_t *opt);
int rb3gpu_shard_merge(rb3gpu_shard_t *s, int64_t len, const uint8_t *d_bwt, const uint64_t *d_tw, int64_t n_chains, const int64_t *chain_tp, int64_t *n_rounds);
int rb3gpu_shard_gather(rb3gpu_shard_t *s);
int rb3gpu_shard_get_acc(const rb3gpu_shard_t *s, int64_t acc[RB3GPU_ASIZE + 1]);
int rb3gpu_shard_export_runs(rb3gpu_shard_t *s, rb3gpu_emit_f emit, void *data);
int rb3gpu_shard_export_run_words(rb3gpu_shard_t *s, rb3gpu_emit_words_f emit, void *data);
void rb3gpu_shard_destroy(rb3gpu_shard_t *s);
/* bounds moved to where equal shares of the block array's BYTES lie, if the largest interval holds more than pct per cent more than the mean (pct < 0:
 * always), every interval rebuilt from its new range on its own device; called by rb3gpu_shard_merge after every batch with pct = 25 (SURVEY 8(e);
 * RB3GPU_SHARD_REBALANCE_PCT overrides, -1 = never).  1: rebalanced, 0: not needed, < 0: error */
int rb3gpu_shard_rebalance(rb3gpu_shard_t *s, int pct);
rb3gpu_t *rb3gpu_shard_handle(rb3gpu_shard_t *s, int i);
int rb3gpu_shard_bounds(const rb3gpu_shard_t *s, int64_t *bounds);

/* k-mer counting over one or more indexes (`ropebwt3 kount`, main.c:333-423 of the reference): every k-mer over A C G T (no $, no N)
 * that occurs at least min_occ times in SOME index of hs[0..n_idx), with its count in every index (0 where it does not occur); all 4^k
 * k-mers for min_occ <= 0.  The trie is expanded one depth at a time on the device of hs[0], on its stream, after the pending work of
 * every handle; all handles must be on one device.  Results reach cb in the reference's output order, in chunks:
 *   kmers   n_out * k symbols, 1..4 = A C G T, k-mer r at kmers[r * k]
 *   counts  n_out * n_idx, the counts of k-mer r at counts[r * n_idx]
 * (host memory that is valid during the call only).  A nonzero return from cb stops the walk and is returned.  max_level_nodes caps the
 * nodes of one depth held at once (0: a share of the free device memory); a depth whose children exceed it is walked in slices, each to
 * the end, which changes nothing in the output.  RB3GPU_EINVAL for k < 1, n_idx < 1, a NULL callback or handles on different devices;
 * RB3GPU_ESTATE for a handle without an index.  st (may be NULL): ms_total wall time of the call, ms_expand the expansion kernel alone
 * (HIP events), n_nodes nodes expanded (rank pairs: n_nodes * n_idx), n_out k-mers, n_slices 1 + the times a depth was cut */
typedef int (*rb3gpu_kount_cb)(void *ud, int64_t n_out, int n_idx, int k, const uint8_t *kmers, const int64_t *counts);
typedef struct { double ms_total, ms_expand; int64_t n_nodes, n_out, n_slices; } rb3gpu_kount_stats_t;
int rb3gpu_kount(rb3gpu_t *const *hs, int n_idx, int k, int64_t min_occ, int64_t max_level_nodes, rb3gpu_kount_cb cb, void *ud, rb3gpu_kount_stats_t *st);

/* super-maximal exact matches of queries against the index (`ropebwt3 mem`, search.c and rb3_fmd_smem_TG, fm-index.c:483-528 of the reference):
 * the matches of query q = symbols[offsets[q], offsets[q + 1]) (nt6 codes 0..5, as rb3_char2nt6 makes them; n_query + 1 offsets, offsets[0] = 0) that are
 * at least min_len long, occur at least min_occ times (both strands) and lie in no other such match, as the reference finds them.  Every query is cut
 * into chunks of `chunk` symbols (<= 0: the default, 2048) that are searched independently, a walker of eight lanes each; the result does not depend on
 * `chunk`.  Records reach cb in the reference's output order -- queries in input order, matches by start -- in one piece per output slice (host memory
 * valid during the call only): st, en the match in the query, size its occurrences, x0 the first row of its interval.  A nonzero return from cb stops
 * the call and is returned.  The call holds the symbols, 8 bytes per walker and 36 bytes per query symbol of a slice (rb3gpu_tune "mem_slice", default 8 M
 * symbols) on the device; callers bound the symbols of a call (the CLI: -K).  RB3GPU_EINVAL for min_len < 1, min_occ < 1, a query longer than 2^31 - 1,
 * 2^31 queries or more, or a NULL callback; RB3GPU_ESTATE for a handle without an index or with one that does not hold both strands.  st (may be NULL):
 * ms_total wall time of the call, ms_walk the walkers' kernel alone (HIP events), n_steps extensions (a rank pair each), n_walkers, n_records, n_slices */
typedef struct { int64_t query, x0, size; int32_t st, en; } rb3gpu_mem_rec_t;
typedef int (*rb3gpu_mem_cb)(void *ud, int64_t n, const rb3gpu_mem_rec_t *recs);
typedef struct { double ms_total, ms_walk; int64_t n_steps, n_walkers, n_records, n_slices; } rb3gpu_mem_stats_t;
int rb3gpu_mem(rb3gpu_t *h, int64_t n_query, const int64_t *offsets, const uint8_t *symbols, int64_t min_len, int64_t min_occ, int64_t chunk,
		rb3gpu_mem_cb cb, void *ud, rb3gpu_mem_stats_t *st);

/* The sampled suffix array of the index in place, kept on the device for rb3gpu_locate / rb3gpu_mem_pos (8 bytes per string and per sample).
 *   rb3gpu_ssa_set   upload host arrays as rb3_ssa_restore reads them from a .ssa file (ssa.c:215-241): r2i[m], ssa[n_ssa]; RB3GPU_EINVAL unless m, n_ssa
 *                    and ms are what rb3gpu_ssa_dims gives for ssa_shift (m = acc[1]: the file belongs to this index)
 *   rb3gpu_ssa_keep  build it on the device (the kernels of rb3gpu_ssa_gen) and keep it there: nothing crosses to the host
 *   rb3gpu_ssa_drop  give it up; whatever replaces the index -- a merge, a load, a build -- does the same
 *   rb3gpu_ssa_info  its sample rate and number of samples; RB3GPU_ESTATE without one */
int rb3gpu_ssa_set(rb3gpu_t *h, int ssa_shift, int ms, int64_t m, int64_t n_ssa, const uint64_t *r2i, const uint64_t *ssa);
int rb3gpu_ssa_keep(rb3gpu_t *h, int ssa_shift);
int rb3gpu_ssa_drop(rb3gpu_t *h);
int rb3gpu_ssa_info(const rb3gpu_t *h, int *ssa_shift, int64_t *n_ssa);

/* where the rows of intervals lie in the indexed sequences (rb3_ssa_multi, ssa.c:158-192 of the reference, for a batch): for interval i = [lo[i], hi[i])
 * up to min(max_pos, hi[i] - lo[i]) pairs -- sid: string (sequence sid >> 1, reverse strand if sid & 1), pos: offset of the row's suffix in that string --,
 * the same pairs in the same order as the reference, whose traversal (sampled rows first, then the largest piece of a heap) also decides WHICH rows are
 * reported when max_pos is below the size.  lo[i] >= hi[i]: no pairs.  Pairs reach cb slice by slice (host memory valid during the call only): the n
 * intervals from i0 on, pair k of interval i0 + i at pos[off[i] + k], off[n] pairs in all.  A nonzero return from cb stops the call and is returned.
 * An octet of lanes per interval; its heap lies in LDS (rb3gpu_tune "locate_heap" entries, default 32, at most 80) and an interval that needs more is run
 * again with a heap in global memory, as many such intervals at a time as "locate_slice" bytes admit (default 256 MB).  RB3GPU_EINVAL for a non-empty
 * interval with lo < acc[1] or hi > acc[6] (rows of sentinels: the reference reads in front of its array there), max_pos < 0 or a NULL callback;
 * RB3GPU_ESTATE without an index or without a sampled suffix array; RB3GPU_EINTERNAL if a traversal ended with another number of pairs than it must.
 * st (may be NULL): ms_total wall time, ms_locate the locate kernels alone (HIP events), n_pops pieces taken off a heap (a rank pair each), n_intervals,
 * n_tier2 intervals run with a heap in global memory, max_heap most entries a heap held, n_pairs, n_slices */
typedef struct { int64_t sid, pos; } rb3gpu_pos_t;
typedef int (*rb3gpu_locate_cb)(void *ud, int64_t i0, int64_t n, const int64_t *off, const rb3gpu_pos_t *pos);
typedef struct { double ms_total, ms_locate; int64_t n_pops, n_intervals, n_tier2, max_heap, n_pairs, n_slices; } rb3gpu_locate_stats_t;
int rb3gpu_locate(rb3gpu_t *h, int64_t n, const int64_t *lo, const int64_t *hi, int64_t max_pos, rb3gpu_locate_cb cb, void *ud, rb3gpu_locate_stats_t *st);

/* rb3gpu_mem with the positions of every match (`mem -p`): up to max_pos >= 1 pairs per record, those of rb3gpu_locate on [x0, x0 + size).  The records of
 * a slice stay on the device between the search and the locate step; cb gets n records at a time with their pairs, pair k of record i at pos[off[i] + k].
 * RB3GPU_ESTATE without a sampled suffix array on the handle; everything else as rb3gpu_mem and rb3gpu_locate.  lst (may be NULL): the locate step */
typedef int (*rb3gpu_mem_pos_cb)(void *ud, int64_t n, const rb3gpu_mem_rec_t *recs, const int64_t *off, const rb3gpu_pos_t *pos);
int rb3gpu_mem_pos(rb3gpu_t *h, int64_t n_query, const int64_t *offsets, const uint8_t *symbols, int64_t min_len, int64_t min_occ, int64_t chunk, int64_t max_pos,
		rb3gpu_mem_pos_cb cb, void *ud, rb3gpu_mem_stats_t *st, rb3gpu_locate_stats_t *lst);

/* haplotype diversity of windows (`ropebwt3 hapdiv`, search.c and the BWA-SW dynamic program sw_core, bwa-sw.c:329-526 of the reference, in its end-to-end
 * mode on a linear query with end_len 1): window i = symbols[win_off[i], win_off[i] + k) (nt6 codes; the caller makes the windows of its queries, the CLI
 * every -w symbols) is aligned end to end against the index, n_best cells kept per row as the reference keeps them, ties included.  Its record: n_al, the
 * alignments of the last row that no better one contains, that end in a match or mismatch, score at least min_sc and lie within e2e_drop (< 0: off) of the
 * best; max_ed, the largest edit distance among them; n_hap[min(ed, 6)], the occurrences by edit distance.  A window without an alignment is nine zeros.
 * Records reach cb in window order, one piece per slice of rb3gpu_tune "hapdiv_slice" windows (default 64 K; host memory valid during the call only):
 * the n windows from i0 on.  A nonzero return from cb stops the call and is returned.  A wave per window; the call holds the symbols, 36 bytes per window
 * of a slice and, per window in flight (at most 2048, fewer where the free memory says so), 12 bytes per cell of (k + 1) * n_best and a candidate table
 * for the windows whose table outgrows LDS ("hapdiv_table" slots, default and at most 256).  RB3GPU_EINVAL for k < 1, n_best < 1, (k + 1) * n_best of
 * 2^32 or more, or a NULL callback; RB3GPU_ESTATE without an index or with one that does not hold both strands; RB3GPU_EINTERNAL if a window cannot be
 * represented (a table or stack beyond its capacity, a backtrack into a gap whose column was not kept: the reference stops on an assertion there) --
 * never a wrong record.  st (may be NULL): ms_total wall time, ms_dp the kernel alone (HIP events), n_ext extensions (a rank pair each), n_windows,
 * n_tier2 windows whose table went to global memory, n_slices */
typedef struct { int32_t n_best, min_sc, match, mis, gap_open, gap_ext, e2e_drop; } rb3gpu_hapdiv_opt_t;
typedef struct { int32_t n_al, max_ed, n_hap[7]; } rb3gpu_hapdiv_rec_t;
typedef int (*rb3gpu_hapdiv_cb)(void *ud, int64_t i0, int64_t n, const rb3gpu_hapdiv_rec_t *recs);
typedef struct { double ms_total, ms_dp; int64_t n_ext, n_windows, n_tier2, n_slices; } rb3gpu_hapdiv_stats_t;
int rb3gpu_hapdiv(rb3gpu_t *h, int64_t n_win, const int64_t *win_off, const uint8_t *symbols, int32_t k, const rb3gpu_hapdiv_opt_t *opt,
		rb3gpu_hapdiv_cb cb, void *ud, rb3gpu_hapdiv_stats_t *st);

/* end-to-end alignments of whole queries with their alignment and positions (`ropebwt3 sw -e`, `--all-e2e`, `-g`: rb3_sw, bwa-sw.c:532-560 of the reference, in
 * its end-to-end mode): query q = symbols[offsets[q], offsets[q + 1]) (nt6 codes) is aligned end to end against the index by the dynamic program of
 * rb3gpu_hapdiv, but mismatches and gaps are allowed only once end_len symbols are aligned (-k; -e sets 1).  Its hits are the cells of the last row that
 * no better one contains, that end in a match or mismatch, score at least min_sc and lie within e2e_drop (< 0: off) of the best, in the reference's
 * order.  A hit: its interval [lo, hi), its score, the symbols of the query (qlen) and of the index (rlen) it spans, and its alignment, n_steps bytes
 * from steps[step_off]: one byte per step from query position 0 on, (op << 4 | base) with op 0 `=`, 1 `X`, 2 `I`, 3 `D` and base 1..5 the symbol of the
 * index at that step (an `I` carries the base of the cell it leaves; `=` is "the base is the query's symbol", so N against N is `=`).  cigar, cs, rs,
 * matching and block length are functions of the bytes.  max_pos >= 0: positions through the sampled suffix array of the handle (rb3gpu_ssa_set /
 * rb3gpu_ssa_keep), as rb3_sw asks for them: hit k of a query gets n_pos = min(rest > 0 ? rest : 1, hi - lo) pairs from pos[pos_off], rest = max_pos at
 * the first hit and less n_pos after each -- so max_pos 0 is one position per hit.  The intervals go from the alignment step to the locate step on
 * the device; every hit is located at the largest cap a hit can have, max(max_pos, 1), and cut: the traversal's pairs at a smaller cap are a prefix of
 * those at a larger.  max_pos < 0: no positions (--no-ssa).  cb gets the queries slice by slice in query order (host memory valid during the call only):
 * the nq queries from q0 on, n_hit[i] hits of query q0 + i, their records one after another in hits[].  A nonzero return stops the call and is returned.
 * A slice is at most rb3gpu_tune "sw_slice" queries (default 16 K), fewer where its backtrack matrices, 12 bytes per cell of (len + 1) * n_best for
 * every query of the slice, would not fit; "sw_table" as "hapdiv_table".  A query of length 0 has no hits.  RB3GPU_EINVAL for n_best < 1, end_len < 1,
 * (len + 1) * n_best of 2^32 or more for any query, or a NULL callback; RB3GPU_ESTATE without an index, with one that does not hold both strands, or
 * when positions are asked for without a sampled suffix array; RB3GPU_EINTERNAL if a query cannot be represented (as rb3gpu_hapdiv) -- never a wrong
 * record.  st (may be NULL): ms_total wall time, ms_dp the rows and the counting walk, ms_backtrack the writing walk (HIP events), n_ext extensions,
 * n_hits, n_steps, n_tier2 queries whose table went to global memory, n_slices; lst (may be NULL): the locate step */
typedef struct { int32_t n_best, min_sc, match, mis, gap_open, gap_ext, e2e_drop, end_len; int64_t max_pos; } rb3gpu_sw_opt_t;
typedef struct { int64_t lo, hi; int32_t score, qlen, rlen, n_steps; int64_t step_off, pos_off, n_pos; } rb3gpu_sw_hit_t;
typedef int (*rb3gpu_sw_cb)(void *ud, int64_t q0, int64_t nq, const int32_t *n_hit, const rb3gpu_sw_hit_t *hits, const uint8_t *steps, const rb3gpu_pos_t *pos);
typedef struct { double ms_total, ms_dp, ms_backtrack; int64_t n_ext, n_hits, n_steps, n_tier2, n_slices; } rb3gpu_sw_stats_t;
int rb3gpu_sw_e2e(rb3gpu_t *h, int64_t n_query, const int64_t *offsets, const uint8_t *symbols, const rb3gpu_sw_opt_t *opt, rb3gpu_sw_cb cb, void *ud,
		rb3gpu_sw_stats_t *st, rb3gpu_locate_stats_t *lst);

/* local alignment of whole queries over their DAWG (`ropebwt3 sw` in its default mode: rb3_sw, bwa-sw.c:532-560, with rb3_dawg_gen): the rows of the dynamic
 * program of rb3gpu_sw_e2e are the nodes of the query's directed acyclic word graph, which the caller builds (rb3h_dawg_batch of the host library; a graph is a
 * function of the query alone).  Query q owns the nodes [node_off[q], node_off[q + 1]) (n_query + 1 offsets, node_off[0] = 0; at least the root, node 0 of the
 * query); node g of the batch carries symbol node_sym[g] (1..4) and has the predecessors pre[pre_off[g], pre_off[g + 1]) (one offset more than there are nodes,
 * pre_off[0] = 0), each a node number WITHIN the query and smaller than the node's own, in the order candidates arrive from them.  offsets are those of the
 * queries' symbols as for rb3gpu_sw_e2e (symbols may be NULL: the nodes carry what is aligned).  A query has at most ONE hit: column 0 of the first node whose
 * best score is above that of every earlier node, if that score reaches min_sc; its record, step bytes and positions are those of rb3gpu_sw_e2e (`=` is "the
 * base is the node's symbol": the graph counts an N of the query as A), qlen the symbols of the query it spans, and hit_node[q] (n_query entries, written
 * before the callback sees the slice of q) the node it ends at, -1 without a hit: the caller's qoff0 and n_qoff of that node say where on the query.
 * e2e_drop plays no part.  Positions: one hit, so n_pos = min(max(max_pos, 1), hi - lo).  A slice is at most rb3gpu_tune "sw_slice" queries, fewer where the
 * cells of all nodes (56 bytes per cell of n_node * n_best) and their backtrack words (12) would not fit in a quarter of the free memory; one query at least.
 * A node's cells are extended once for every successor.  RB3GPU_EINVAL for a graph that is not one (offsets that decrease, a predecessor that is not an
 * earlier node, more than 2 len + 2 nodes), n_node * n_best of 2^32 or more, and what rb3gpu_sw_e2e refuses; RB3GPU_ESTATE as there; RB3GPU_EINTERNAL if a
 * query cannot be represented -- never a wrong record.  st (may be NULL): sw as rb3gpu_sw_e2e, n_nodes and n_edges of the batch */
typedef struct { rb3gpu_sw_stats_t sw; int64_t n_nodes, n_edges; } rb3gpu_swl_stats_t;
int rb3gpu_sw_local(rb3gpu_t *h, int64_t n_query, const int64_t *offsets, const uint8_t *symbols, const int64_t *node_off, const uint8_t *node_sym, const int64_t *pre_off,
		const int32_t *pre, const rb3gpu_sw_opt_t *opt, rb3gpu_sw_cb cb, void *ud, int32_t *hit_node, rb3gpu_swl_stats_t *st, rb3gpu_locate_stats_t *lst);

/* the longest suffix of every query that occurs in the index, and how often (`ropebwt3 suffix`, main.c:167-217 of the reference: the one-sided backward
 * extension rb3_fmi_extend1, fm-index.h:140-147, from the last symbol of the query leftwards until the interval is empty): query q = symbols[offsets[q],
 * offsets[q + 1]) (nt6 codes 0..5 as for rb3gpu_mem; n_query + 1 offsets, offsets[0] = 0) gets out[q]: start, where that suffix begins in the query (0: the whole
 * query occurs; the query's length: not even its last symbol does), and size, its occurrences (0 where start is the length).  A query of no symbols is
 * (0, 0).  Any index serves, one strand or both.  An octet of lanes per query, a rank pair of one symbol per step; rb3gpu_tune "suffix_slice" queries per
 * launch (default 4 M).  The call holds the symbols, 8 bytes per query and 16 per query of a slice on the device.  RB3GPU_EINVAL for a query of 2^31
 * symbols or more (it is not walked); RB3GPU_ESTATE for a handle without an index.  st (may be NULL): ms_total wall time of the call, ms_walk the kernel
 * alone (HIP events), n_steps extensions (a rank pair each), n_queries, n_symbols, n_slices */
typedef struct { int64_t start, size; } rb3gpu_suffix_rec_t;
typedef struct { double ms_total, ms_walk; int64_t n_queries, n_symbols, n_steps, n_slices; } rb3gpu_suffix_stats_t;
int rb3gpu_suffix(rb3gpu_t *h, int64_t n_query, const int64_t *offsets, const uint8_t *symbols, rb3gpu_suffix_rec_t *out, rb3gpu_suffix_stats_t *st);

/* does a query hold a seed: a stretch of at least min_len symbols that occurs in the index (rb3_fmd_smem_present, fm-index.c:483-498 and 530-538 of the reference,
 * the test behind `sw -j`, bwa-sw.c:536-539)?  Query q as for rb3gpu_suffix gets present[q] = 1 if it does and 0 if not; a query of fewer than min_len symbols, an
 * empty one among them, gets 0.  All six symbol codes are extended as they come: an N of the query matches an indexed N.  Any index serves, one strand or both.
 * A window of min_len symbols is walked from its last symbol to its first with the step of rb3gpu_suffix; where the interval empties at symbol i the next window
 * starts at i + 1, as in the reference.  A query is cut into walkers of `chunk` window starts each (0: rb3gpu_tune "seed_chunk", default 2048), an octet of
 * lanes per walker; the answer is the OR of the walkers' and does not depend on chunk.  rb3gpu_tune "seed_slice": walkers per launch
 * (default 1 M).  The call holds the symbols, 9 bytes per query and 16 per walker of a slice on the device.  RB3GPU_EINVAL for min_len < 2 (at 1 the reference's
 * loop answers 1 for any query that is not empty, whatever the index holds) and for a query of 2^31 symbols or more; RB3GPU_ESTATE for a handle without an index.
 * st (may be NULL): ms_total wall time of the call, ms_walk the kernel alone (HIP events), n_steps extensions (a rank pair each; with more than one walker
 * per query it depends on which walker finds a seed first), n_queries, n_present, n_walkers, n_slices */
typedef struct { double ms_total, ms_walk; int64_t n_queries, n_present, n_walkers, n_steps, n_slices; } rb3gpu_seed_stats_t;
int rb3gpu_seed_present(rb3gpu_t *h, int64_t n_query, const int64_t *offsets, const uint8_t *symbols, int64_t min_len, int64_t chunk, uint8_t *present, rb3gpu_seed_stats_t *st);

/* the indexed strings spelled out (`ropebwt3 get`, rb3_fmi_retrieve, fm-index.c:552-567 of the reference): from row rows[i] the LF walk until the row whose
 * symbol is the sentinel; the symbols met, reversed, are the string in front of the suffix of that row -- for a sentinel's row k < acc[1] the whole of
 * string k -- and the row the walk ends at is what rb3_fmi_retrieve returns.  A row outside [0, acc[6]) has no string and end row -1; such rows never
 * reach the device.  The answers reach cb in the order asked, duplicates included, a slice at a time (host memory valid during the call only): the n rows
 * from i0 on, their end rows, and the string of row i0 + i at symbols[off[i], off[i + 1]) (nt6 codes, text order; n + 1 offsets, off[0] = 0).  A nonzero
 * return from cb stops the call and is returned.  An octet of lanes per row; the walk is made twice -- once for the lengths, once, after an exclusive
 * scan of the lengths of a slice, to write the symbols where they belong -- and a slice is as many consecutive rows as rb3gpu_tune "get_slice" symbols
 * admit (default 64 M; a longer string is a slice of its own), so the output held on the device is bounded by that budget or the longest string, not by
 * the request.  One string is one dependent chain of LF steps: a single long string runs at the latency of a rank.  RB3GPU_EINVAL for a NULL callback;
 * RB3GPU_ESTATE without an index; RB3GPU_EUNSUP for a string of 2^32 symbols or more; RB3GPU_EINTERNAL for a walk that does not end (not an index).
 * st (may be NULL): ms_total wall time, ms_count and ms_emit the two walks (HIP events), n_steps LF steps of both, n_rows, n_symbols, n_slices */
typedef int (*rb3gpu_retrieve_cb)(void *ud, int64_t i0, int64_t n, const int64_t *end_row, const int64_t *off, const uint8_t *symbols);
typedef struct { double ms_total, ms_count, ms_emit; int64_t n_rows, n_symbols, n_steps, n_slices; } rb3gpu_retrieve_stats_t;
int rb3gpu_retrieve(rb3gpu_t *h, int64_t n, const int64_t *rows, rb3gpu_retrieve_cb cb, void *ud, rb3gpu_retrieve_stats_t *st);

/* rb3gpu_retrieve in pieces: the same answers through the same callback, cut into the same slices by "get_slice", but no walker follows more
 * than one piece of a string.  The rows of the index are cut by splitters -- the acc[1] sentinel rows and every row k >= acc[1] with (k - acc[1]) a multiple of
 * 2^S, S = rb3gpu_tune "get_piece" (default 8) -- and the call walks the WHOLE index once, every piece from its splitter to the next at the same time, joins the
 * pieces by pointer jumping, sorts them by (string, distance from its start) and then writes every slice of rows with all of the pieces of its strings side by
 * side.  It pays where a string is long or much of the index is asked for; for a few short rows rb3gpu_retrieve does less.  n < 0 with rows NULL: all the
 * strings, rows 0 .. acc[1] - 1 (the callback's i0 then counts strings).  The call holds about 48 bytes per piece (acc[1] + (acc[6] - acc[1]) / 2^S pieces),
 * 8 per string and 60 per row asked for on the device besides the output of a slice; nothing is kept between calls.  Errors as rb3gpu_retrieve; RB3GPU_EUNSUP
 * also for acc[1] >= 2^31 or 2^32 pieces or more.  st (may be NULL): ms_total wall time; ms_pieces, ms_join, ms_sort, ms_emit the phases (HIP events);
 * n_pieces; max_piece_steps the longest piece; n_steps the LF steps of the pieces, of the rows down to their first splitter, and of the writing walks */
typedef struct { double ms_total, ms_pieces, ms_join, ms_sort, ms_emit; int64_t n_rows, n_symbols, n_slices, n_pieces, n_steps, max_piece_steps; } rb3gpu_pieces_stats_t;
int rb3gpu_retrieve_pieces(rb3gpu_t *h, int64_t n, const int64_t *rows, rb3gpu_retrieve_cb cb, void *ud, rb3gpu_pieces_stats_t *st);

/* strings taken OUT of the index the handle holds (no counterpart in the reference): the inverse of a merge.  rows[i] are string numbers in
 * [0, acc[1]) -- there is none of rb3gpu_retrieve's "row inside a string" --, duplicates collapse.  String r occupies the rows the LF walk from row r stands
 * on, the row whose symbol is the sentinel included; those rows are marked in a bitmap of one bit per row, counted, and the chunked builder of
 * rb3gpu_from_fmd_words ("load_chunk") is fed with the rows that stay.  pieces == 0: one octet of lanes walks one string (a dependent chain of len + 1 LF
 * steps); pieces != 0: the whole index is walked once in pieces as in rb3gpu_retrieve_pieces ("get_piece") and the pieces of the strings asked for mark their
 * rows side by side -- for long strings.  The order of the strings that stay (rb3gpu_get_order) is what it was.  Before anything is replaced the marked rows are
 * checked: as many as the strings' len + 1 sum to, one sentinel per string.  On success the handle holds the new index (acc included; a sampled suffix array
 * kept on the handle is dropped); on ANY failure it still holds the old one.  RB3GPU_EINVAL for a row outside [0, acc[1]) and for a request that would leave no
 * string (n == 0 succeeds and changes nothing); RB3GPU_ESTATE without an index; RB3GPU_EUNSUP with pieces for acc[1] >= 2^31, 2^32 pieces or more, or a string of
 * 2^32 symbols or more; RB3GPU_EINTERNAL if the check fails.  Device memory beside the two indexes: the bitmap (acc[6] / 8 bytes), 12 bytes per 8192 rows, the
 * builder's chunk, and with pieces 32 bytes per piece and 9 per string.  st (may be NULL): ms_total wall time, ms_mark the walks and ms_build the rebuild (HIP
 * events), n_strings distinct strings, n_rows rows deleted, n_steps LF steps, n_pieces and max_piece_steps (pieces only), removed[c] deleted symbols per letter */
typedef struct { double ms_total, ms_mark, ms_build; int64_t n_strings, n_rows, n_steps, n_pieces, max_piece_steps, removed[6]; } rb3gpu_remove_stats_t;
int rb3gpu_remove(rb3gpu_t *h, int64_t n, const int64_t *rows, int pieces, rb3gpu_remove_stats_t *st);

/* which strings of the index are redundant (no counterpart in the reference): exact copies of another string, and strings that lie wholly inside a
 * longer one.  ALL acc[1] strings are judged.  From row r the LF walk of rb3gpu_retrieve spells string r from its last symbol to its first, and the symbols read
 * drive two backward searches of rb3gpu_suffix: `any` from all the rows and `suf` from the sentinels' rows.  Where the walk reads the sentinel, rec[r] (may be NULL;
 * acc[1] records) is occ = |any|, the places string r occurs at anywhere in the index, itself included; cls = the sentinels in front of suf, the same for all copies
 * of a string and for no other string; copies = the sentinels inside suf, the strings that ARE string r.  A walk whose `any` has come down to one row ends there --
 * the string is unique -- with (1, 1, -1): a unique read costs about log4(acc[6]) steps, not its length (rb3gpu_tune "dedup_early" 0: every walk goes down to its
 * sentinel; the kinds are the same).  A unit is a row; with pair != 0 unit u is rows 2u and 2u + 1 of an index of both strands in input order, judged on row 2u,
 * and every row enters the class table as unit r >> 1: a copy of a reverse complement is a copy, a palindrome keeps itself, and a sequence inside another one's
 * reverse complement is inside a string of the index.  kind[u] (acc[1] >> pair bytes): 'C' contained, occ > copies (never with dup_only != 0); else 'D' duplicate,
 * copies > 1 and u is not the smallest unit of its class; else 'K'.  keeper[u]: the smallest unit of u's class, u itself where copies == 1.  Symbols are compared
 * as indexed (an N equals an N); a string of no symbols occurs at every row.  An octet of lanes per string; a step is the two dependent trips of a rank (directory word, slot) with five requests in flight in each;
 * rb3gpu_tune "dedup_slice" strings per launch (default 4 M).  One string is one dependent chain: a long string that is NOT unique near its end runs at the latency
 * of a rank.  The call holds 28 bytes per string and 9 per unit on the device; nothing is kept on the handle and the index is not changed.  RB3GPU_ESTATE without an
 * index; RB3GPU_EINVAL for pair on an odd acc[1] and for a unit whose two rows disagree in occ or copies (not an index of both strands in input order);
 * RB3GPU_EUNSUP for acc[1] >= 2^31 and for a string of 2^31 symbols or more; RB3GPU_EINTERNAL for a walk that does not end and for a walk whose own last row is not
 * among the copies it counted.  st (may be NULL): ms_total wall time, ms_walk the walks alone (HIP events), n_strings, n_steps, n_early walks ended early, n_dup and
 * n_contained units, n_classes classes of more than one string, n_slices */
typedef struct { int64_t occ, copies, cls; } rb3gpu_dedup_rec_t;
typedef struct { double ms_total, ms_walk; int64_t n_strings, n_steps, n_early, n_dup, n_contained, n_classes, n_slices; } rb3gpu_dedup_stats_t;
int rb3gpu_dedup(rb3gpu_t *h, int pair, int dup_only, uint8_t *kind, int64_t *keeper, rb3gpu_dedup_rec_t *rec, rb3gpu_dedup_stats_t *st);

/* which strings of the index overlap, end to start, and by how much (no counterpart in the reference): the record (a, b, len, len_b) says that the last
 * len symbols of string a are the first len symbols of string b, min_len <= len < the length of a, len <= len_b = the length of b.  ALL acc[1] strings are walked.
 * From row a the LF walk of rb3gpu_retrieve spells string a from its last symbol to its first, and the symbols read drive the backward search of rb3gpu_suffix from
 * all the rows: after d symbols the interval holds every row whose suffix starts with the last d symbols of a, and the sentinels among its BWT symbols are the
 * strings that START with them -- occ0(hi) - occ0(lo) of them, the group of depth d, named by the sentinel ranks in between.  The pass that reads a's own sentinel is
 * the whole string and no overlap.  A group of more than max_hits partners is left out as a whole (0: none is).  A walk whose interval has come down to one row ends
 * there: that row is its own suffix, and only the whole string is left (rb3gpu_tune "ovl_early" 0: every walk goes down to its sentinel; the records are the same).
 * Nothing is filtered: a == b is a self-overlap, and len == len_b a partner that is wholly the overlap (what rb3gpu_dedup calls contained); on an index of both
 * strands the four orientations are there, each overlap from both of its sides.  Symbols are compared as indexed (an N equals an N).  Three stages: COUNT, an octet
 * of lanes per string, three rank loads in flight per pass, rb3gpu_tune "ovl_strings" strings per launch (default 4 M), gives the records of every string and the
 * largest depth that has any; then, unless there is no record (and len is NULL), the lengths and end rows of all strings by the counting walk of rb3gpu_retrieve and
 * the table from sentinel rank to string; then EMIT walks the strings that have records again, to that depth only.  The records reach cb in slices (host memory
 * valid during the call only) of consecutive strings whose records sum to at most rb3gpu_tune "ovl_slice" (default 16 M records; a string with more is a slice of
 * its own), ordered by a ascending, then len descending, then sentinel rank ascending -- the index's own order of the partners.  len (may be NULL; acc[1] entries)
 * receives the length of every string before the first callback.  A nonzero return from cb stops the call and is returned; without a record cb is never called.
 * The call holds 48 bytes per string and the records of a slice on the device; nothing is kept on the handle and the index is not changed.  RB3GPU_ESTATE without an
 * index; RB3GPU_EINVAL for min_len < 1, max_hits < 0 and a NULL callback; RB3GPU_EUNSUP for acc[1] >= 2^31, a string of 2^31 symbols or more and a string with 2^31
 * records or more; RB3GPU_EINTERNAL for a walk that does not end, a rank table that is not written exactly once per entry and a stored count that differs from the
 * counted one.  st (may be NULL): ms_total wall time; ms_count, ms_who, ms_emit the stages (HIP events); n_steps_count and n_steps_emit passes of the two walks;
 * n_early walks ended early; n_hits records; n_groups kept groups; n_capped_groups and n_capped_hits the groups over max_hits and their partners; n_emitters strings
 * with records; n_slices callbacks */
typedef struct { int32_t a, b, len, len_b; } rb3gpu_overlap_rec_t;
typedef struct { double ms_total, ms_count, ms_who, ms_emit;
                 int64_t n_strings, n_steps_count, n_steps_emit, n_early, n_hits, n_groups, n_capped_groups, n_capped_hits, n_emitters, n_slices; } rb3gpu_overlap_stats_t;
typedef int (*rb3gpu_overlap_cb)(void *ud, int64_t n, const rb3gpu_overlap_rec_t *recs);
int rb3gpu_overlap(rb3gpu_t *h, int64_t min_len, int64_t max_hits, int64_t *len, rb3gpu_overlap_cb cb, void *ud, rb3gpu_overlap_stats_t *st);

/* the irreducible overlaps: the records of rb3gpu_overlap for the same index, min_len and max_hits -- the set R -- without those that two longer ones imply (the
 * transitive reduction of Myers' string graph; no counterpart in the reference).  (a, b, o) is reducible iff some (a, c, o_c) of R has o_c > o and
 * len(c) > o_c and (c, b, len(c) - o_c + o) is in R: c overlaps a by more, reaches beyond the end of a, and what it adds there is a prefix of what b adds.  Nothing else
 * is filtered: c == a and c == b count, a witness counts whether it is itself reducible or not (the answer does not depend on any order), copies of a witness are all
 * kept and copies of a reducible partner all reduced.  The kept records are a subsequence of rb3gpu_overlap's in its order; the deepest group of every string is kept
 * whole, so the strings with kept records are the strings with records; with max_hits the rule is applied to the capped set.  The record type, the callback, the
 * slices (consecutive strings whose KEPT records sum to at most "ovl_slice") and len are rb3gpu_overlap's.  Stages: COUNT, the lengths, the rank table and the scan
 * as there; EMIT of ALL the records into one resident array, "ovl_strings" strings per launch; REDUCE, an octet of lanes per record, the lanes over the records of
 * the same string with a deeper overlap, each with one binary search in the list of its witness, rb3gpu_tune "ovl_reduce_strings" strings per launch (default 4 M);
 * COMPACT, a scan of the keep flags and an order-preserving scatter per slice.  The call holds 28 bytes per record (the record, its flag, its scanned position) and
 * 4 bytes per string more than rb3gpu_overlap on the device, and nothing on the handle.  More records than rb3gpu_tune "ovl_resident" (0, the default: no limit but
 * the allocation) is RB3GPU_EUNSUP, an allocation that fails RB3GPU_ENOMEM, both before the first callback: use a larger min_len, a max_hits, or rb3gpu_overlap.
 * Other codes as rb3gpu_overlap, and RB3GPU_EINTERNAL also for a string with records and none kept and for kept + reduced != n_hits.  st (may be NULL): ms_reduce
 * and ms_compact the two new stages (HIP events; ms_emit includes the inverse rank table); n_kept the records delivered; resident_bytes what REDUCE and COMPACT held
 * on the device; the rest as in rb3gpu_overlap_stats_t */
typedef struct { double ms_total, ms_count, ms_who, ms_emit, ms_reduce, ms_compact;
                 int64_t n_strings, n_hits, n_kept, n_groups, n_capped_groups, n_capped_hits, n_emitters, n_slices, resident_bytes; } rb3gpu_reduce_stats_t;
int rb3gpu_overlap_reduced(rb3gpu_t *h, int64_t min_len, int64_t max_hits, int64_t *len, rb3gpu_overlap_cb cb, void *ud, rb3gpu_reduce_stats_t *st);

/* the unitigs: the paths of the string graph along which nothing branches, each spelled as one sequence (no counterpart in the reference).  K is what
 * rb3gpu_overlap_reduced delivers for the same min_len and max_hits, in its order; the vertices are the strings.  A record (a, b, o) of K is SIMPLE iff it is the only
 * record of K out of a, the only one into b (records are counted, not partners) and a != b; the simple records join the vertices into disjoint paths and cycles.  A
 * unitig is a path from its head to its tail -- a vertex without simple records is a unitig of one member -- or a cycle, cut in front of its smallest row: that row is
 * the head and spells its whole string, and the overlap that closes the circle is the unitig's `circ` (> 0; 0 for a path).  Member v starts at off(v) in its unitig,
 * off(head) = 0 and off(next) = off(v) + len(v) - o_in(next); its symbols [o_in, len) are the ones it adds, so the unitig's length is the head's plus the sum of
 * len - o_in over the others.  Unitigs are numbered by ascending head.  The LINKS are the records of K that are not simple, in K's order: each goes from a tail to a head.
 * pair != 0 (an index of both strands in input order: row v ^ 1 is the other strand of row v): the graph must be strand-symmetric, next[next[v] ^ 1] == v ^ 1 wherever
 * v has a next -- n_asym counts the vertices where it is not, and with n_asym > 0 the call is RB3GPU_EUNSUP before any callback (contained sequences or max_hits do
 * that: rb3gpu_dedup and rb3gpu_remove first, max_hits 0, or pair 0).  Chains then come as mirror pairs and one of each is delivered: a path iff head <= tail ^ 1 (equal:
 * the path is its own mirror image), a cycle iff its head is even, a link iff a <= b ^ 1; an end of a link on a chain that is not delivered names the mirror chain's
 * unitig with from_rev / to_rev = 1.  pair == 0: everything is delivered, every orientation 0.
 * cb is called once per slice of consecutive unitigs whose lengths sum to at most rb3gpu_tune "utg_slice" symbols (a longer one alone): unitigs [u0, u0 + n), their
 * members one unitig after the other by rank, and the symbols (nt6, text order) of unitig u0 + i at symbols[off[i], off[i + 1]).  lcb (may be NULL) is called once
 * after the last slice, with all the links, if there are any.  Host memory is valid during the callback only; a callback that returns non-zero ends the call with
 * that value.  The records stay on the device from the reduction to the links: the ceiling "ovl_resident" and the codes are rb3gpu_overlap_reduced's.  RB3GPU_EINVAL
 * also for pair on an odd number of strings; RB3GPU_EINTERNAL also where the members delivered, the symbols written, the steps walked and the scanned totals differ.
 * st (may be NULL): ms_reduce the stages of rb3gpu_overlap_reduced, ms_graph, ms_rank, ms_emit (HIP events); n_simple the simple records; n_rounds the rounds of
 * pointer jumping; n_unitigs, n_members, n_symbols, n_cycles, max_members of what is delivered; n_steps_emit == n_symbols: one LF step per symbol of the output */
typedef struct { int32_t head, tail, members, circ; int64_t len; } rb3gpu_unitig_t;
typedef struct { int32_t row, o_in; int64_t off; } rb3gpu_unitig_member_t;
typedef struct { int32_t from, to, len; uint8_t from_rev, to_rev, pad[2]; } rb3gpu_unitig_link_t;
typedef struct { double ms_total, ms_reduce, ms_graph, ms_rank, ms_emit;
                 int64_t n_strings, n_kept, n_simple, n_unitigs, n_members, n_symbols, n_steps_emit, n_cycles, n_asym, n_links, n_rounds, max_members, n_slices,
                         resident_bytes; } rb3gpu_unitig_stats_t;
typedef int (*rb3gpu_unitig_cb)(void *ud, int64_t u0, int64_t n, const rb3gpu_unitig_t *utg, const rb3gpu_unitig_member_t *mem, const int64_t *off, const uint8_t *symbols);
typedef int (*rb3gpu_unitig_link_cb)(void *ud, int64_t n, const rb3gpu_unitig_link_t *links);
int rb3gpu_unitigs(rb3gpu_t *h, int64_t min_len, int64_t max_hits, int pair, rb3gpu_unitig_cb cb, void *ud, rb3gpu_unitig_link_cb lcb, rb3gpu_unitig_stats_t *st);

/* regions of the indexed strings, read through the sampled suffix array the handle holds (rb3gpu_ssa_set / rb3gpu_ssa_keep; no counterpart in the reference;
 * DESIGN.md 7m): random access into the indexed text.  A region is (row r, beg, end): the symbols [beg, end) of string r, the string rb3gpu_retrieve spells for
 * row r < acc[1]; 0-based, end exclusive; valid iff 0 <= r < acc[1] and 0 <= beg < end <= the length of the string.  Sample x of the sampled suffix array says that
 * row acc[1] + (x << ssa_shift) is the suffix of string s at text offset o; sorted by (s, o) -- a table of 4 bytes per sample, made by the first call and kept with
 * the sampled suffix array until that is dropped or replaced -- the samples are an index from text coordinates to rows.  A region is read by its anchor, the sample
 * of r with the smallest offset >= end (sentinel row r, at the length of the string, where there is none), and by every sample of r with beg < o < end, each an
 * octet of lanes that walks LF down to beg or to the row of the next sample: o_anchor - beg steps per region, no chain longer than one gap between samples
 * whatever the length of the string, nothing outside the region touched.  A region without an anchor needs the length of its string: it is measured by a walk
 * from row r to the first sample (or the sentinel), and only such regions are.  ALL regions are validated before the callback sees anything.  The answers
 * reach cb in the order asked, duplicates and overlaps answered independently, a slice at a time (host memory valid during the call only): the n regions from i0
 * on, region i0 + i at symbols[off[i], off[i + 1]) (nt6 codes, text order; n + 1 offsets, off[0] = 0); a slice is as many consecutive regions as
 * rb3gpu_tune "fetch_slice" symbols admit (default 64 M; a longer region is a slice of its own).  A nonzero return from cb stops the call and is returned.
 * n == 0 succeeds.  RB3GPU_EINVAL for a NULL callback and for an invalid region: *bad (may be NULL; -1 otherwise) receives the index of the first one, and
 * nothing has reached the callback; RB3GPU_ESTATE without an index or without a sampled suffix array on the handle; RB3GPU_EUNSUP for 2^32 - 1 samples or more;
 * RB3GPU_EINTERNAL, and no output for the slice, where a walker lands on a sample that does not say (its string, its offset) or reads the start of its string
 * above beg: the sampled suffix array is not of this index.  The handle is unchanged by any outcome, apart from the table.  The call holds 68 bytes per region
 * and the output of a slice on the device; while the table is made, 24 bytes per sample more.  st (may be NULL): ms_total wall time; ms_table (0 unless this call
 * made the table), ms_plan (plan and measuring), ms_walk the phases (HIP events); n_walkers; n_measured regions without an anchor; n_steps LF steps of the
 * measuring walks and of the walkers; max_walk_steps the longest walk of a walker */
typedef struct { int64_t row, beg, end; } rb3gpu_region_t;
typedef int (*rb3gpu_fetch_cb)(void *ud, int64_t i0, int64_t n, const int64_t *off, const uint8_t *symbols); /* nt6 codes, text order; n + 1 offsets */
typedef struct { double ms_total, ms_table, ms_plan, ms_walk; int64_t n_regions, n_symbols, n_walkers, n_measured, n_steps, max_walk_steps, n_slices; } rb3gpu_fetch_stats_t;
int rb3gpu_fetch(rb3gpu_t *h, int64_t n, const rb3gpu_region_t *reg, int64_t *bad, rb3gpu_fetch_cb cb, void *ud, rb3gpu_fetch_stats_t *st);

/* the HIP device and stream of a handle (for communicators implemented outside the library) */
int rb3gpu_device_of(const rb3gpu_t *h);
void *rb3gpu_stream_of(const rb3gpu_t *h);
/* wait for a stream handed to a communicator's all_to_all (a communicator that moves the send regions with anything that is not ordered behind that stream -- the
 * runtime's synchronous copies, a library on another stream -- calls this first: the engine's streams are non-blocking) */
int rb3gpu_stream_sync(void *stream);

/* Diagnostic switches of a handle (no reference analogue; none is needed in normal use).  Each key is also read ONCE from
 * the environment variable RB3GPU_<KEY> when the handle is created; the merge path itself never calls getenv().
 *   "tent" 0/1, "staged" 0/1, "group_rebuild" 0/1, "window_rebuild" 0/1, "reb_force" 0/1/-1 (the run-space rebuild always / never), "octs" 1..8, "blkmul", "blkcap", "ssa_split" 4..20,
 *   "lf_check" n (verify the LF relation of every n-th batch row against the index after each merge; default 4096, 0 = off)
 *   "tent_q" 1/2/4/8 (width of the drop-out masks in units of 256 bits; 0 = follows what the walkers report), "trec" 0/1/-1 (records of a
 *   text-order walk in text order: never / always / where the index does not fit the caches), "copy_walkers" 0/1, "b2_split" S (splitter
 *   spacing 2^S of the walker list the engine makes for the BWT-only entry points; -1 = by the size of the batch), "abs_limit" N (indexes
 *   of fewer than N symbols carry the LF base in their slot headers; at most 2^32, only before an index exists: RB3GPU_ESTATE after);
 *   "mem_slice" N (query symbols per output slice of rb3gpu_mem; 0 = 8 M);
 *   "hapdiv_slice" N (windows per launch of rb3gpu_hapdiv; 0 = 64 K), "hapdiv_table" N (slots of a window's candidate table in LDS; 0 = 256, at most 256);
 *   "sw_slice" N (queries per launch of rb3gpu_sw_e2e and rb3gpu_sw_local; 0 = 16 K), "sw_table" N (as "hapdiv_table", for both);
 *   "suffix_slice" N (queries per launch of rb3gpu_suffix; 0 = 4 M), "get_slice" N (symbols of an emit slice of rb3gpu_retrieve; 0 = 64 M);
 *   "dedup_slice" N (strings per launch of rb3gpu_dedup; 0 = 4 M), "dedup_early" 0/1 (its walks end once the string is known to be unique; default 1);
 *   "ovl_strings" N (strings per launch of the counting walk of rb3gpu_overlap; 0 = 4 M), "ovl_slice" N (records of an emit slice; 0 = 16 M), "ovl_early" 0/1 (default 1);
 *   "ovl_resident" N (records rb3gpu_overlap_reduced may hold on the device; 0 = as many as can be allocated), "ovl_reduce_strings" N (strings per launch of its reduction; 0 = 4 M);
 *   "utg_slice" N (symbols of an emit slice of rb3gpu_unitigs; 0 = 64 M), "utg_strings" N (members per launch of its emitting walk; 0 = 4 M);
 *   "get_piece" S (splitter spacing 2^S of rb3gpu_retrieve_pieces, 1..20; 0 = 8); "fetch_slice" N (symbols of a slice of regions of rb3gpu_fetch; 0 = 64 M);
 *   "seed_chunk" N (window starts per walker of rb3gpu_seed_present where the call names none; 0 = 2048), "seed_slice" N (its walkers per launch; 0 = 1 M);
 *   "locate_heap" N (entries of an octet's heap in LDS, rb3gpu_locate; 0 = 32, at most 80), "locate_slice" N (bytes of global-memory heaps at once; 0 = 256 MB);
 *   the full table with defaults is in docs/LAB_NOTEBOOK.md section 8c
 * Test hooks "force_fallback", "tent_limit", "text_mode" exist only in the test build of the library (compiled with
 * -DRB3GPU_TEST_HOOKS, librb3gpu_hooks.so); the release library answers RB3GPU_EUNSUP.  Unknown key: RB3GPU_EINVAL. */
int rb3gpu_tune(rb3gpu_t *h, const char *key, int64_t value);

/* Test seam of the merge's settle phase (test build only; the release library answers RB3GPU_EUNSUP).  The caller hands over a
 * table of tentative stretches as the walkers of a merge would have left it, and the settle runs on it through the host functions a merge calls.
 *   ids[n_ids] (ascending), records: the stretch ids in use and their 64-byte records (rb3_stretch_t, csrc/rb3gpu_kernels.h); every other id is zero;
 *   masks: NULL, or for q > 1 the 8q mask words of every listed id (those of ids of the upper half are ignored);
 *   n_a, n_b: the extents of the two halves of the table; chunk_ctr: NULL, or the 64 chunk counters the extent of the lower half is worked out from
 *   instead of n_a (the path of a merge with narrow masks: the first settle kernel does it on its way);
 *   q: 1, 2, 4, 8 (masks of 256 q bits); maxhops: walkers a dependency path is followed over before the second chance takes it;
 *   engine: 0 = the merge's own (the settle kernels, then pointer jumping if a path was longer than maxhops), 1 = "resolve_v1" (q = 1 only);
 *   phase: 0 = only the masks of the events, worked out from the handle's index; 1 = everything else, the masks taken as given; 2 = everything.
 * Out: sfin_out[n_ids] (0: unsettled, else 1 + the unknown), masks_out (NULL, or 8q words per id: what the phase left behind -- per event after phase 0,
 * cumulative after the others), bad_out[3] (the counters of the validation; [2] != 0: a path was longer than maxhops), *second_chance (it ran).
 * RB3GPU_EINVAL for a table that names an id outside the extents or an interval outside the index: nothing malformed reaches the device.  The handle
 * stays usable (its bookkeeping of the table's used part is kept). */
int rb3gpu_test_settle(rb3gpu_t *h, int64_t n_ids, const int32_t *ids, const void *records, const uint32_t *masks, int64_t n_a, int64_t n_b, const uint32_t *chunk_ctr,
		int q, int maxhops, int engine, int phase, int32_t *sfin_out, uint32_t *masks_out, uint64_t *bad_out, int *second_chance);

int rb3gpu_stats(const rb3gpu_t *h, rb3gpu_stats_t *st);
/* what the handle holds right now, buffer by buffer (diagnostics: which scratch makes up bytes_peak): i = 0, 1, ... until RB3GPU_EINVAL; *name is a static
 * string.  (No counterpart in the reference: its memory is the rope's, mrope.c:15-34.) */
int rb3gpu_buffer_bytes(const rb3gpu_t *h, int i, const char **name, int64_t *bytes);
void rb3gpu_stats_reset(rb3gpu_t *h);

/* device scratch helpers so that callers without a HIP binding (C host code, ctypes) can
 * keep a partial BWT resident in HBM: plain hipMalloc/hipMemcpy/hipFree on the handle's device */
int rb3gpu_dev_alloc(rb3gpu_t *h, int64_t n_bytes, void **d_ptr);
int rb3gpu_dev_upload(rb3gpu_t *h, void *d_dst, const void *src, int64_t n_bytes);
int rb3gpu_dev_download(rb3gpu_t *h, void *dst, const void *d_src, int64_t n_bytes);
int rb3gpu_dev_free(rb3gpu_t *h, void *d_ptr);
int rb3gpu_dev_copy(rb3gpu_t *h, void *d_dst, const void *d_src, int64_t n_bytes);   /* device to device */
int rb3gpu_dev_memset(rb3gpu_t *h, void *d_dst, int byte, int64_t n_bytes);
int rb3gpu_sync(rb3gpu_t *h);

/* number of HIP devices visible, or a negative error */
int rb3gpu_device_count(void);

#ifdef __cplusplus
}
#endif

#endif
