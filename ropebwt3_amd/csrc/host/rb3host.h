/*
 * rb3host.h -- host-side C of the MI355X build: everything around the HIP merge engine that
 * `ropebwt3 build` needs (sequence input, per-batch suffix sorting, FMD / FMR codecs).
 * Citations are file:line in the reference tree.
 */
#ifndef RB3HOST_H
#define RB3HOST_H

#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RB3H_VERSION "3.10-r281-mi355x-r4"

extern int rb3h_verbose;

/* ---- misc (misc.c:7-16, 116-150) ---- */
int64_t rb3h_parse_num(const char *str);
int rb3h_parse_rows(const char *str, int64_t *a, int64_t *b);              /* `7` or `3-9` of `remove`: 0, or -1 for anything else */
typedef struct { int64_t name_len, beg, end; int strand, stranded; } rb3h_region_t; /* the name is the first name_len bytes of what was parsed; strand +1 or -1, stranded: it was named */
int rb3h_region_parse(const char *str, int bed, rb3h_region_t *r);           /* `name:beg-end[:+|:-]` of `fetch`, or a BED line: 0, or -1 for anything else */
double rb3h_realtime(void);
double rb3h_cputime(void);
double rb3h_percent_cpu(void);
long rb3h_peakrss(void);
void rb3h_init(void);

/* ---- suffix sorting of one batch (sais-ss.c:50-56) ----
 * n_threads is there for signature parity with rb3_build_sais and is IGNORED: this from-scratch SA-IS is sequential
 * (parallelism on the host side is `-p N`: N batches at once).  It is the fallback sorter only. */
int rb3h_build_bwt(int64_t n_seq, int64_t len, uint8_t *seq, int n_threads);
/* same, plus the LF-walker list for rb3gpu_merge_plain_walkers (layout = rb3gpu_walker_t): the
 * sampled inverse suffix array is free here because the suffix array is still in memory */
typedef struct { int64_t row, ka0, nsteps, flags; } rb3h_walker_t;
int rb3h_build_bwt_walkers(int64_t n_seq, int64_t len, uint8_t *seq, int n_threads, int64_t step, int64_t *n_walkers, rb3h_walker_t **walkers);
int rb3h_walkers_from_ckrow(int64_t len, const uint8_t *text, int64_t step, const int64_t *ckrow, int64_t *n_walkers, rb3h_walker_t **walkers);
int rb3h_walkers_text(int64_t len, const uint8_t *text, int64_t step, int64_t *n_walkers, rb3h_walker_t **walkers); /* by text position (rb3gpu_merge_text_dev) */

/* ---- sequence input (io.c) ---- */
typedef struct { int64_t l, m; uint8_t *s; } rb3h_buf_t;
struct rb3h_seqio_s;
typedef struct rb3h_seqio_s rb3h_seqio_t;
rb3h_seqio_t *rb3h_seq_open(const char *fn, int is_line);                  /* io.c:60-72 */
void rb3h_seq_close(rb3h_seqio_t *fp);                                     /* io.c:74-82 */
/* a byte range of a plain file (`build --gpus N` on one file): the records that START in [beg, end); end <= 0: to the end of the file */
int rb3h_seq_splittable(const char *fn, int64_t *size);                    /* a regular file that is not gzip-compressed */
rb3h_seqio_t *rb3h_seq_open_range(const char *fn, int is_line, int64_t beg, int64_t end);
int64_t rb3h_seq_record_start(const char *fn, int is_line, int64_t off);            /* the cut rb3h_seq_open_range makes at an offset (-1: not a plain file) */
/* io.c:104-125: fill `seq` with nt6(forward)+0 and nt6(revcomp)+0 per record until
 * seq->l > max_len; returns the number of strings appended (0 at EOF) or <0 on a parse error;
 * *n_empty counts records of length 0, which are skipped (out of contract in the reference) */
int64_t rb3h_seq_read(rb3h_seqio_t *fp, rb3h_buf_t *seq, int64_t max_len, int is_for, int is_rev, int64_t *n_empty);
/* where the batch buffer (`seq` of rb3h_seq_read) gets its memory: alloc returns at least min_bytes and says how much it
 * gave in *cap (a pool may hand out a larger buffer); NULL, NULL = realloc/free (default).  The CLI sets page-locked memory
 * here (rb3gpu_pinned_alloc) so that a batch goes to HBM with one DMA; a batch buffer is then freed with rb3h_batch_free. */
typedef void *(*rb3h_alloc_f)(int64_t min_bytes, int64_t *cap);
typedef void (*rb3h_free_f)(void *p);
void rb3h_seq_set_batch_allocator(rb3h_alloc_f alloc, rb3h_free_f release);
void rb3h_batch_free(void *p);
int rb3h_seq_error(const rb3h_seqio_t *fp); /* != 0: a FASTX parsing error ended the file early (code as in kseq: -2 truncated quality, ...) */
/* one record with its name (io.c:127-144): the query commands' reader; see seqio.c */
int64_t rb3h_seq_read1(rb3h_seqio_t *fp, const uint8_t **seq, const char **name);
/* a batch of whole records for a query command (the loop of search.c:366-378): records are added until sym.l >= max_sym or n >= max_rec.  Record q is the nt6
 * codes sym.s[off[q], off[q + 1]) and its name names.s + name_off[q] (-1: none, a file of lines); eof: rb3h_seq_read1 said the file is over (see rb3h_seq_error).
 * Returns n, -1 (no memory) or -2 (a record of more than max_len symbols); nothing of a failed batch is for use.  Prints nothing; the buffers serve the next call */
typedef struct { rb3h_buf_t sym, names; int64_t *off, *name_off, n, m; int eof; } rb3h_qbatch_t;
int64_t rb3h_qbatch_read(rb3h_seqio_t *fp, rb3h_qbatch_t *b, int64_t max_sym, int64_t max_rec, int64_t max_len);
void rb3h_qbatch_free(rb3h_qbatch_t *b);
int64_t rb3h_strand_pairs(int64_t len, const uint8_t *text, int64_t n_seq, int64_t max_pairs, int64_t *pair_start); /* record offsets of a both-strand batch */
void rb3h_char2nt6(int64_t l, uint8_t *s);                                 /* io.c:23-28 */
void rb3h_revcomp6(int64_t l, uint8_t *s);                                 /* io.c:30-40 */

/* ---- the output of `mem` (write_per_seq, search.c:240-325) ---- */
typedef struct { int64_t query, x0, size; int32_t st, en; } rb3h_mem_rec_t; /* = rb3gpu_mem_rec_t */
#define RB3H_MEM_LINES 0   /* name, start, end, occurrences per match */
#define RB3H_MEM_GAP   1   /* --gap=NUM: the stretches of at least min_gap symbols that no match covers: name, start, end, query length */
#define RB3H_MEM_COV   2   /* --cov: name, query length, symbols covered; nothing for a query without cover */
/* the lines of ONE query appended to `out` (grown with realloc): its n matches r[0..n) by start, its name (NULL: seq<id + 1>) and length; 0 or -1 (no memory) */
int rb3h_mem_format(rb3h_buf_t *out, int mode, int64_t min_gap, const char *name, int64_t id, int64_t len, int64_t n, const rb3h_mem_rec_t *r);

/* the same lines with the positions of every match (`mem -p`, search.c:305-314): after the occurrences the number of positions and name:strand:position of each.
 * The positions of r[i] are pos[off[i], off[i + 1]); a match without positions gets no extra column.  sid: the indexed sequences (rb3h_sid_read) */
typedef struct { int64_t sid, pos; } rb3h_pos_t;                           /* = rb3gpu_pos_t */
typedef struct { int64_t n_seq; char **name; int64_t *len; } rb3h_sid_t;
int rb3h_mem_format_pos(rb3h_buf_t *out, const char *name, int64_t id, int64_t n, const rb3h_mem_rec_t *r, const int64_t *off, const rb3h_pos_t *pos, const rb3h_sid_t *sid);
/* the text `hapdiv` writes for one query (write_hapdiv, search.c:327-353): its n windows start every w symbols and are k long; r holds nine numbers per
 * window (n_al, max_ed, n_hap[0..6]); consecutive windows with the same nine make one line: name, first start, last end, the nine */
int rb3h_hapdiv_format(rb3h_buf_t *out, const char *name, int64_t id, int64_t k, int64_t w, int64_t n, const int32_t *r);

/* ---- the output of `sw` in end-to-end mode (swfmt.c) ---- */
typedef struct { int64_t lo, hi; int32_t score, qlen, rlen, n_steps; int64_t step_off, pos_off, n_pos; } rb3h_sw_hit_t; /* = rb3gpu_sw_hit_t */
/* the PAF lines of ONE query (write_paf, search.c:175-216): its n hits with their step bytes (one per step from query position 0 on, op << 4 | base with op
 * 0 = 1 X 2 I 3 D) and positions (hit i: pos[pos_off, pos_off + n_pos)); seq: its nt6 codes.  sid NULL: positions as string number and offset.  unmapped: the -u
 * line of a query without a hit; with_rs: the rs tag of --seq.  0, -1 (no memory) or -2 (a position names a string the name list does not have) */
int rb3h_sw_format_paf(rb3h_buf_t *out, const char *name, int64_t id, int64_t len, const uint8_t *seq, int64_t n, const rb3h_sw_hit_t *hits, const uint8_t *steps,
		const rb3h_pos_t *pos, const rb3h_sid_t *sid, int unmapped, int with_rs);
/* the QS / QH / // block of ONE query and strand (write_all_hits, search.c:218-238); seq: the codes that were aligned; max_out <= 0: no cap */
int rb3h_sw_format_all(rb3h_buf_t *out, const char *name, int64_t id, int64_t len, const uint8_t *seq, int64_t n, const rb3h_sw_hit_t *hits, const uint8_t *steps,
		char strand, int64_t max_out);

/* the same with the hit's place on the query (`sw --local`): columns 3 and 4 are qoff0[i] and qoff0[i] + qlen of hit i, the cs string reads the query from
 * qoff0[i] on, and qh:i: is n_qoff[i].  qoff0 / n_qoff NULL: 0 and 1, which is rb3h_sw_format_paf */
int rb3h_sw_format_paf_at(rb3h_buf_t *out, const char *name, int64_t id, int64_t len, const uint8_t *seq, int64_t n, const rb3h_sw_hit_t *hits, const uint8_t *steps,
		const rb3h_pos_t *pos, const rb3h_sid_t *sid, int unmapped, int with_rs, const int32_t *qoff0, const int32_t *n_qoff);

/* ---- the graph of a query that `sw --local` aligns over (dawg.c) ---- */
/* n_node nodes in topological order, node 0 the root (the empty string); node i carries symbol sym[i] (1..4; 0 for the root), its predecessors are
 * pre[pre_off[i], pre_off[i + 1]) in the order candidates arrive from them, its string starts at qoff0[i] of the query and occurs n_qoff[i] times in it */
typedef struct { int64_t n_node, n_pre; uint8_t *sym; int64_t *pre_off; int32_t *pre, *qoff0, *n_qoff; } rb3h_dawg_t;
int rb3h_dawg_build(int64_t len, const uint8_t *seq, rb3h_dawg_t *g);       /* seq: nt6 codes; 0, -1 (no memory) or -3 (too long) */
/* the graphs of the queries symbols[offsets[q], offsets[q + 1]) one after another (OpenMP over the queries): query q owns the nodes [node_off[q], node_off[q + 1])
 * of `out`, pre_off[] runs over all nodes and names places of pre[], whose entries are node numbers within the query; node_off holds n_query + 1 */
int rb3h_dawg_batch(int64_t n_query, const int64_t *offsets, const uint8_t *symbols, rb3h_dawg_t *out, int64_t *node_off);
void rb3h_dawg_free(rb3h_dawg_t *g);

/* ---- the files beside an index that `mem -p` and `sw` read (sidefile.c) ---- */
typedef struct { int32_t ss, ms; int64_t m, n_ssa; uint64_t *r2i, *ssa; } rb3h_ssa_t;
rb3h_ssa_t *rb3h_ssa_read(const char *fn);                                 /* rb3_ssa_restore, ssa.c:215-241; NULL: no file, wrong magic, or it ends early */
void rb3h_ssa_destroy(rb3h_ssa_t *sa);
rb3h_sid_t *rb3h_sid_read(const char *fn);                                 /* rb3_sid_read, io.c:161-204 (gzip or plain) */
void rb3h_sid_destroy(rb3h_sid_t *sl);

/* ---- FMD (rld0) writer / reader ---- */
struct rb3h_fmdw_s;
typedef struct rb3h_fmdw_s rb3h_fmdw_t;
rb3h_fmdw_t *rb3h_fmdw_init(void);                                         /* rld_init(6, 3), rld0.c:57-75 */
int rb3h_fmdw_enc(rb3h_fmdw_t *w, int64_t l, int c);                        /* rld_enc, rld0.c:153-161 */
int rb3h_fmdw_enc_words(rb3h_fmdw_t *w, int64_t n, const uint64_t *words, int64_t end); /* bulk: start << 3 | sym of maximal runs */
int rb3h_fmdw_adopt(rb3h_fmdw_t *w, uint64_t *words, int64_t n_words, const int64_t acc[7]); /* data section packed elsewhere */
int rb3h_fmdw_finish(rb3h_fmdw_t *w);                                      /* rld_enc_finish, rld0.c:206-216 */
int rb3h_fmdw_dump_file(const rb3h_fmdw_t *w, const char *fn);
int rb3h_fmdw_dump(const rb3h_fmdw_t *w, FILE *fp);                         /* rld_dump, rld0.c:222-243 */
void rb3h_fmdw_destroy(rb3h_fmdw_t *w);
int64_t rb3h_fmdw_nbytes(const rb3h_fmdw_t *w);

typedef int (*rb3h_run_f)(void *data, int c, int64_t l);
/* decode every run of an FMD file in order (rld_restore + rld_dec, rld0.c:267-320, rld0.h:85-122) */
int rb3h_fmd_read_runs(FILE *fp, rb3h_run_f emit, void *data, int64_t mcnt[6]);
int rb3h_fmd_read_words(const char *fn, uint64_t **z, int64_t *n_words, int64_t mcnt[6]); /* undecoded, for rb3gpu_from_fmd_words */
int rb3h_fmd_read_words_fp(FILE *fp, uint64_t **z, int64_t *n_words, int64_t mcnt[6]);    /* the same from a stream whose 4 bytes of magic have been consumed */

/* ---- FMR (mrope) writer / reader ---- */
struct rb3h_fmrw_s;
typedef struct rb3h_fmrw_s rb3h_fmrw_t;
/* stream runs in BWT order, then dump the six ropes (mr_dump, mrope.c:152-159; rope_dump,
 * rope.c:265-287).  cnt[6] = symbol counts of the whole BWT (rope a holds rows C[a]..C[a+1]). */
rb3h_fmrw_t *rb3h_fmrw_init(const int64_t acc[7], int max_nodes, int block_len);
int rb3h_fmrw_enc(rb3h_fmrw_t *w, int64_t l, int c);
int rb3h_fmrw_dump(rb3h_fmrw_t *w, FILE *fp);
void rb3h_fmrw_set_order(rb3h_fmrw_t *w, int so); /* byte 3 of the header (mr_dump, mrope.c:155-156): RB3GPU_SO_* / MR_SO_* */
void rb3h_fmrw_destroy(rb3h_fmrw_t *w);
/* decode an FMR file (mr_restore, mrope.c:161-177; rope_restore, rope.c:289-330) */
int rb3h_fmr_read_runs(FILE *fp, rb3h_run_f emit, void *data);

/* ---- BRE, the reference's interchange format (bre.c) ---- */
#define RB3H_BRE_EOPEN   (-1)  /* the file cannot be opened */
#define RB3H_BRE_EMAGIC  (-2)  /* not "BRE\1" */
#define RB3H_BRE_EHEADER (-3)  /* b_per_sym != 1, asize != 6, b_per_run outside 1..8, or the file ends in its header */
#define RB3H_BRE_ERECORD (-4)  /* a record with a symbol above 5, or of no symbols in front of the footer */
#define RB3H_BRE_EFOOTER (-5)  /* no all-zero record, fewer than 24 bytes behind it, counts that disagree with the records, or no records */
#define RB3H_BRE_ENOMEM  (-6)
/* a BRE file in host memory: rec points at n_rec raw records of 1 + b_per_run bytes (what rb3gpu_from_bre takes), ftr holds the footer's n_rec, n_sym, n_run */
typedef struct { int b_per_run; int64_t n_rec, ftr[3]; const uint8_t *rec; uint8_t *buf; } rb3h_bre_t;
int rb3h_bre_read(const char *fn, rb3h_bre_t *b);                           /* "-": stdin; 0 or an RB3H_BRE_E* code */
int rb3h_bre_read_fp(FILE *fp, rb3h_bre_t *b);                              /* the 4 bytes of magic already consumed */
void rb3h_bre_free(rb3h_bre_t *b);
int rb3h_bre_decode_runs(const rb3h_bre_t *b, rb3h_run_f emit, void *data); /* maximal runs (records of one symbol joined); all three counts are held against the footer */
int rb3h_bre_read_runs(FILE *fp, rb3h_run_f emit, void *data);              /* read_fp + decode_runs */
int rb3h_bre_write_header(FILE *fp, int b_per_run);
int rb3h_bre_write_footer(FILE *fp, int b_per_run, int64_t n_rec, int64_t n_sym, int64_t n_run); /* the all-zero record and the counts */
/* the host's packer: header at init, records as runs arrive (adjacent runs of one symbol are joined, long ones split), footer at finish */
struct rb3h_brew_s;
typedef struct rb3h_brew_s rb3h_brew_t;
rb3h_brew_t *rb3h_brew_init(FILE *fp, int b_per_run);
int rb3h_brew_enc(rb3h_brew_t *w, int64_t l, int c);
int rb3h_brew_enc_words(rb3h_brew_t *w, int64_t n, const uint64_t *words, int64_t end); /* bulk: start << 3 | sym of maximal runs */
int rb3h_brew_finish(rb3h_brew_t *w);
void rb3h_brew_destroy(rb3h_brew_t *w);

/* open an index file of any kind and stream its runs; returns 0, or <0 on error */
int rb3h_index_read_runs(const char *fn, rb3h_run_f emit, void *data);
/* the same in two steps, for a caller that treats the kinds differently and must open the file only once (it may be a pipe, or stdin: "-"):
 * rb3h_index_open reads the 4 bytes of magic and returns the stream behind them (NULL: no file, or shorter; close it unless it is stdin),
 * rb3h_index_kind names them, rb3h_index_read_runs_fp / rb3h_fmd_read_words_fp / rb3h_bre_read_fp go on from there */
enum { RB3H_INDEX_NONE = 0, RB3H_INDEX_FMD, RB3H_INDEX_FMR, RB3H_INDEX_BRE };
FILE *rb3h_index_open(const char *fn, char magic[4]);
int rb3h_index_kind(const char magic[4]);
int rb3h_index_read_runs_fp(FILE *fp, const char magic[4], rb3h_run_f emit, void *data);

#ifdef __cplusplus
}
#endif

#endif
