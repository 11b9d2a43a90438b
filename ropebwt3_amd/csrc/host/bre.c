/* BRE, the reference's run-length interchange format (bre.h; written by `build -e`, mr_print_bre build.c:85-106; read by
 * rld_restore, rld0.c:245-283): a 24-byte header (+ auxiliary bytes), records of one symbol byte and b_per_run length bytes
 * (little-endian), an all-zero record, and three 8-byte counts -- records, symbols, runs.  Unlike the reference, which complains
 * and goes on with what it read, a file without a footer or with one that disagrees with the records is refused. */
#include <stdlib.h>
#include <string.h>
#include "rb3host.h"

static uint64_t le_get(const uint8_t *p, int n)
{
	uint64_t x = 0;
	int i;
	for (i = 0; i < n; ++i) x |= (uint64_t)p[i] << (8 * i);
	return x;
}

static void le_put(uint8_t *p, int n, uint64_t x)
{
	int i;
	for (i = 0; i < n; ++i) p[i] = (uint8_t)(x >> (8 * i));
}

void rb3h_bre_free(rb3h_bre_t *b)
{
	free(b->buf);
	memset(b, 0, sizeof(*b));
}

/* the magic has been consumed by the caller */
int rb3h_bre_read_fp(FILE *fp, rb3h_bre_t *b)
{
	uint8_t hdr[20];
	uint64_t l_aux;
	int64_t n = 0, m = 0, i, rs, n_slots;
	uint8_t *buf = 0;
	memset(b, 0, sizeof(*b));
	if (fread(hdr, 1, 20, fp) != 20) return RB3H_BRE_EHEADER;
	if (hdr[0] != 1 || hdr[1] < 1 || hdr[1] > 8 || le_get(hdr + 4, 8) != 6) return RB3H_BRE_EHEADER; /* b_per_sym, b_per_run, asize */
	l_aux = le_get(hdr + 12, 8);
	if (l_aux >> 40) return RB3H_BRE_EHEADER;
	for (; l_aux > 0; --l_aux) if (fgetc(fp) == EOF) return RB3H_BRE_EHEADER;
	for (;;) { /* the rest of the file (which may be a pipe) */
		size_t k;
		if (m - n < (1 << 16)) {
			uint8_t *t;
			m = m ? m + (m >> 1) : 1 << 20;
			if ((t = (uint8_t*)realloc(buf, (size_t)m)) == 0) { free(buf); return RB3H_BRE_ENOMEM; }
			buf = t;
		}
		if ((k = fread(buf + n, 1, (size_t)(m - n), fp)) == 0) break;
		n += (int64_t)k;
	}
	b->buf = buf, b->rec = buf, b->b_per_run = hdr[1];
	rs = 1 + b->b_per_run, n_slots = n / rs;
	for (i = 0; i < n_slots; ++i) { /* up to the all-zero record */
		const uint8_t *p = buf + i * rs;
		int j, zero = 1;
		for (j = 1; j < rs; ++j) if (p[j]) { zero = 0; break; }
		if (zero && p[0] == 0) break;
		if (zero || p[0] > 5) { rb3h_bre_free(b); return RB3H_BRE_ERECORD; } /* no symbols, or no symbol of the alphabet */
	}
	if (i == n_slots || n - (i + 1) * rs < 24) { rb3h_bre_free(b); return RB3H_BRE_EFOOTER; }
	b->n_rec = i;
	b->ftr[0] = (int64_t)le_get(buf + (i + 1) * rs, 8), b->ftr[1] = (int64_t)le_get(buf + (i + 1) * rs + 8, 8), b->ftr[2] = (int64_t)le_get(buf + (i + 1) * rs + 16, 8);
	if (b->ftr[0] != b->n_rec || b->n_rec == 0) { rb3h_bre_free(b); return RB3H_BRE_EFOOTER; }
	return 0;
}

int rb3h_bre_read(const char *fn, rb3h_bre_t *b)
{
	FILE *fp = strcmp(fn, "-") == 0 ? stdin : fopen(fn, "rb");
	char magic[4];
	int ret;
	memset(b, 0, sizeof(*b));
	if (fp == 0) return RB3H_BRE_EOPEN;
	if (fread(magic, 1, 4, fp) != 4 || memcmp(magic, "BRE\1", 4) != 0) ret = RB3H_BRE_EMAGIC;
	else ret = rb3h_bre_read_fp(fp, b);
	if (fp != stdin) fclose(fp);
	return ret;
}

/* the records as maximal runs (records of one symbol joined), held against the footer */
int rb3h_bre_decode_runs(const rb3h_bre_t *b, rb3h_run_f emit, void *data)
{
	const int bpr = b->b_per_run, rs = 1 + bpr;
	int64_t i, n_sym = 0, n_run = 0, pl = 0;
	int pc = -1;
	for (i = 0; i < b->n_rec; ++i) {
		const uint8_t *p = b->rec + i * rs;
		const uint64_t l = le_get(p + 1, bpr);
		if (p[0] > 5 || l == 0 || l >> 56) return RB3H_BRE_ERECORD;
		n_sym += (int64_t)l;
		if (p[0] == pc) pl += (int64_t)l;
		else {
			if (pl > 0 && emit(data, pc, pl) != 0) return RB3H_BRE_ENOMEM;
			pc = p[0], pl = (int64_t)l, ++n_run;
		}
	}
	if (pl > 0 && emit(data, pc, pl) != 0) return RB3H_BRE_ENOMEM;
	if (b->n_rec != b->ftr[0] || n_sym != b->ftr[1] || n_run != b->ftr[2] || n_sym == 0) return RB3H_BRE_EFOOTER;
	return 0;
}

int rb3h_bre_read_runs(FILE *fp, rb3h_run_f emit, void *data)
{
	rb3h_bre_t b;
	int ret = rb3h_bre_read_fp(fp, &b);
	if (ret == 0) ret = rb3h_bre_decode_runs(&b, emit, data);
	rb3h_bre_free(&b);
	return ret;
}

/* ---- writer ---- */

int rb3h_bre_write_header(FILE *fp, int b_per_run)
{
	uint8_t hdr[24];
	memset(hdr, 0, sizeof(hdr));
	memcpy(hdr, "BRE\1", 4);
	hdr[4] = 1, hdr[5] = (uint8_t)b_per_run, hdr[6] = 2, hdr[7] = 0; /* b_per_sym, b_per_run, atype DNA6, mtype */
	le_put(hdr + 8, 8, 6);  /* asize */
	le_put(hdr + 16, 8, 0); /* l_aux */
	return fwrite(hdr, 1, 24, fp) == 24 ? 0 : -1;
}

int rb3h_bre_write_footer(FILE *fp, int b_per_run, int64_t n_rec, int64_t n_sym, int64_t n_run)
{
	uint8_t ftr[9 + 24];
	const size_t rs = 1 + (size_t)b_per_run;
	memset(ftr, 0, sizeof(ftr));
	le_put(ftr + rs, 8, (uint64_t)n_rec), le_put(ftr + rs + 8, 8, (uint64_t)n_sym), le_put(ftr + rs + 16, 8, (uint64_t)n_run);
	return fwrite(ftr, 1, rs + 24, fp) == rs + 24 ? 0 : -1;
}

/* the host's packer: runs in BWT order (adjacent ones may carry one symbol: joined) -> header, records, footer */
struct rb3h_brew_s {
	FILE *fp;
	int bpr, c, wc, err;
	int64_t l, n_rec, n_sym, n_run, start; /* (c, l): the run that is still open; (wc, start): the last run word, whose run ends with the next one */
	uint8_t *buf;
	size_t n_buf;
};
#define BREW_BUF (1 << 16)

rb3h_brew_t *rb3h_brew_init(FILE *fp, int b_per_run)
{
	rb3h_brew_t *w;
	if (b_per_run < 1 || b_per_run > 8 || (w = (rb3h_brew_t*)calloc(1, sizeof(*w))) == 0) return 0;
	w->fp = fp, w->bpr = b_per_run, w->c = w->wc = -1;
	if ((w->buf = (uint8_t*)malloc(BREW_BUF + 16)) == 0 || rb3h_bre_write_header(fp, b_per_run) < 0) { free(w->buf); free(w); return 0; }
	return w;
}

static void brew_put(rb3h_brew_t *w, uint64_t n_sym)
{
	if (w->n_buf + 9 > BREW_BUF) {
		if (fwrite(w->buf, 1, w->n_buf, w->fp) != w->n_buf) w->err = -1;
		w->n_buf = 0;
	}
	w->buf[w->n_buf] = (uint8_t)w->c;
	le_put(w->buf + w->n_buf + 1, w->bpr, n_sym);
	w->n_buf += 1 + (size_t)w->bpr, ++w->n_rec;
}

/* the open run as records: as many of the largest length the bytes hold as fit into it, then what is left over */
static void brew_flush_run(rb3h_brew_t *w)
{
	const uint64_t cap = w->bpr >= 8 ? ~0ull : (1ull << (8 * w->bpr)) - 1;
	uint64_t k, n_full, tail;
	if (w->c < 0 || w->l <= 0) return;
	n_full = (uint64_t)w->l / cap, tail = (uint64_t)w->l % cap;
	++w->n_run, w->n_sym += w->l;
	for (k = 0; k < n_full; ++k) brew_put(w, cap);
	if (tail > 0) brew_put(w, tail);
	w->l = 0;
}

int rb3h_brew_enc(rb3h_brew_t *w, int64_t l, int c)
{
	if (l <= 0) return 0;
	if (c == w->c) w->l += l;
	else brew_flush_run(w), w->c = c, w->l = l;
	return w->err;
}

/* bulk: start << 3 | sym of maximal runs, as rb3gpu_export_run_words / rb3gpu_shard_export_run_words hand them out */
int rb3h_brew_enc_words(rb3h_brew_t *w, int64_t n, const uint64_t *words, int64_t end)
{
	int64_t i;
	for (i = 0; i < n; ++i) {
		const int64_t s = (int64_t)(words[i] >> 3);
		if (w->wc >= 0) rb3h_brew_enc(w, s - w->start, w->wc);
		w->wc = (int)(words[i] & 7), w->start = s;
	}
	if (end >= 0 && w->wc >= 0) rb3h_brew_enc(w, end - w->start, w->wc), w->wc = -1;
	return w->err;
}

int rb3h_brew_finish(rb3h_brew_t *w)
{
	brew_flush_run(w);
	if (w->n_buf > 0 && fwrite(w->buf, 1, w->n_buf, w->fp) != w->n_buf) w->err = -1;
	w->n_buf = 0;
	if (w->err == 0 && rb3h_bre_write_footer(w->fp, w->bpr, w->n_rec, w->n_sym, w->n_run) < 0) w->err = -1;
	return w->err;
}

void rb3h_brew_destroy(rb3h_brew_t *w)
{
	if (w == 0) return;
	free(w->buf);
	free(w);
}
