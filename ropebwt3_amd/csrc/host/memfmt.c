/*
 * memfmt.c -- the text `mem` writes for one query (write_per_seq, search.c:240-325, and the gaps of worker_for_seq,
 * search.c:110-126), into a buffer that its caller writes out in large pieces: a printf per line is the whole wall
 * time of a command that prints millions of them.  And the lines of `hapdiv` (write_hapdiv, search.c:327-353).
 */
#include <stdlib.h>
#include <string.h>
#include "rb3host.h"

static int fmt_reserve(rb3h_buf_t *b, int64_t more)
{
	if (b->l + more <= b->m) return 0;
	{
		int64_t m = b->l + more;
		uint8_t *s;
		m += (m >> 1) + 64;
		s = (uint8_t*)realloc(b->s, (size_t)m);
		if (s == 0) return -1;
		b->s = s, b->m = m;
	}
	return 0;
}

static inline uint8_t *fmt_num(uint8_t *p, int64_t x) /* "%ld" */
{
	char t[24];
	int nt = 0;
	uint64_t u = x < 0 ? (uint64_t)0 - (uint64_t)x : (uint64_t)x;
	if (x < 0) *p++ = '-';
	do t[nt++] = (char)('0' + u % 10), u /= 10; while (u);
	while (nt > 0) *p++ = (uint8_t)t[--nt];
	return p;
}

static inline uint8_t *fmt_name(uint8_t *p, const char *name, size_t l_name, int64_t id)
{
	if (name) { memcpy(p, name, l_name); return p + l_name; }
	memcpy(p, "seq", 3);
	return fmt_num(p + 3, id + 1);
}

int rb3h_mem_format(rb3h_buf_t *out, int mode, int64_t min_gap, const char *name, int64_t id, int64_t len, int64_t n, const rb3h_mem_rec_t *r)
{
	const size_t l_name = name ? strlen(name) : 0;
	const int64_t line_max = (int64_t)l_name + 24 + 3 * 22 + 2;
	int64_t i;
	uint8_t *p;
	if (mode == RB3H_MEM_GAP) { /* search.c:110-126 */
		int64_t last = 0;
		for (i = 0; i <= n; ++i) {
			const int64_t st = i < n ? r[i].st : len, en = i < n ? r[i].en : len;
			int gap;
			if (i < n) {
				gap = st > last && st - last >= min_gap;
			} else gap = len - last >= min_gap;
			if (gap) {
				if (fmt_reserve(out, line_max) < 0) return -1;
				p = fmt_name(out->s + out->l, name, l_name, id);
				*p++ = '\t', p = fmt_num(p, last);
				*p++ = '\t', p = fmt_num(p, st);
				*p++ = '\t', p = fmt_num(p, len);
				*p++ = '\n';
				out->l = p - out->s;
			}
			if (i < n) last = st > last ? en : (last > en ? last : en);
		}
	} else if (mode == RB3H_MEM_COV) { /* search.c:279-295 */
		int64_t st0 = 0, en0 = 0, cov = 0;
		for (i = 0; i < n; ++i) {
			if (r[i].st > en0) cov += en0 - st0, st0 = r[i].st, en0 = r[i].en;
			else en0 = en0 > r[i].en ? en0 : r[i].en;
		}
		cov += en0 - st0;
		if (cov > 0) {
			if (fmt_reserve(out, line_max) < 0) return -1;
			p = fmt_name(out->s + out->l, name, l_name, id);
			*p++ = '\t', p = fmt_num(p, len);
			*p++ = '\t', p = fmt_num(p, cov);
			*p++ = '\n';
			out->l = p - out->s;
		}
	} else { /* search.c:296-318 without positions */
		if (fmt_reserve(out, n * line_max) < 0) return -1;
		p = out->s + out->l;
		for (i = 0; i < n; ++i) {
			p = fmt_name(p, name, l_name, id);
			*p++ = '\t', p = fmt_num(p, r[i].st);
			*p++ = '\t', p = fmt_num(p, r[i].en);
			*p++ = '\t', p = fmt_num(p, r[i].size);
			*p++ = '\n';
		}
		out->l = p - out->s;
	}
	return 0;
}

int rb3h_mem_format_pos(rb3h_buf_t *out, const char *name, int64_t id, int64_t n, const rb3h_mem_rec_t *r, const int64_t *off, const rb3h_pos_t *pos, const rb3h_sid_t *sid)
{
	const size_t l_name = name ? strlen(name) : 0;
	int64_t i, k;
	for (i = 0; i < n; ++i) { /* search.c:298-317 */
		const int64_t np = off[i + 1] - off[i];
		uint8_t *p;
		if (fmt_reserve(out, (int64_t)l_name + 24 + 4 * 22 + 2) < 0) return -1;
		p = fmt_name(out->s + out->l, name, l_name, id);
		*p++ = '\t', p = fmt_num(p, r[i].st);
		*p++ = '\t', p = fmt_num(p, r[i].en);
		*p++ = '\t', p = fmt_num(p, r[i].size);
		if (np > 0) *p++ = '\t', p = fmt_num(p, np);
		out->l = p - out->s;
		for (k = off[i]; k < off[i + 1]; ++k) {
			const int64_t s = pos[k].sid >> 1;
			const char *sn;
			size_t l_sn;
			int64_t x;
			if (s < 0 || s >= sid->n_seq) return -2; /* (a string the name list does not know: the files do not belong together) */
			sn = sid->name[s], l_sn = strlen(sn);
			x = pos[k].sid & 1 ? sid->len[s] - (pos[k].pos + (r[i].en - r[i].st)) : pos[k].pos;
			if (fmt_reserve(out, (int64_t)l_sn + 32) < 0) return -1;
			p = out->s + out->l;
			*p++ = '\t';
			memcpy(p, sn, l_sn), p += l_sn;
			*p++ = ':', *p++ = (uint8_t)"+-"[pos[k].sid & 1], *p++ = ':';
			p = fmt_num(p, x);
			out->l = p - out->s;
		}
		if (fmt_reserve(out, 1) < 0) return -1;
		out->s[out->l++] = '\n';
	}
	return 0;
}

int rb3h_hapdiv_format(rb3h_buf_t *out, const char *name, int64_t id, int64_t k, int64_t w, int64_t n, const int32_t *r)
{
	const size_t l_name = name ? strlen(name) : 0;
	int64_t i, j;
	for (i = 0; i < n; i = j) {
		uint8_t *p;
		int e;
		for (j = i + 1; j < n && memcmp(r + 9 * i, r + 9 * j, 36) == 0; ++j) {}
		if (fmt_reserve(out, (int64_t)l_name + 24 + 11 * 22 + 2) < 0) return -1;
		p = fmt_name(out->s + out->l, name, l_name, id);
		*p++ = '\t', p = fmt_num(p, i * w);
		*p++ = '\t', p = fmt_num(p, (j - 1) * w + k);
		for (e = 0; e < 9; ++e) *p++ = '\t', p = fmt_num(p, r[9 * i + e]);
		*p++ = '\n';
		out->l = p - out->s;
	}
	return 0;
}
