/*
 * swfmt.c -- the text `sw` writes for one query (end to end, or its one local hit with its place on the query), made from the step bytes of its hits (rb3gpu_sw_e2e: one byte per
 * step from query position 0 on, op << 4 | base): the PAF of write_paf (search.c:175-216) with the cigar, the cs string (sw_cs_core,
 * bwa-sw.c:116-152), the rs tag and the further positions, the -u line of a query without a hit, and the QS / QH / // block of
 * write_all_hits (search.c:218-238).  Into a buffer that the caller writes out in large pieces, as memfmt.c does.
 */
#include <stdlib.h>
#include <string.h>
#include "rb3host.h"

static int sw_reserve(rb3h_buf_t *b, int64_t more)
{
	int64_t m;
	uint8_t *s;
	if (b->l + more <= b->m) return 0;
	m = b->l + more, m += (m >> 1) + 64;
	s = (uint8_t*)realloc(b->s, (size_t)m);
	if (s == 0) return -1;
	b->s = s, b->m = m;
	return 0;
}

static inline uint8_t *sw_num(uint8_t *p, int64_t x)
{
	char t[24];
	int nt = 0;
	uint64_t u = x < 0 ? (uint64_t)0 - (uint64_t)x : (uint64_t)x;
	if (x < 0) *p++ = '-';
	do t[nt++] = (char)('0' + u % 10), u /= 10; while (u);
	while (nt > 0) *p++ = (uint8_t)t[--nt];
	return p;
}

static inline uint8_t *sw_str(uint8_t *p, const char *s)
{
	const size_t l = strlen(s);
	memcpy(p, s, l);
	return p + l;
}

static inline uint8_t *sw_name(uint8_t *p, const char *name, int64_t id)
{
	if (name) return sw_str(p, name);
	return sw_num(sw_str(p, "seq"), id + 1);
}

/* cs (at most 3 bytes per step and 12 per run) */
static uint8_t *sw_cs(uint8_t *p, const uint8_t *seq, int32_t n, const uint8_t *st)
{
	int32_t i, j, y = 0;
	for (i = 0; i < n; i = j) {
		const int op = st[i] >> 4;
		for (j = i + 1; j < n && st[j] >> 4 == op; ++j) {}
		if (op == 0) *p++ = ':', p = sw_num(p, j - i), y += j - i;
		else if (op == 1) {
			int32_t t;
			for (t = i; t < j; ++t, ++y) *p++ = '*', *p++ = (uint8_t)"$acgtn"[seq[y] < 5 ? seq[y] : 5], *p++ = (uint8_t)"$acgtn"[st[t] & 7];
		} else if (op == 2) {
			int32_t t;
			*p++ = '+';
			for (t = i; t < j; ++t, ++y) *p++ = (uint8_t)"$acgtn"[seq[y] < 5 ? seq[y] : 5];
		} else {
			int32_t t;
			*p++ = '-';
			for (t = i; t < j; ++t) *p++ = (uint8_t)"$acgtn"[st[t] & 7];
		}
	}
	return p;
}

static void sw_lens(int32_t n, const uint8_t *st, int64_t *mlen, int64_t *blen)
{
	int32_t i;
	int64_t m = 0;
	for (i = 0; i < n; ++i) m += st[i] >> 4 == 0;
	*mlen = m, *blen = n;
}

static void sw_stranded(const rb3h_sid_t *sid, const rb3h_pos_t *pos, int32_t rlen, int64_t *clen, int64_t *st, int64_t *en) /* pos_stranded, search.c:166-173 */
{
	*clen = sid->len[pos->sid >> 1];
	if ((pos->sid & 1) == 0) *st = pos->pos, *en = pos->pos + rlen;
	else *st = *clen - (pos->pos + rlen), *en = *clen - pos->pos;
}

int rb3h_sw_format_paf_at(rb3h_buf_t *out, const char *name, int64_t id, int64_t len, const uint8_t *seq, int64_t n, const rb3h_sw_hit_t *hits, const uint8_t *steps,
		const rb3h_pos_t *pos, const rb3h_sid_t *sid, int unmapped, int with_rs, const int32_t *qoff0, const int32_t *n_qoff)
{
	const int64_t l_name = name ? (int64_t)strlen(name) : 24;
	int64_t i, k;
	uint8_t *p;
	if (n == 0) {
		if (!unmapped) return 0;
		if (sw_reserve(out, l_name + 64) < 0) return -1;
		p = sw_name(out->s + out->l, name, id);
		*p++ = '\t', p = sw_num(p, len);
		p = sw_str(p, "\t*\t*\t*\t*\t*\t*\t*\t0\t0\t0\n");
		out->l = p - out->s;
		return 0;
	}
	for (i = 0; i < n; ++i) {
		const rb3h_sw_hit_t *h = hits + i;
		const uint8_t *st = steps + h->step_off;
		const rb3h_pos_t *hp = h->n_pos > 0 ? pos + h->pos_off : 0;
		const int64_t q0 = qoff0 ? qoff0[i] : 0; /* where the hit starts on the query: 0 end to end, the node's place in the local mode */
		int64_t mlen, blen, l_sn = 0;
		int32_t j;
		if (q0 < 0 || q0 + h->qlen > len) return -3;
		for (k = 0; k < h->n_pos; ++k) { /* (a string the name list does not know: the files do not belong together) */
			if (sid && (hp[k].sid < 0 || (hp[k].sid >> 1) >= sid->n_seq)) return -2;
			if (sid) l_sn += (int64_t)strlen(sid->name[hp[k].sid >> 1]);
		}
		if (sw_reserve(out, l_name + 512 + (int64_t)h->n_steps * 20 + l_sn + h->n_pos * 48) < 0) return -1;
		p = sw_name(out->s + out->l, name, id);
		*p++ = '\t', p = sw_num(p, len);
		*p++ = '\t', p = sw_num(p, q0);
		*p++ = '\t', p = sw_num(p, q0 + h->qlen);
		if (hp) {
			if (sid) {
				int64_t clen, s0, e0;
				sw_stranded(sid, hp, h->rlen, &clen, &s0, &e0);
				*p++ = '\t', *p++ = (uint8_t)"+-"[hp->sid & 1];
				*p++ = '\t', p = sw_str(p, sid->name[hp->sid >> 1]);
				*p++ = '\t', p = sw_num(p, clen);
				*p++ = '\t', p = sw_num(p, s0);
				*p++ = '\t', p = sw_num(p, e0);
			} else {
				p = sw_str(p, "\t+\t"), p = sw_num(p, hp->sid);
				p = sw_str(p, "\t*\t"), p = sw_num(p, hp->pos);
				*p++ = '\t', p = sw_num(p, hp->pos + h->rlen);
			}
		} else p = sw_str(p, "\t*\t*\t"), p = sw_num(p, h->rlen), p = sw_str(p, "\t*\t*");
		sw_lens(h->n_steps, st, &mlen, &blen);
		*p++ = '\t', p = sw_num(p, mlen);
		*p++ = '\t', p = sw_num(p, blen);
		p = sw_str(p, "\t0\tAS:i:"), p = sw_num(p, h->score);
		p = sw_str(p, "\tqh:i:"), p = sw_num(p, n_qoff ? n_qoff[i] : 1);
		p = sw_str(p, "\trh:i:"), p = sw_num(p, h->hi - h->lo);
		p = sw_str(p, "\tcg:Z:");
		for (j = 0; j < h->n_steps;) {
			int32_t e = j + 1;
			while (e < h->n_steps && st[e] >> 4 == st[j] >> 4) ++e;
			p = sw_num(p, e - j), *p++ = (uint8_t)"=XID"[st[j] >> 4 & 3];
			j = e;
		}
		p = sw_str(p, "\tcs:Z:"), p = sw_cs(p, seq + q0, h->n_steps, st);
		if (with_rs) {
			p = sw_str(p, "\trs:Z:");
			for (j = 0; j < h->n_steps; ++j)
				if (st[j] >> 4 != 2) *p++ = (uint8_t)"$ACGTN"[(st[j] & 7) < 5 ? (st[j] & 7) : 5];
		}
		if (h->n_pos > 1) {
			p = sw_str(p, sid ? "\tap:Z:" : "\taq:Z:");
			for (k = 1; k < h->n_pos; ++k) {
				if (sid) {
					int64_t clen, s0, e0;
					sw_stranded(sid, hp + k, h->rlen, &clen, &s0, &e0);
					p = sw_str(p, sid->name[hp[k].sid >> 1]);
					*p++ = ',', *p++ = (uint8_t)"+-"[hp[k].sid & 1], *p++ = ',';
					p = sw_num(p, s0), *p++ = ';';
				} else p = sw_num(p, hp[k].sid), *p++ = ',', p = sw_num(p, hp[k].pos), *p++ = ';';
			}
		}
		*p++ = '\n';
		out->l = p - out->s;
	}
	return 0;
}

int rb3h_sw_format_paf(rb3h_buf_t *out, const char *name, int64_t id, int64_t len, const uint8_t *seq, int64_t n, const rb3h_sw_hit_t *hits, const uint8_t *steps,
		const rb3h_pos_t *pos, const rb3h_sid_t *sid, int unmapped, int with_rs)
{
	return rb3h_sw_format_paf_at(out, name, id, len, seq, n, hits, steps, pos, sid, unmapped, with_rs, 0, 0);
}

int rb3h_sw_format_all(rb3h_buf_t *out, const char *name, int64_t id, int64_t len, const uint8_t *seq, int64_t n, const rb3h_sw_hit_t *hits, const uint8_t *steps,
		char strand, int64_t max_out)
{
	const int64_t l_name = name ? (int64_t)strlen(name) : 24;
	int64_t i, n_out = 0, tot = 0;
	uint8_t *p;
	if (max_out <= 0) max_out = INT64_MAX;
	for (i = 0; i < n; ++i) tot += hits[i].hi - hits[i].lo;
	for (i = 0; i < n; ++i) {
		n_out += hits[i].hi - hits[i].lo;
		if (n_out >= max_out) break;
	}
	if (sw_reserve(out, l_name + 160) < 0) return -1;
	p = sw_str(out->s + out->l, "QS\t"), p = sw_name(p, name, id);
	*p++ = '\t', p = sw_num(p, len);
	*p++ = '\t', p = sw_num(p, n);
	*p++ = '\t', *p++ = (uint8_t)strand;
	*p++ = '\t', p = sw_num(p, n_out);
	*p++ = '\t', p = sw_num(p, tot);
	*p++ = '\n';
	out->l = p - out->s;
	for (i = 0, n_out = 0; i < n; ++i) {
		const rb3h_sw_hit_t *h = hits + i;
		int64_t mlen, blen;
		if (sw_reserve(out, 128 + (int64_t)h->n_steps * 16) < 0) return -1;
		sw_lens(h->n_steps, steps + h->step_off, &mlen, &blen);
		p = sw_str(out->s + out->l, "QH\t"), p = sw_num(p, h->hi - h->lo);
		*p++ = '\t', p = sw_num(p, h->score);
		*p++ = '\t', p = sw_num(p, blen - mlen);
		*p++ = '\t', p = sw_cs(p, seq, h->n_steps, steps + h->step_off);
		*p++ = '\n';
		out->l = p - out->s;
		n_out += h->hi - h->lo;
		if (n_out >= max_out) break;
	}
	if (sw_reserve(out, 4) < 0) return -1;
	memcpy(out->s + out->l, "//\n", 3), out->l += 3;
	return 0;
}
