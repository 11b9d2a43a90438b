/*
 * sidefile.c -- the two files `mem -p` needs beside an index: <index>.ssa, the sampled suffix array as rb3_ssa_dump writes it
 * (ssa.c:198-213), and <index>.len.gz, the names and lengths of the indexed sequences (rb3_sid_read, io.c:161-204).
 */
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include "rb3host.h"

void rb3h_ssa_destroy(rb3h_ssa_t *sa)
{
	if (sa == 0) return;
	free(sa->r2i); free(sa->ssa); free(sa);
}

/* magic "SSA\1", ss and ms (4 bytes each), m and n_ssa (8 bytes each): 28 bytes; then r2i[m] and ssa[n_ssa].  Unlike rb3_ssa_restore
 * (ssa.c:215-241), which does not look at what fread returns, a file that ends early is refused: its samples would be noise */
rb3h_ssa_t *rb3h_ssa_read(const char *fn)
{
	FILE *fp;
	char magic[4];
	uint32_t y[2];
	rb3h_ssa_t *sa;
	if (fn == 0 || (fp = fopen(fn, "rb")) == 0) return 0;
	sa = (rb3h_ssa_t*)calloc(1, sizeof(*sa));
	if (sa == 0) { fclose(fp); return 0; }
	if (fread(magic, 1, 4, fp) != 4 || memcmp(magic, "SSA\1", 4) != 0 || fread(y, 4, 2, fp) != 2 || fread(&sa->m, 8, 1, fp) != 1 || fread(&sa->n_ssa, 8, 1, fp) != 1
			|| sa->m < 0 || sa->n_ssa < 0 || y[0] > 62 || y[1] > 63) goto fail;
	sa->ss = (int32_t)y[0], sa->ms = (int32_t)y[1];
	{ /* the arrays must be in the file before memory is asked for them */
		long at = ftell(fp), end;
		if (at < 0 || fseek(fp, 0, SEEK_END) != 0 || (end = ftell(fp)) < 0 || fseek(fp, at, SEEK_SET) != 0) goto fail;
		if ((uint64_t)(end - at) / 8 < (uint64_t)sa->m + (uint64_t)sa->n_ssa) goto fail;
	}
	sa->r2i = (uint64_t*)calloc((size_t)(sa->m > 0 ? sa->m : 1), 8);
	sa->ssa = (uint64_t*)calloc((size_t)(sa->n_ssa > 0 ? sa->n_ssa : 1), 8);
	if (sa->r2i == 0 || sa->ssa == 0) goto fail;
	if (fread(sa->r2i, 8, (size_t)sa->m, fp) != (size_t)sa->m || fread(sa->ssa, 8, (size_t)sa->n_ssa, fp) != (size_t)sa->n_ssa) goto fail;
	fclose(fp);
	return sa;
fail:
	fclose(fp);
	rb3h_ssa_destroy(sa);
	return 0;
}

void rb3h_sid_destroy(rb3h_sid_t *sl)
{
	int64_t i;
	if (sl == 0) return;
	for (i = 0; i < sl->n_seq; ++i) free(sl->name[i]);
	free(sl->name); free(sl->len); free(sl);
}

/* one line: the name is what stands before the first blank or tab, the length what stands between that and the next one (atol); a line
 * with one field only or a length <= 0 is skipped.  Every blank ends a field: "a  5" has an empty second field and is skipped */
static int sid_line(rb3h_sid_t *sl, int64_t *m_seq, char *s)
{
	char *p, *q, *name = 0;
	int64_t len = -1;
	int i;
	for (p = q = s, i = 0;; ++p) {
		if (*p == ' ' || *p == '\t' || *p == 0) {
			const int c = *p;
			*p = 0;
			if (i == 0) name = q;
			else if (i == 1) len = atol(q);
			++i, q = p + 1;
			if (c == 0 || i == 2) break;
		}
	}
	if (i != 2 || len <= 0) return 0;
	if (sl->n_seq == *m_seq) {
		const int64_t m = *m_seq ? *m_seq * 2 : 16;
		char **nn = (char**)realloc(sl->name, (size_t)m * sizeof(char*));
		int64_t *nl;
		if (nn == 0) return -1;
		sl->name = nn;
		nl = (int64_t*)realloc(sl->len, (size_t)m * 8);
		if (nl == 0) return -1;
		sl->len = nl, *m_seq = m;
	}
	if ((sl->name[sl->n_seq] = strdup(name)) == 0) return -1;
	sl->len[sl->n_seq++] = len;
	return 0;
}

rb3h_sid_t *rb3h_sid_read(const char *fn)
{
	gzFile fp;
	rb3h_sid_t *sl;
	int64_t m_seq = 0, l = 0, m = 0;
	char *line = 0, buf[65536];
	int n, i, err = 0;
	if (fn == 0 || (fp = gzopen(fn, "r")) == 0) return 0;
	sl = (rb3h_sid_t*)calloc(1, sizeof(*sl));
	if (sl == 0) { gzclose(fp); return 0; }
	while (!err && (n = gzread(fp, buf, sizeof(buf))) > 0) {
		for (i = 0; i < n && !err; ++i) {
			if (l + 2 > m) {
				char *t;
				m = m ? m * 2 : 256;
				if ((t = (char*)realloc(line, (size_t)m)) == 0) { err = 1; break; }
				line = t;
			}
			if (buf[i] == '\n') {
				if (l > 0 && line[l - 1] == '\r') --l; /* (ks_getuntil with KS_SEP_LINE drops it too) */
				line[l] = 0;
				if (sid_line(sl, &m_seq, line) < 0) err = 1;
				l = 0;
			} else line[l++] = buf[i];
		}
	}
	if (!err && l > 0) { /* a last line without its newline */
		line[l] = 0;
		if (sid_line(sl, &m_seq, line) < 0) err = 1;
	}
	if (n < 0) err = 1;
	free(line);
	gzclose(fp);
	if (err) { rb3h_sid_destroy(sl); return 0; }
	return sl;
}
