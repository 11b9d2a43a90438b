/* misc.c -- number parsing and timers (restates misc.c:7-16, 116-150 of the reference) */
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <sys/resource.h>
#include <sys/time.h>
#include "rb3host.h"

int rb3h_verbose = 3;
static double rb3h_t0 = 0;

int64_t rb3h_parse_num(const char *str) /* "7g", "500k", "2.5M" */
{
	char *p;
	double x = strtod(str, &p);
	if (*p == 'G' || *p == 'g') x *= 1e9;
	else if (*p == 'M' || *p == 'm') x *= 1e6;
	else if (*p == 'K' || *p == 'k') x *= 1e3;
	return (int64_t)(x + .499);
}

/* an argument of `remove`: a number `A` or an inclusive range `A-B` (A <= B), decimal digits only, each below 2^62; nothing in front, between or behind
 * (so no sign, no blank, no empty side).  0 and (*a, *b), or -1: nothing is guessed */
int rb3h_parse_rows(const char *str, int64_t *a, int64_t *b)
{
	int64_t v[2] = { 0, 0 };
	int i = 0, nd = 0;
	const char *p;
	if (str == 0) return -1;
	for (p = str; *p; ++p) {
		if (*p >= '0' && *p <= '9') {
			if (v[i] > ((int64_t)1 << 58)) return -1;
			v[i] = v[i] * 10 + (*p - '0'), ++nd;
		} else if (*p == '-' && i == 0 && nd > 0) i = 1, nd = 0;
		else return -1;
	}
	if (nd == 0) return -1;
	if (i == 0) v[1] = v[0];
	if (v[1] < v[0]) return -1;
	*a = v[0], *b = v[1];
	return 0;
}

/* digits only, below 2^62, up to `end`; the value, or -1 for anything else (an empty field included) */
static int64_t region_num(const char *p, const char *end)
{
	int64_t v = 0;
	if (p >= end) return -1;
	for (; p < end; ++p) {
		if (*p < '0' || *p > '9' || v > ((((int64_t)1 << 62) - 1) - (*p - '0')) / 10) return -1;
		v = v * 10 + (*p - '0');
	}
	return v;
}

/* a region of `fetch`, 0-based and end-exclusive.  bed == 0: the word `name:beg-end`, optionally followed by `:+` or `:-`; the name is cut at the LAST colons,
 * so it may hold colons itself.  bed != 0: a BED line -- tab-separated columns 1-3, the strand from column 6 if there is one (`+`, `-`, or `.` for none); a
 * line end behind it is passed over.  The name is str[0, name_len) and is not empty; beg < end, both decimal digits only and below 2^62; strand +1 or -1, stranded 1 if the region names its strand.
 * 0, or -1: nothing is guessed */
int rb3h_region_parse(const char *str, int bed, rb3h_region_t *r)
{
	const char *e, *c, *d;
	if (str == 0 || r == 0) return -1;
	e = str + strlen(str);
	r->strand = 1, r->stranded = 0;
	if (bed) {
		const char *col[8];
		int n = 1;
		while (e > str && (e[-1] == '\n' || e[-1] == '\r')) --e;
		col[0] = str;
		for (c = str; c < e; ++c)
			if (*c == '\t') { if (n < 7) col[n] = c + 1; ++n; }
		if (n < 3) return -1;
		if (n < 7) col[n] = e + 1; /* (the end of the last column, as if a tab stood there) */
		r->name_len = col[1] - 1 - str;
		r->beg = region_num(col[1], col[2] - 1), r->end = region_num(col[2], col[3] - 1);
		if (n >= 6) {
			if (col[6] - 1 - col[5] != 1) return -1;
			if (*col[5] == '-') r->strand = -1, r->stranded = 1;
			else if (*col[5] == '+') r->stranded = 1;
			else if (*col[5] != '.') return -1;
		}
	} else {
		if (e - str >= 2 && e[-2] == ':' && (e[-1] == '+' || e[-1] == '-')) r->strand = e[-1] == '-' ? -1 : 1, r->stranded = 1, e -= 2;
		for (c = e; c > str && c[-1] != ':'; --c) {}
		if (c == str) return -1; /* no colon */
		for (d = c; d < e && *d != '-'; ++d) {}
		if (d == e) return -1; /* no dash */
		r->name_len = c - 1 - str;
		r->beg = region_num(c, d), r->end = region_num(d + 1, e);
	}
	if (r->name_len <= 0 || r->beg < 0 || r->end < 0 || r->beg >= r->end) return -1;
	return 0;
}

double rb3h_cputime(void)
{
	struct rusage r;
	getrusage(RUSAGE_SELF, &r);
	return r.ru_utime.tv_sec + r.ru_stime.tv_sec + 1e-6 * (r.ru_utime.tv_usec + r.ru_stime.tv_usec);
}

static double wall(void)
{
	struct timeval tp;
	gettimeofday(&tp, 0);
	return tp.tv_sec + tp.tv_usec * 1e-6;
}

void rb3h_init(void) { rb3h_t0 = wall(); }
double rb3h_realtime(void) { return wall() - rb3h_t0; }

double rb3h_percent_cpu(void)
{
	double rt = rb3h_realtime();
	return rt > 0 ? (rb3h_cputime() + 1e-6) / (rt + 1e-6) : 0;
}

long rb3h_peakrss(void)
{
	struct rusage r;
	getrusage(RUSAGE_SELF, &r);
	return r.ru_maxrss * 1024;
}
