"""The reference's MEM pre-filter of `sw -j`, restated over the cumulative counts of a BwtIndex (tests/sw_model.py): does a stretch of
min_len symbols of the query occur in the index (rb3_fmd_smem_present, fm-index.c:530-538, over rb3_fmd_smem1_TG with check_long,
fm-index.c:483-498)?

A window of min_len symbols that starts at x is walked from its last symbol to its first, one backward extension a step; only the size
of the interval is looked at, so one strand's interval [lo, hi) is all that is kept.  Where the extension by q[i] leaves nothing, the
next window starts at i + 1: every window in between holds q[i .. x + min_len - 1], which does not occur.  A window that reaches its
first symbol is a seed.  All six codes are extended as they come: an N matches an indexed N."""


def present(ix, q, min_len, a=0, b=None):
    """(1 if a window that starts in [a, b) occurs else 0, extension steps); b None: every start.  min_len >= 2"""
    assert min_len >= 2
    q = [min(int(c), 5) for c in q]
    n, x, steps = len(q), a, 0
    while True:
        if n - x < min_len or (b is not None and x >= b):    # fm-index.c:489, or the end of a walker's range of starts
            return 0, steps
        c = q[x + min_len - 1]
        lo, hi = ix.acc[c], ix.acc[c + 1]                    # rb3_fmd_set_intv: no rank
        i = x + min_len - 2
        while i >= x:
            c = q[i]
            steps += 1
            lo, hi = ix.acc[c] + ix.cum[c][lo], ix.acc[c] + ix.cum[c][hi]
            if hi - lo < 1:
                break
            i -= 1
        if i < x:
            return 1, steps
        x = i + 1


def present_chunked(ix, q, min_len, chunk):
    """the OR over walkers of `chunk` window starts each: the same answer as present() whatever the chunk"""
    n_start = len(q) - min_len + 1
    return int(any(present(ix, q, min_len, a, min(a + chunk, n_start))[0] for a in range(0, max(n_start, 0), chunk)))


def brute(strings, q, min_len):
    """some window of min_len symbols of q is a substring of one of the strings (lists of codes 1..5, both strands if the index holds both)"""
    texts = [bytes(s) for s in strings]
    qb = bytes(min(int(c), 5) for c in q)
    return int(any(any(qb[x:x + min_len] in t for t in texts) for x in range(len(qb) - min_len + 1)))
