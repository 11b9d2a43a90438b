"""Python model of `mem` (super-maximal exact matches), written from the definition on the STRINGS of the index rather than from the
FM-index walk:

- the index holds strings (both strands of every record); occ(p) is the number of places p occurs in them, never across a string end;
- for a query q and a start x, e(x) is the largest end with occ(q[x:e]) >= min_occ (e(x) = x if even q[x] is rarer): occ only falls
  as a pattern grows, so e is found by extending, and e(x) never decreases along x;
- (x, e(x)) is a match if it is at least min_len long and e(x) > e(x - 1), i.e. it lies in no match that starts earlier (one that
  starts later ends later or is shorter); its size is occ(q[x:e(x)]);
- the one exception is the reference's -l1: it never checks a single symbol against min_occ, so a position x with e(x) = x is reported
  as (x, x + 1) with whatever size q[x] has, zero included (no match can contain such a position).

occ comes from a suffix array of the text (prefix doubling in numpy) and a binary search per pattern: fine for texts of some 10^5
symbols and patterns of a few thousand."""
import numpy as np

from tests import kount_model as km

MEM_REC = np.dtype([("query", "<i8"), ("x0", "<i8"), ("size", "<i8"), ("st", "<i4"), ("en", "<i4")])


class Text:
    """the strings of an index (symbol arrays 1..5, no sentinel) as one searchable text"""

    def __init__(self, strings):
        parts = []
        for s in strings:
            parts += [np.asarray(s, dtype=np.uint8), np.zeros(1, dtype=np.uint8)]
        t = np.concatenate(parts) if parts else np.zeros(1, dtype=np.uint8)
        self.t = t.tobytes()
        n = t.size
        rank = t.astype(np.int64)
        sa = np.argsort(rank, kind="stable")
        k = 1
        while k < n:
            nxt = np.zeros(n, dtype=np.int64)
            nxt[:n - k] = rank[k:] + 1
            key = rank * (n + 2) + nxt
            sa = np.argsort(key, kind="stable")
            ks = key[sa]
            r = np.concatenate([[0], np.cumsum(ks[1:] != ks[:-1])])
            rank = np.empty(n, dtype=np.int64)
            rank[sa] = r
            if r[-1] == n - 1:
                break
            k *= 2
        self.sa = sa.tolist()

    def occ(self, p):
        """the number of occurrences of pattern p (bytes of symbols 1..5)"""
        t, sa, m = self.t, self.sa, len(p)
        lo, hi = 0, len(sa)
        while lo < hi:                       # the first suffix whose first m symbols are >= p
            mid = (lo + hi) // 2
            if t[sa[mid]:sa[mid] + m] < p:
                lo = mid + 1
            else:
                hi = mid
        first, hi = lo, len(sa)
        while lo < hi:                       # the first one whose first m symbols are > p
            mid = (lo + hi) // 2
            if t[sa[mid]:sa[mid] + m] <= p:
                lo = mid + 1
            else:
                hi = mid
        return lo - first


def both_strands(records):
    """the strings an index built from `records` with both strands holds"""
    out = []
    for r in records:
        r = np.asarray(r, dtype=np.uint8)
        rc = r[::-1].copy()
        m = (rc >= 1) & (rc <= 4)
        rc[m] = 5 - rc[m]
        out += [r, rc]
    return out


def matches(text, q, min_len, min_occ):
    """[(st, en, size)] of query q (symbols 1..5) against a Text, in the reference's order"""
    q = bytes(bytearray(np.asarray(q, dtype=np.uint8).tolist()))
    n, out, e, prev_e = len(q), [], 0, 0
    for x in range(n):
        e = max(e, x)
        while e < n and text.occ(q[x:e + 1]) >= min_occ:
            e += 1
        if e == x:
            if min_len == 1:
                out.append((x, x + 1, text.occ(q[x:x + 1])))
        elif e - x >= min_len and e > prev_e:
            out.append((x, e, text.occ(q[x:e])))
        prev_e = max(prev_e, e)
    return out


def mem(strings, queries, min_len, min_occ):
    """the records (MEM_REC without x0) of the queries against the index that holds `strings`"""
    text = strings if isinstance(strings, Text) else Text(strings)
    rows = []
    for i, q in enumerate(queries):
        rows += [(i, 0, size, st, en) for st, en, size in matches(text, q, min_len, min_occ)]
    return np.array(rows, dtype=MEM_REC) if rows else np.zeros(0, dtype=MEM_REC)


def lines(recs, names=None, first_id=0):
    """the reference's output bytes for records (names[q] or seq<first_id + q + 1>)"""
    out = []
    for r in recs:
        q = int(r["query"])
        nm = names[q] if names is not None and names[q] is not None else "seq%d" % (first_id + q + 1)
        out.append(b"%s\t%d\t%d\t%d\n" % (nm.encode() if isinstance(nm, str) else nm, r["st"], r["en"], r["size"]))
    return b"".join(out)


def gaps(recs_of_query, length, min_gap):
    """[(st, en)] of the stretches of at least min_gap symbols of a query of `length` that none of its matches covers"""
    covered = np.zeros(length + 1, dtype=bool)
    for r in recs_of_query:
        covered[r["st"]:r["en"]] = True
    out, x = [], 0
    while x < length:
        if covered[x]:
            x += 1
            continue
        y = x
        while y < length and not covered[y]:
            y += 1
        if y - x >= min_gap:
            out.append((x, y))
        x = y
    return out


def coverage(recs_of_query, length):
    covered = np.zeros(length + 1, dtype=bool)
    for r in recs_of_query:
        covered[r["st"]:r["en"]] = True
    return int(covered[:length].sum())


def read_queries(path, is_line=False):
    """[(name or None, characters as bytes)] of a FASTA / FASTQ file or a file of lines, gzip or not, as the reference reads them"""
    import gzip
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    ls = raw.split(b"\n")
    if ls and ls[-1] == b"":
        ls.pop()
    ls = [l[:-1] if len(l) > 1 and l.endswith(b"\r") else l for l in ls]
    if is_line:
        return [(None, l) for l in ls]
    out, i = [], 0
    while i < len(ls):
        if not ls[i][:1] in (b">", b"@"):
            i += 1
            continue
        fq = ls[i][:1] == b"@"
        name = ls[i][1:].split()[0] if ls[i][1:].split() and not ls[i][1:2].isspace() else b""
        i += 1
        seq = []
        while i < len(ls) and ls[i][:1] not in (b">", b"+", b"@"):
            seq.append(ls[i])
            i += 1
        s = b"".join(seq)
        if i < len(ls) and ls[i][:1] == b"+":
            i += 1
            got = 0
            while i < len(ls) and got < len(s):
                got += len(ls[i])
                i += 1
        out.append((name.decode(), s))
        del fq
    return out


NT6 = np.full(256, 5, dtype=np.uint8)
NT6[:5] = np.arange(5)
for _i, _c in enumerate(b"ACGT"):
    NT6[_c] = NT6[_c + 32] = _i + 1


def nt6(s):
    return NT6[np.frombuffer(s, dtype=np.uint8)]


def index_strings(golden_dir, name, cli):
    """the strings of a committed index (from its plain BWT)"""
    return km.strings_of(km.golden_plain(golden_dir, name, cli))
