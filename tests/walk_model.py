"""Python model of the two plain walks over an FM-index, `suffix` and `get`, on a plain BWT (symbols 0..5 = $ACGTN): the index is nothing but
the cumulative counts of every symbol (occ[c][k] = #{i < k : B[i] = c}, C[c] = #symbols < c), and the two loops are restated as they are
defined -- many walks side by side, one numpy step for all of them:

- suffix: from the interval of all rows, extend by the query's symbols from the last one leftwards (k, l <- C[c] + occ[c][k], C[c] + occ[c][l]);
  the first symbol that empties the interval stays outside: start = its position + 1, size = the interval before it (0 if none was taken);
- get: from row k follow LF (k <- C[B[k]] + occ[B[k]][k]) until B[k] is the sentinel; the symbols met, reversed, are the string, and the row
  where the walk stopped is the end row.  A row outside [0, n) has no string and end row -1."""
import numpy as np

from tests import mem_model as mm

LETTERS = np.frombuffer(b"$ACGTN", dtype=np.uint8)


class Fm:
    def __init__(self, bwt):
        self.b = np.ascontiguousarray(bwt, dtype=np.uint8)
        self.n = int(self.b.size)
        self.acc = np.concatenate([[0], np.cumsum(np.bincount(self.b, minlength=6))]).astype(np.int64)
        self.occ = np.zeros((6, self.n + 1), dtype=np.int64 if self.n >= 2 ** 31 else np.int32)
        for c in range(6):
            np.cumsum(self.b == c, out=self.occ[c, 1:])

    def suffix(self, queries):
        """(start, length, size) int64 arrays, one entry per query (uint8 arrays of nt6 codes)"""
        nq = len(queries)
        length = np.array([q.size for q in queries], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(length)])
        sym = np.minimum(np.concatenate(queries), 5) if nq and off[-1] else np.zeros(0, dtype=np.uint8)
        k, l = np.zeros(nq, dtype=np.int64), np.full(nq, self.n, dtype=np.int64)
        i, size = length - 1, np.zeros(nq, dtype=np.int64)
        live = np.flatnonzero(i >= 0)
        while live.size:
            c = sym[off[live] + i[live]].astype(np.int64)
            nk, nl = self.acc[c] + self.occ[c, k[live]], self.acc[c] + self.occ[c, l[live]]
            hit = nl > nk
            on = live[hit]
            k[on], l[on], size[on] = nk[hit], nl[hit], (nl - nk)[hit]
            i[on] -= 1
            live = on[i[on] >= 0]
        return i + 1, length, size

    def retrieve(self, rows):
        """(end_rows int64, [uint8 array of nt6 codes in text order per row])"""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        end = np.full(rows.size, -1, dtype=np.int64)
        ids = np.flatnonzero((rows >= 0) & (rows < self.n))
        k = rows[ids]
        got_id, got_sym = [], []
        while ids.size:
            c = self.b[k]
            stop = c == 0
            end[ids[stop]] = k[stop]
            ids, k, c = ids[~stop], k[~stop], c[~stop].astype(np.int64)
            got_id.append(ids), got_sym.append(c.astype(np.uint8))
            k = self.acc[c] + self.occ[c, k]
        seqs = [np.zeros(0, dtype=np.uint8)] * rows.size
        if got_id:
            gid, gsym = np.concatenate(got_id), np.concatenate(got_sym)
            o = np.argsort(gid, kind="stable")        # per row in walk order; the string is the walk reversed
            cnt = np.bincount(gid, minlength=rows.size)
            for r, s in zip(range(rows.size), np.split(gsym[o], np.cumsum(cnt)[:-1])):
                seqs[r] = s[::-1].copy()
        return end, seqs


def suffix_text(fm, files, is_line):
    """the bytes of `suffix [-L] <index> files...`: files are paths, read as the reference reads them (tests/mem_model.read_queries)"""
    out, n_rec = [], 0
    for f in files:
        qs = mm.read_queries(f, is_line)
        start, length, size = fm.suffix([mm.nt6(s) for _, s in qs])
        for j, (name, _) in enumerate(qs):
            nm = name.encode() if name is not None else b"seq%d" % (n_rec + j + 1)
            out.append(b"%s\t%d\t%d\t%d\n" % (nm, start[j], length[j], size[j]))
        n_rec += len(qs)
    return b"".join(out)


def get_text(fm, rows):
    """the bytes of `get <index> rows...`"""
    end, seqs = fm.retrieve(rows)
    return b"".join(b">%d %d\n" % (int(k), int(e)) + LETTERS[s].tobytes() + b"\n" for k, e, s in zip(rows, end, seqs) if e >= 0)
