"""Python model of `sw -e`: the end-to-end BWA-SW dynamic program of a whole query against an FM-index with the backtrack kept.

It extends tests/sw_model.py (the model of `hapdiv`, left as it is) by two things:

  end_len   a mismatch, a gap of the index side (E) and the gap phase of the query side (F) are allowed only once end_len symbols of
            the query are aligned.  On a linear query every cell of row i has consumed i symbols, its parent i - 1, so the three tests
            of the reference collapse to one: row i is `inner` when i - 1 >= end_len.  sw_model.fill() has end_len 1 built in, so its
            row loop is restated here with that one line changed (fill);
  backtrack the walk from a cell of the last row to the root, one step per cell visited: the operation (= X I D) and the base of the
            index at that cell.  The first step is query position 0.  cigar, cs, rs, the matching and the block length follow from
            the steps alone (steps_of, cigar_of, cs_of, rs_of).

Lines: paf_line / unmapped_line (the PAF of `sw`), all_hits_block (the QS / QH / // blocks of --all-e2e and -g)."""
import heapq

from tests import sw_model as sw

OP_EQ, OP_X, OP_I, OP_D = 0, 1, 2, 3
OPS = "=XID"
DEFAULTS = dict(sw.DEFAULTS, end_len=11)
ALL_HEADER = b"CC\tQS  queryName  queryLen  numHap\nCC\tQH  refCount   score     editDist   cs   strand   nOut   totAln\nCC\n"


def fill(ix, seq, opt):
    """sw_model.fill with end_len: (rows, best score)"""
    o = dict(DEFAULTS)
    o.update(opt or {})
    N, ma, mi, go, ge, end_len = o["n_best"], o["match"], o["mis"], o["gap_open"], o["gap_ext"], o["end_len"]
    k = len(seq)
    rows = [[sw.Cell(0, ix.acc[6], 0)]] + [[] for _ in range(k)]
    tab = sw.SlotTable(N * 4)
    best = 0
    for i in range(1, k + 1):
        cq, prev = int(seq[k - i]), rows[i - 1]
        tab.clear()
        inner = i - 1 >= end_len                 # the one line that differs from sw_model.fill
        for col, p in enumerate(prev):
            pos = (i - 1) * N + col
            last_rc = 0
            ext = ix.extend(p.lo, p.hi, p.lo_rc)
            for c in range(1, 6):
                sc = ma if (c == cq and c != 5) else -mi
                l, h, rc = ext[c]
                if h == l or p.H + sc <= 0 or (c != cq and not inner):
                    continue
                last_rc = rc
                sw.merge(tab, sw.Cell(l, h, rc, H=p.H + sc, H_pos=pos))
            if p.H - go > p.E:
                ef, e = sw.OPEN, p.H - go
            else:
                ef, e = sw.EXT, p.E
            e -= ge
            if e > 0 and inner:
                sw.merge(tab, sw.Cell(p.lo, p.hi, last_rc, H=e, E=e, H_from=sw.FROM_E, E_from=ef, E_pos=pos))
        if tab.count == 0:
            continue
        row = sw.top_cells(tab, N)
        fpar = []
        if inner and prev:
            heap = [c.H for c in row]
            heapq.heapify(heap)
            stack = [c.copy() for c in reversed(row) if c.H > go + ge]
            while stack:
                z = stack.pop()
                low = 0 if len(heap) < N else heap[0]
                if z.H - go > z.F:
                    ff, f = sw.OPEN, z.H - go
                else:
                    ff, f = sw.EXT, z.F
                f -= ge
                if f <= low:
                    continue
                ext = ix.extend(z.lo, z.hi, z.lo_rc)
                for c in range(1, 6):
                    l, h, rc = ext[c]
                    if h == l:
                        continue
                    q, ch = sw.merge(tab, sw.Cell(l, h, rc, H=f, F=f, H_from=sw.FROM_F, F_from=ff))
                    if ch & 4:
                        if len(heap) < N:
                            heapq.heappush(heap, f)
                        elif f > heap[0]:
                            heapq.heapreplace(heap, f)
                        fpar.append((z.lo, z.hi))
                        q.F_from, q.F_par = ff, len(fpar) - 1
                        if f - ge > low:
                            stack.append(q.copy())
        row = sw.top_cells(tab, N)
        if fpar:
            where = {(c.lo, c.hi): j for j, c in enumerate(row)}
            for c in row:
                if c.F == 0 or c.F_par == sw.UNSET:
                    continue
                j = where.get(fpar[c.F_par])
                if j is None:
                    c.F_par = sw.UNSET
                else:
                    c.F_par, c.F_set = j, 1
        rows[i] = row
        best = max(best, row[0].H)
        if i == k:
            kept = []
            for c in row:
                if any((q.lo_rc <= c.lo_rc and q.lo_rc + (q.hi - q.lo) >= c.lo_rc + (c.hi - c.lo)) or (q.lo <= c.lo and q.hi >= c.hi) for q in kept):
                    c.flt = 1
                else:
                    kept.append(c)
    return rows, best


def steps_of(ix, rows, seq, N, pos):
    """[(op, reference base)] of the walk from cell `pos` (row * N + column) back to the root; the first step is query position 0"""
    k, out, last = len(seq), [], 0
    while pos > 0:
        r = pos // N
        p = rows[r][pos % N]
        state = p.H_from if last == 0 else last
        ext = (p.E_from if state == sw.FROM_E else p.F_from) if state in (sw.FROM_E, sw.FROM_F) else 0
        base = ix.base_of(p.lo)
        if state == sw.FROM_H:
            out.append((OP_EQ if base == int(seq[k - r]) else OP_X, base))
            pos = p.H_pos
        elif state == sw.FROM_E:
            out.append((OP_I, base))
            pos = p.E_pos
        else:
            if p.F == 0 or not p.F_set:
                raise sw.Unrepresentable()
            out.append((OP_D, base))
            pos = r * N + p.F_par
        last = state if ext else 0
    return out


def align(ix, seq, opt=None):
    """the hits of one query (symbols 1..5) in the reference's order: [dict(lo, hi, score, steps)]"""
    o = dict(DEFAULTS)
    o.update(opt or {})
    N = o["n_best"]
    if len(seq) == 0:
        return []
    rows, best = fill(ix, seq, o)
    last = rows[len(seq)]
    if best < o["min_sc"] or not last:
        return []
    h0, out = last[0].H, []
    for j, c in enumerate(last):
        if c.flt or c.H_from != sw.FROM_H or c.H < o["min_sc"] or (o["e2e_drop"] >= 0 and h0 - c.H > o["e2e_drop"]):
            continue
        out.append(dict(lo=c.lo, hi=c.hi, score=c.H, steps=steps_of(ix, rows, seq, N, len(seq) * N + j)))
    return out


def cigar_of(steps):
    """([(length, op)], mlen, blen)"""
    runs = []
    for op, _ in steps:
        if runs and runs[-1][1] == op:
            runs[-1][0] += 1
        else:
            runs.append([1, op])
    return [(n, op) for n, op in runs], sum(n for n, op in runs if op == OP_EQ), sum(n for n, op in runs)


def rs_of(steps):
    return "".join("$ACGTN"[b] for op, b in steps if op != OP_I)


def cs_of(steps, seq):
    out, y, i = [], 0, 0
    while i < len(steps):
        j = i
        while j < len(steps) and steps[j][0] == steps[i][0]:
            j += 1
        op = steps[i][0]
        if op == OP_EQ:
            out.append(":%d" % (j - i))
            y += j - i
        elif op == OP_X:
            for t in range(i, j):
                out.append("*%c%c" % ("$acgtn"[int(seq[y])], "$acgtn"[steps[t][1]]))
                y += 1
        elif op == OP_I:
            out.append("+" + "".join("$acgtn"[int(seq[y + t])] for t in range(j - i)))
            y += j - i
        else:
            out.append("-" + "".join("$acgtn"[steps[t][1]] for t in range(i, j)))
        i = j
    return "".join(out)


def lens_of(steps):
    """(qlen, rlen)"""
    return sum(1 for op, _ in steps if op != OP_D), sum(1 for op, _ in steps if op != OP_I)


def n_positions(hits, max_pos):
    """how many positions every hit of a query gets: rest = max_pos at the first hit, n = rest if rest > 0 else 1, less what was found"""
    rest, out = max_pos, []
    for h in hits:
        n = min(rest if rest > 0 else 1, h["hi"] - h["lo"])
        out.append(n)
        rest -= n
    return out


def _name(name, qid):
    return name if name is not None else "seq%d" % (qid + 1)


def paf_line(name, qid, seq, hit, pos=None, names=None, lengths=None, with_rs=False):
    """pos: [(sid, pos)] of the hit (None or empty: no position); names / lengths: of the indexed sequences (None: no name list)"""
    steps = hit["steps"]
    qlen, rlen = lens_of(steps)
    runs, mlen, blen = cigar_of(steps)
    f = [_name(name, qid), str(len(seq)), "0", str(qlen)]

    def stranded(p):
        clen = lengths[p[0] >> 1]
        return (clen, p[1], p[1] + rlen) if p[0] & 1 == 0 else (clen, clen - (p[1] + rlen), clen - p[1])

    if pos:
        sid, at = pos[0]
        if names is not None:
            clen, st, en = stranded(pos[0])
            f += ["+-"[sid & 1], names[sid >> 1], str(clen), str(st), str(en)]
        else:
            f += ["+", str(sid), "*", str(at), str(at + rlen)]
    else:
        f += ["*", "*", str(rlen), "*", "*"]
    f += [str(mlen), str(blen), "0", "AS:i:%d" % hit["score"], "qh:i:1", "rh:i:%d" % (hit["hi"] - hit["lo"]),
          "cg:Z:" + "".join("%d%s" % (n, OPS[op]) for n, op in runs), "cs:Z:" + cs_of(steps, seq)]
    if with_rs:
        f.append("rs:Z:" + rs_of(steps))
    if pos and len(pos) > 1:
        if names is not None:
            f.append("ap:Z:" + "".join("%s,%s,%d;" % (names[p[0] >> 1], "+-"[p[0] & 1], stranded(p)[1]) for p in pos[1:]))
        else:
            f.append("aq:Z:" + "".join("%d,%d;" % p for p in pos[1:]))
    return ("\t".join(f) + "\n").encode()


def unmapped_line(name, qid, seq):
    return ("%s\t%d\t*\t*\t*\t*\t*\t*\t*\t0\t0\t0\n" % (_name(name, qid), len(seq))).encode()


def all_hits_block(name, qid, seq, hits, strand, max_out=0):
    """seq: the symbols that were aligned (the reverse complement for the `-` block: its cs is written from them)"""
    cap = max_out if max_out > 0 else 1 << 62
    tot = sum(h["hi"] - h["lo"] for h in hits)
    n_out = 0
    for h in hits:
        n_out += h["hi"] - h["lo"]
        if n_out >= cap:
            break
    out = ["QS\t%s\t%d\t%d\t%s\t%d\t%d\n" % (_name(name, qid), len(seq), len(hits), strand, n_out, tot)]
    n_out = 0
    for h in hits:
        _, mlen, blen = cigar_of(h["steps"])
        out.append("QH\t%d\t%d\t%d\t%s\n" % (h["hi"] - h["lo"], h["score"], blen - mlen, cs_of(h["steps"], seq)))
        n_out += h["hi"] - h["lo"]
        if n_out >= cap:
            break
    out.append("//\n")
    return "".join(out).encode()


def revcomp6(seq):
    return [5 - int(c) if 1 <= int(c) <= 4 else int(c) for c in reversed(seq)]
