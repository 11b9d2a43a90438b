"""Python model of `sw --local`: BWA-SW local alignment of a query against an FM-index over the query's DAWG, restated from its behaviour.

Two parts are new against tests/swaln_model.py (the model of `sw -e`, left as it is):

  dawg      the directed acyclic word graph of the query: one node per distinct interval of the query's own suffix array that a backward
            search can reach, an edge W -> cW per backward extension.  Symbols above 4 count as A when the query is indexed, so a node
            reached over an N carries symbol 1.  The NUMBER of a node decides the order of everything after it, and it comes from a stack
            traversal: in-degrees first, then a node gets the next number at the moment its last incoming edge is seen (children 3..0, the
            stack last in first out).  Predecessor lists are filled by ascending node, children 0..3;
  fill      the dynamic program with a row per node: candidates come from the cells of ALL predecessors in list order, a cut (max_min_sc)
            drops cells that cannot reach the best n_best of a node with several predecessors, every cell carries how many symbols of the
            query it has consumed (qlen, the maximum over what merged into it), and mismatches and gaps are allowed by that number.  The F
            phase of a node runs iff the LAST predecessor cell the loops visited has consumed end_len symbols.

The one hit of a query is column 0 of the first node whose best score is above every earlier node's, if that score reaches min_sc.  Its walk
back to the root is that of swaln_model with rows named by node and `=` decided against the node's symbol."""
import heapq

from tests import sw_model as sw
from tests import swaln_model as swaln

DEFAULTS = dict(swaln.DEFAULTS)


class Dawg:
    __slots__ = ("n_node", "sym", "pre", "qoff0", "n_qoff", "sa")


def suffix_array(s8):
    """sa[0] = len, then the suffixes in order"""
    b = bytes(s8)
    return [len(b)] + sorted(range(len(b)), key=lambda i: b[i:])


def dawg(seq):
    n = len(seq)
    s8 = [1 if int(c) >= 5 else int(c) for c in seq]
    sa = suffix_array(s8)
    cum = [[0] * (n + 2) for _ in range(4)]           # cum[c][k]: rows [0, k) of the BWT that hold symbol c + 1 (the $ row holds none)
    cnt = [0] * 4
    for i in range(n + 1):
        for c in range(4):
            cum[c][i] = cnt[c]
        if sa[i] > 0:
            cnt[s8[sa[i] - 1] - 1] += 1
    for c in range(4):
        cum[c][n + 1] = cnt[c]
    acc = [1]
    for c in range(3):
        acc.append(acc[-1] + cnt[c])

    def children(lo, hi, order):
        for c in order:
            l, h = acc[c] + cum[c][lo], acc[c] + cum[c][hi]
            if l != h:
                yield c, l, h

    root = (0, n + 1)
    deg = {root: 0}
    stack = [root]
    while stack:
        lo, hi = stack.pop()
        for c, l, h in children(lo, hi, (3, 2, 1, 0)):
            if (l, h) not in deg:
                deg[(l, h)] = 0
                stack.append((l, h))
            deg[(l, h)] += 1
    ident, seen = {root: 0}, dict.fromkeys(deg, 0)
    nodes, sym = [root], [0]
    stack = [root]
    while stack:
        lo, hi = stack.pop()
        for c, l, h in children(lo, hi, (3, 2, 1, 0)):
            seen[(l, h)] += 1
            if seen[(l, h)] == deg[(l, h)]:
                ident[(l, h)] = len(nodes)
                nodes.append((l, h))
                sym.append(c + 1)
                stack.append((l, h))
    assert len(nodes) == len(deg)
    pre = [[] for _ in nodes]
    for i, (lo, hi) in enumerate(nodes):
        for c, l, h in children(lo, hi, (0, 1, 2, 3)):
            pre[ident[(l, h)]].append(i)
    g = Dawg()
    g.n_node, g.sym, g.pre, g.sa = len(nodes), sym, pre, sa
    g.qoff0 = [sa[lo] for lo, hi in nodes]
    g.n_qoff = [hi - lo for lo, hi in nodes]
    return g


class LCell(sw.Cell):
    __slots__ = ("qlen",)


def new_cell(lo, hi, lo_rc, qlen, **kw):
    c = LCell(lo, hi, lo_rc, **kw)
    c.qlen = qlen
    return c


def copy_cell(p):
    c = LCell.__new__(LCell)
    for s in sw.Cell.__slots__:
        setattr(c, s, getattr(p, s))
    c.qlen = p.qlen
    return c


def merge(tab, cand):
    """sw_model.merge with the query length: a merge into a present key keeps the larger"""
    slot, absent = tab.put(cand)
    if absent:
        return cand, 7
    q = tab.slots[slot]
    q.qlen = max(q.qlen, cand.qlen)
    ch = 0
    if q.E < cand.E:
        q.E, q.E_from, q.E_pos, ch = cand.E, cand.E_from, cand.E_pos, ch | 2
    if q.F < cand.F:
        q.F, q.F_from, ch = cand.F, cand.F_from, ch | 4
    if q.H < cand.H:
        q.H, q.H_from, ch = cand.H, cand.H_from, ch | 1
        if cand.H_from == sw.FROM_H:
            q.H_pos = cand.H_pos
    return q, ch


def top_cells(tab, n):
    keys = sorted(((tab.slots[i].H << 32 | i) for i in tab.occupied()), reverse=True)[:n]
    return [copy_cell(tab.slots[x & sw.M32]) for x in keys]


def fill(ix, g, opt):
    """(rows, best score, best position, nodes where max_min_sc was above 0): rows[i] the kept cells of node i"""
    o = dict(DEFAULTS)
    o.update(opt or {})
    N, ma, mi, go, ge, end_len = o["n_best"], o["match"], o["mis"], o["gap_open"], o["gap_ext"], o["end_len"]
    rows = [[new_cell(0, ix.acc[6], 0, 0)]] + [[] for _ in range(g.n_node - 1)]
    tab = sw.SlotTable(N * 4)
    best, best_pos, n_cut = 0, 0, 0
    for i in range(1, g.n_node):
        cq, pre = g.sym[i], g.pre[i]
        tab.clear()
        max_min_sc = 0
        if len(pre) > 1:
            hs = [c.H for pid in pre for c in rows[pid]]
            if len(hs) > N:
                max_min_sc = sorted(hs, reverse=True)[N]
            max_min_sc = max(max_min_sc - max(go + ge, mi), 0)
        if max_min_sc > 0:
            n_cut += 1
        p = None
        for pid in pre:
            for col, p in enumerate(rows[pid]):
                if p.H + ma < max_min_sc:
                    continue
                pos = pid * N + col
                last_rc = 0
                ext = ix.extend(p.lo, p.hi, p.lo_rc)
                for c in range(1, 6):
                    sc = ma if (c == cq and c != 5) else -mi
                    l, h, rc = ext[c]
                    if h == l or p.H + sc <= 0 or p.H + sc < max_min_sc or (c != cq and p.qlen < end_len):
                        continue
                    last_rc = rc
                    merge(tab, new_cell(l, h, rc, p.qlen + 1, H=p.H + sc, H_pos=pos))
                if p.H - go > p.E:
                    ef, e = sw.OPEN, p.H - go
                else:
                    ef, e = sw.EXT, p.E
                e -= ge
                if e > 0 and e >= max_min_sc and p.qlen >= end_len:
                    merge(tab, new_cell(p.lo, p.hi, last_rc, p.qlen + 1, H=e, E=e, H_from=sw.FROM_E, E_from=ef, E_pos=pos))
        if tab.count == 0:
            continue
        row = top_cells(tab, N)
        fpar = []
        if p.qlen >= end_len:
            heap = [c.H for c in row]
            heapq.heapify(heap)
            stack = [copy_cell(c) for c in reversed(row) if c.H > go + ge]
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
                    q, ch = merge(tab, new_cell(l, h, rc, z.qlen, H=f, F=f, H_from=sw.FROM_F, F_from=ff))
                    if ch & 4:
                        if len(heap) < N:
                            heapq.heappush(heap, f)
                        elif f > heap[0]:
                            heapq.heapreplace(heap, f)
                        fpar.append((z.lo, z.hi))
                        q.F_from, q.F_par = ff, len(fpar) - 1
                        if f - ge > low:
                            stack.append(copy_cell(q))
        row = top_cells(tab, N)
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
        if row[0].H > best:
            best, best_pos = row[0].H, i * N
    return rows, best, best_pos, n_cut


def steps_of(ix, rows, g, N, pos):
    """[(op, reference base)] of the walk from cell `pos` (node * N + column) back to the root"""
    out, last = [], 0
    while pos > 0:
        r = pos // N
        p = rows[r][pos % N]
        state = p.H_from if last == 0 else last
        ext = (p.E_from if state == sw.FROM_E else p.F_from) if state in (sw.FROM_E, sw.FROM_F) else 0
        base = ix.base_of(p.lo)
        if state == sw.FROM_H:
            out.append((swaln.OP_EQ if base == g.sym[r] else swaln.OP_X, base))
            pos = p.H_pos
        elif state == sw.FROM_E:
            out.append((swaln.OP_I, base))
            pos = p.E_pos
        else:
            if p.F == 0 or not p.F_set:
                raise sw.Unrepresentable()
            out.append((swaln.OP_D, base))
            pos = r * N + p.F_par
        last = state if ext else 0
    return out


def align(ix, seq, opt=None, g=None):
    """the hit of one query (symbols 1..5) or None: dict(lo, hi, score, steps, qoff0, n_qoff, n_cut, n_node)"""
    o = dict(DEFAULTS)
    o.update(opt or {})
    if g is None:
        g = dawg(seq)
    rows, best, best_pos, n_cut = fill(ix, g, o)
    align.last = dict(n_cut=n_cut, n_node=g.n_node, n_pre=sum(len(p) for p in g.pre))
    if best < o["min_sc"]:
        return None
    N = o["n_best"]
    node = best_pos // N
    c = rows[node][0]
    return dict(lo=c.lo, hi=c.hi, score=c.H, steps=steps_of(ix, rows, g, N, best_pos), qoff0=g.qoff0[node], n_qoff=g.n_qoff[node])


def n_positions(hit, max_pos):
    return min(max_pos if max_pos > 0 else 1, hit["hi"] - hit["lo"])


def paf_line(name, qid, seq, hit, pos=None, names=None, lengths=None, with_rs=False):
    """swaln_model.paf_line with the query's start, the cs string written from there, and the hit's count on the query"""
    steps = hit["steps"]
    qlen, rlen = swaln.lens_of(steps)
    runs, mlen, blen = swaln.cigar_of(steps)
    f = [swaln._name(name, qid), str(len(seq)), str(hit["qoff0"]), str(hit["qoff0"] + qlen)]

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
    f += [str(mlen), str(blen), "0", "AS:i:%d" % hit["score"], "qh:i:%d" % hit["n_qoff"], "rh:i:%d" % (hit["hi"] - hit["lo"]),
          "cg:Z:" + "".join("%d%s" % (n, swaln.OPS[op]) for n, op in runs), "cs:Z:" + swaln.cs_of(steps, list(seq)[hit["qoff0"]:])]
    if with_rs:
        f.append("rs:Z:" + swaln.rs_of(steps))
    if pos and len(pos) > 1:
        if names is not None:
            f.append("ap:Z:" + "".join("%s,%s,%d;" % (names[p[0] >> 1], "+-"[p[0] & 1], stranded(p)[1]) for p in pos[1:]))
        else:
            f.append("aq:Z:" + "".join("%d,%d;" % p for p in pos[1:]))
    return ("\t".join(f) + "\n").encode()


unmapped_line = swaln.unmapped_line
