"""Python model of `hapdiv`: the end-to-end BWA-SW dynamic program of a window against an FM-index, restated from its behaviour.

The window of k symbols is consumed from its END: row i (1..k) aligns the last i symbols, and a cell of a row is a bidirectional
interval (lo, hi, lo_rc) of the index with the best scores H (any end), E (ends in a gap of the index side) and F (ends in a gap of
the window side).  What makes the answer more than "the best N cells of every row" is ORDER: candidates of a row meet in an
open-addressing table keyed by (lo, hi), the first of two equal candidates wins, and a row keeps the N cells of the largest
(H, slot in the table).  So the table is modelled slot by slot (SlotTable): its hash, its linear probing, its growth at 3/4 load with
the in-place re-placement that moves displaced entries on, and its capacity, which is kept from row to row within a window.

Ranks come from the plain BWT (BwtIndex): acc[c] + the number of c before a row.  A backward extension by c of (lo, size, lo_rc) is
(acc[c] + rank(c, lo), rank(c, lo + size) - rank(c, lo), lo_rc + the sizes of the symbols laid out before c's complement on the other
strand: $ T G C A N)."""
import heapq

import numpy as np

FROM_H, FROM_E, FROM_F = 0, 1, 2
OPEN, EXT = 0, 1
NONE = 0xFFFFFFFF          # no cell
UNSET = 0x3FFFFFF          # no F parent
MAX_ED = 6
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1

DEFAULTS = dict(n_best=25, min_sc=30, match=1, mis=3, gap_open=5, gap_ext=2, e2e_drop=-1)


class Unrepresentable(Exception):
    """the backtrack walked into an F step that has no column (the reference stops on an assertion there)"""


def mix32(x):
    x &= M64
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    x ^= x >> 31
    return x & M32


def key_hash(lo, hi):
    return (mix32(lo) + mix32(hi)) & M32


def home_slot(h, bits):
    return (h * 2654435769 & M32) >> (32 - bits)


class Cell:
    __slots__ = ("H", "E", "F", "H_from", "E_from", "F_from", "F_par", "F_set", "H_pos", "E_pos", "lo", "hi", "lo_rc", "flt")

    def __init__(self, lo, hi, lo_rc, H=0, E=0, F=0, H_from=FROM_H, E_from=OPEN, F_from=OPEN, H_pos=NONE, E_pos=NONE):
        self.lo, self.hi, self.lo_rc, self.H, self.E, self.F = lo, hi, lo_rc, H, E, F
        self.H_from, self.E_from, self.F_from, self.H_pos, self.E_pos = H_from, E_from, F_from, H_pos, E_pos
        self.F_par, self.F_set, self.flt = UNSET, 0, 0

    def copy(self):
        c = Cell.__new__(Cell)
        for s in Cell.__slots__:
            setattr(c, s, getattr(self, s))
        return c


class SlotTable:
    """cells by (lo, hi) in 2^bits slots: linear probing from home_slot, doubling at 3/4 load BEFORE the probe of a put"""

    def __init__(self, want):
        self.bits = 2
        while (1 << self.bits) < want:
            self.bits += 1
        self.slots = [None] * (1 << self.bits)
        self.count = 0
        self.grown = 0

    def clear(self):
        self.slots = [None] * (1 << self.bits)
        self.count = 0

    def occupied(self):
        return [i for i, c in enumerate(self.slots) if c is not None]

    def _grow(self):
        old_n, bits = 1 << self.bits, self.bits + 1
        mask = (1 << bits) - 1
        slots = self.slots + [None] * old_n
        old_used = [c is not None for c in self.slots]
        new_used = [False] * (2 * old_n)
        for j in range(old_n):                    # every old entry in slot order; an entry whose new slot still holds an
            if not old_used[j]:                   # old one takes the slot and sends that one on
                continue
            cur, old_used[j] = slots[j], False
            while True:
                i = home_slot(key_hash(cur.lo, cur.hi), bits)
                while new_used[i]:
                    i = (i + 1) & mask
                new_used[i] = True
                if i < old_n and old_used[i]:
                    slots[i], cur = cur, slots[i]
                    old_used[i] = False
                else:
                    slots[i] = cur
                    break
        self.slots = [c if u else None for c, u in zip(slots, new_used)]
        self.bits = bits
        self.grown += 1

    def find(self, lo, hi):
        mask = (1 << self.bits) - 1
        i = first = home_slot(key_hash(lo, hi), self.bits)
        while self.slots[i] is not None and not (self.slots[i].lo == lo and self.slots[i].hi == hi):
            i = (i + 1) & mask
            if i == first:
                return None
        return i if self.slots[i] is not None else None

    def put(self, cell):
        """(slot, absent): the cell is stored only if its key was absent"""
        n = 1 << self.bits
        if self.count >= (n >> 1) + (n >> 2):
            self._grow()
            n = 1 << self.bits
        mask = n - 1
        i = home_slot(key_hash(cell.lo, cell.hi), self.bits)
        while self.slots[i] is not None and not (self.slots[i].lo == cell.lo and self.slots[i].hi == cell.hi):
            i = (i + 1) & mask
        if self.slots[i] is None:
            self.slots[i] = cell
            self.count += 1
            return i, True
        return i, False


def merge(tab, cand):
    """the candidate into the table: (the stored cell, which of H=1 E=2 F=4 changed).  Strict comparisons: the first arrival keeps a tie"""
    slot, absent = tab.put(cand)
    if absent:
        return cand, 7
    q, ch = tab.slots[slot], 0
    if q.E < cand.E:
        q.E, q.E_from, q.E_pos, ch = cand.E, cand.E_from, cand.E_pos, ch | 2
    if q.F < cand.F:
        q.F, q.F_from, ch = cand.F, cand.F_from, ch | 4
    if q.H < cand.H:
        q.H, q.H_from, ch = cand.H, cand.H_from, ch | 1
        if cand.H_from == FROM_H:
            q.H_pos = cand.H_pos
    return q, ch


def top_cells(tab, n):
    """copies of the n cells of the largest (H, slot), largest first"""
    keys = sorted(((tab.slots[i].H << 32 | i) for i in tab.occupied()), reverse=True)[:n]
    return [tab.slots[x & M32].copy() for x in keys]


class BwtIndex:
    def __init__(self, bwt):
        b = np.asarray(bwt, dtype=np.uint8)
        self.n = int(b.size)
        self.cum = []
        for c in range(6):
            a = np.zeros(b.size + 1, dtype=np.int64)
            np.cumsum(b == c, out=a[1:])
            self.cum.append(a.tolist())
        self.acc = [0]
        for c in range(6):
            self.acc.append(self.acc[-1] + self.cum[c][-1])

    def extend(self, lo, hi, lo_rc):
        """[(lo, hi, lo_rc)] of the backward extension by every symbol 0..5"""
        size = [self.cum[c][hi] - self.cum[c][lo] for c in range(6)]
        out, at = [None] * 6, lo_rc
        for c in (0, 4, 3, 2, 1, 5):
            l = self.acc[c] + self.cum[c][lo]
            out[c] = (l, l + size[c], at)
            at += size[c]
        return out

    def base_of(self, lo):
        c = 1
        while c < 7 and self.acc[c] <= lo:
            c += 1
        return c - 1


def fill(ix, seq, opt):
    """(rows, best score): rows[i] the kept cells of row i, the last row with its contained cells flagged"""
    o = dict(DEFAULTS)
    o.update(opt or {})
    N, ma, mi, go, ge = o["n_best"], o["match"], o["mis"], o["gap_open"], o["gap_ext"]
    k = len(seq)
    rows = [[Cell(0, ix.acc[6], 0)]] + [[] for _ in range(k)]
    tab = SlotTable(N * 4)
    best = 0
    n_ext = 0
    for i in range(1, k + 1):
        cq, prev = int(seq[k - i]), rows[i - 1]
        tab.clear()
        inner = i - 1 >= 1                     # mismatches and gaps only once one symbol is aligned (end_len 1)
        for col, p in enumerate(prev):
            pos = (i - 1) * N + col
            last_rc = 0
            n_ext += 1
            ext = ix.extend(p.lo, p.hi, p.lo_rc)
            for c in range(1, 6):
                sc = ma if (c == cq and c != 5) else -mi
                l, h, rc = ext[c]
                if h == l or p.H + sc <= 0 or (c != cq and not inner):
                    continue
                last_rc = rc
                merge(tab, Cell(l, h, rc, H=p.H + sc, H_pos=pos))
            if p.H - go > p.E:
                ef, e = OPEN, p.H - go
            else:
                ef, e = EXT, p.E
            e -= ge
            if e > 0 and inner:                # the gap cell keeps the parent's interval, but the OTHER strand's start of the last
                merge(tab, Cell(p.lo, p.hi, last_rc, H=e, E=e, H_from=FROM_E, E_from=ef, E_pos=pos))   # candidate made above
        if tab.count == 0:
            continue
        row = top_cells(tab, N)
        fpar = []
        if inner and prev:
            heap = [c.H for c in row]
            heapq.heapify(heap)
            stack = [c.copy() for c in reversed(row) if c.H > go + ge]
            while stack:
                z = stack.pop()
                low = 0 if len(heap) < N else heap[0]
                if z.H - go > z.F:
                    ff, f = OPEN, z.H - go
                else:
                    ff, f = EXT, z.F
                f -= ge
                if f <= low:
                    continue
                n_ext += 1
                ext = ix.extend(z.lo, z.hi, z.lo_rc)
                for c in range(1, 6):
                    l, h, rc = ext[c]
                    if h == l:
                        continue
                    q, ch = merge(tab, Cell(l, h, rc, H=f, F=f, H_from=FROM_F, F_from=ff))
                    if ch & 4:
                        if len(heap) < N:
                            heapq.heappush(heap, f)
                        elif f > heap[0]:
                            heapq.heapreplace(heap, f)
                        fpar.append((z.lo, z.hi))
                        q.F_from, q.F_par = ff, len(fpar) - 1
                        if f - ge > low:
                            stack.append(q.copy())
        row = top_cells(tab, N)
        if fpar:
            where = {(c.lo, c.hi): j for j, c in enumerate(row)}
            for c in row:
                if c.F == 0 or c.F_par == UNSET:
                    continue
                j = where.get(fpar[c.F_par])
                if j is None:
                    c.F_par = UNSET
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
    fill.last_ext = n_ext
    return rows, best


def edit_distance(ix, rows, seq, N, pos):
    """mismatches + gap symbols on the path back from cell `pos` (row * N + column) to the root"""
    k, ed, last = len(seq), 0, 0
    while pos > 0:
        r = pos // N
        p = rows[r][pos % N]
        state = p.H_from if last == 0 else last
        ext = (p.E_from if state == FROM_E else p.F_from) if state in (FROM_E, FROM_F) else 0
        if state == FROM_H:
            ed += 1 if ix.base_of(p.lo) != int(seq[k - r]) else 0
            pos = p.H_pos
        elif state == FROM_E:
            pos, ed = p.E_pos, ed + 1
        else:
            if p.F == 0 or not p.F_set:
                raise Unrepresentable()
            pos, ed = r * N + p.F_par, ed + 1
        last = state if ext else 0
    return ed


def window(ix, seq, opt=None):
    """(n_al, max_ed, n_hap[0..6]) of one window (symbols 1..5)"""
    o = dict(DEFAULTS)
    o.update(opt or {})
    N = o["n_best"]
    rows, best = fill(ix, seq, o)
    out = [0] * 9
    last = rows[len(seq)]
    if best < o["min_sc"] or not last:
        return tuple(out)
    h0 = last[0].H
    for j, c in enumerate(last):
        if c.flt or c.H_from != FROM_H or c.H < o["min_sc"] or (o["e2e_drop"] >= 0 and h0 - c.H > o["e2e_drop"]):
            continue
        ed = edit_distance(ix, rows, seq, N, len(seq) * N + j)
        out[0] += 1
        out[1] = max(out[1], ed)
        out[2 + min(ed, MAX_ED)] += c.hi - c.lo
    return tuple(out)


def hapdiv(ix, queries, k, w, opt=None):
    """[(query, offset, the nine numbers)] of every window of every query (symbol arrays)"""
    out = []
    for qi, q in enumerate(queries):
        off = 0
        while off + k <= len(q):
            out.append((qi, off, window(ix, q[off:off + k], opt)))
            off += w
    return out


def merge_lines(windows, k, names=None, first_id=0):
    """the output bytes: consecutive windows of one query with equal numbers make one line"""
    out, i = [], 0
    while i < len(windows):
        j = i
        while j + 1 < len(windows) and windows[j + 1][0] == windows[i][0] and tuple(windows[j + 1][2]) == tuple(windows[i][2]):
            j += 1
        q = windows[i][0]
        nm = names[q] if names is not None and names[q] is not None else "seq%d" % (first_id + q + 1)
        nm = nm.encode() if isinstance(nm, str) else nm
        out.append(nm + b"\t%d\t%d" % (windows[i][1], windows[j][1] + k) + b"".join(b"\t%d" % int(x) for x in windows[i][2]) + b"\n")
        i = j + 1
    return b"".join(out)
