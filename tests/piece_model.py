"""Python model of `get` in pieces over tests/walk_model.Fm, every stage restated as it is defined:

- splitters: with m = acc[1], n = acc[6], splitter p < m is sentinel row p and splitter p >= m is row m + ((p - m) << S); there are
  m + ceil((n - m) / 2^S) of them;
- a piece is the LF walk from a splitter's row until the step that reads the sentinel or lands on a splitter's row: (next splitter, or the string
  the walk ended in -- the sentinel row LF leads to -- ; steps), and the row the sentinel was read at is the end row of that string;
- pointer jumping, ceil(log2 #splitters) + 1 rounds, makes every piece (string, D): D is the number of LF steps from the piece's row up to and
  including the one that reads the sentinel, so the symbol read at a row of distance d is symbol d - 2 of its string;
- the pieces are sorted by (string << 32 | D - 1); a row asked for walks to the first splitter it meets (none if it is a splitter's row, and it may
  read the sentinel first), has D = its own steps + D of that splitter, and its pieces are the sorted range from the first piece of the string to
  that splitter;
- emit: the row's own walk and every piece of the range are walked again and the symbol read at distance d goes to position d - 2."""
import numpy as np

from tests import walk_model as wm


def _ranges(lo, cnt):
    """the indices lo[i], lo[i] + 1, ... (cnt[i] of them) for every i, end to end, and the i of each"""
    tot = int(cnt.sum())
    who = np.repeat(np.arange(cnt.size), cnt)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    return lo[who] + (np.arange(tot) - start[who]), who


class Pieces:
    def __init__(self, fm, S):
        self.fm, self.S = fm, int(S)
        self.m, self.n = int(fm.acc[1]), fm.n
        m, n = self.m, self.n
        self.nsp = m + (((n - m) + (1 << S) - 1) >> S)
        p = np.arange(self.nsp, dtype=np.int64)
        self.row = np.where(p < m, p, m + ((p - m) << S))
        self.end_row = np.full(m, -1, dtype=np.int64)
        # 1. the pieces, all at the same time; every step is kept as (piece, step, symbol) for the emit
        self.nxt, self.string, self.steps, (self.t_id, self.t_step, self.t_sym) = self._walk(self.row, True)
        o = np.argsort(self.t_id, kind="stable")
        self.t_id, self.t_step, self.t_sym = self.t_id[o], self.t_step[o], self.t_sym[o]
        self.t_off = np.concatenate([[0], np.cumsum(np.bincount(self.t_id, minlength=self.nsp))])
        # 2. the join
        nxt, s, D = self.nxt.copy(), self.string.copy(), self.steps.copy()
        rounds = 1
        while (1 << (rounds - 1)) < self.nsp:
            rounds += 1
        for _ in range(rounds):
            go = np.flatnonzero(nxt >= 0)
            q = nxt[go]
            D[go], s[go], nxt[go] = D[go] + D[q], s[q], nxt[q]
        assert (nxt < 0).all() and (s >= 0).all() and (s < m).all()
        self.D, self.s = D, s
        # 3. the order
        self.key = (s << 32) | (D - 1)
        self.sorted = np.argsort(self.key, kind="stable")
        self.skey = self.key[self.sorted]
        self.pos = np.empty(self.nsp, dtype=np.int64)
        self.pos[self.sorted] = np.arange(self.nsp)

    def is_split(self, k):
        return (k < self.m) | (((k - self.m) & ((1 << self.S) - 1)) == 0)

    def _walk(self, rows, trace):
        """from every row until the sentinel is read or a splitter's row is reached: (next splitter or -1, string or -1, steps[, the steps taken])"""
        fm, m = self.fm, self.m
        nw = rows.size
        nxt, string, steps = np.full(nw, -1, dtype=np.int64), np.full(nw, -1, dtype=np.int64), np.zeros(nw, dtype=np.int64)
        ids, k = np.arange(nw), rows.astype(np.int64)
        tr = ([], [], [])
        while ids.size:
            c = fm.b[k].astype(np.int64)
            k2 = fm.acc[c] + fm.occ[c, k]
            steps[ids] += 1
            if trace:
                tr[0].append(ids), tr[1].append(steps[ids]), tr[2].append(c.astype(np.uint8))
            dollar = c == 0
            string[ids[dollar]] = k2[dollar]
            self.end_row[k2[dollar]] = k[dollar]
            split = ~dollar & self.is_split(k2)
            nxt[ids[split]] = np.where(k2[split] < m, k2[split], m + ((k2[split] - m) >> self.S))
            on = ~dollar & ~split
            ids, k = ids[on], k2[on]
        if trace:
            return nxt, string, steps, tuple(np.concatenate(x) if x else np.zeros(0, dtype=np.int64) for x in tr)
        return nxt, string, steps

    def retrieve(self, rows):
        """(end rows, [string per row], stats) as Rb3Gpu.retrieve(rows, pieces=True) answers"""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        m = self.m
        end = np.full(rows.size, -1, dtype=np.int64)
        seqs = [np.zeros(0, dtype=np.uint8)] * rows.size
        at = np.flatnonzero((rows >= 0) & (rows < self.n))
        k = rows[at]
        sp = self.is_split(k)
        meet, s, l0 = np.full(k.size, -1, dtype=np.int64), np.full(k.size, -1, dtype=np.int64), np.zeros(k.size, dtype=np.int64)
        meet[sp] = np.where(k[sp] < m, k[sp], m + ((k[sp] - m) >> self.S))
        w = np.flatnonzero(~sp)
        meet[w], s[w], l0[w], (h_id, h_step, h_sym) = self._walk(k[w], True)
        hit = meet >= 0
        D = l0.copy()
        D[hit] += self.D[meet[hit]]
        s[hit] = self.s[meet[hit]]
        first = np.searchsorted(self.skey, s << 32)
        cnt = np.where(hit, self.pos[np.maximum(meet, 0)] - first + 1, 0)
        assert (cnt[hit] >= 1).all()
        end[at] = self.end_row[s]
        # emit: one buffer for all the rows, the symbol read at distance d of row v at off[v] + d - 2
        off = np.concatenate([[0], np.cumsum(D - 1)])
        out = np.full(int(off[-1]), 255, dtype=np.uint8)
        hv = w[h_id]                                     # the rows' own walks: step t of row v is read at distance D[v] - t + 1
        put = h_sym != 0
        out[off[hv[put]] + (D[hv[put]] - h_step[put] + 1) - 2] = h_sym[put]
        sidx, v = _ranges(first, cnt)                    # the pieces of every row
        q = self.sorted[sidx]
        assert (self.s[q] == s[v]).all() and (self.D[q] <= D[v]).all()
        tidx, qi = _ranges(self.t_off[q], self.t_off[q + 1] - self.t_off[q])
        d = self.D[q[qi]] - self.t_step[tidx] + 1
        put = self.t_sym[tidx] != 0
        out[off[v[qi[put]]] + d[put] - 2] = self.t_sym[tidx[put]]
        assert (out != 255).all()
        for i, a in enumerate(at):
            seqs[a] = out[off[i]:off[i + 1]].copy()
        stats = {"n_pieces": self.nsp, "max_piece_steps": int(self.steps.max()), "n_symbols": int(off[-1]), "n_rows": int(rows.size),
                 "n_steps": int(self.steps.sum() + l0.sum() + h_step.size + tidx.size)}
        return end, seqs, stats


def get_text(pc, rows):
    """the bytes of `get --pieces <index> rows...`"""
    end, seqs, _ = pc.retrieve(rows)
    return b"".join(b">%d %d\n" % (int(k), int(e)) + wm.LETTERS[s].tobytes() + b"\n" for k, e, s in zip(rows, end, seqs) if e >= 0)
