"""Inputs that make the candidate table of the dynamic program (hd_merge / hd_grow of rb3gpu_hapdiv.h; SlotTable of tests/sw_model.py) grow, and
the models run on them with a table that keeps count.  numpy and the models only: tests/test_cpu_dptable.py checks that every case does what
it is named for, tests/test_gpu_dptable.py holds the kernels against the same answers, tools/make_golden_dptable.py writes the fixtures.

Real indexes are sparse at depth: a row rarely gets the 3N distinct intervals that make a table of 4N slots grow.  Here the index is dense
and the scores are mild -- a random genome of 30 000 symbols with its reverse complement holds every string of up to about 6 symbols, and at
match 2, mismatch 1, gap open 2, gap extension 1 the first rows keep N cells that all extend by all four symbols -- so every window grows
its table in an early row, whatever N is.

  WINDOWS   7 pieces of the genome of 25..31 symbols, one with 5 % mutations (`hapdiv -a25 -w4` cuts 10 windows from them; `sw -e` takes them whole)
  TWICE     4 pieces of 25 symbols found with the counting table: at match 3 they grow a table made for N = 2 twice, both times in the F phase
  FPHASE    4 more: at match 5, gap open 1 they grow a table made for N = 64 from 256 to 512 slots in the F phase, so it leaves LDS there
  REPEATS   6 queries for `sw --local -k1`, each a piece of the genome whose second half is its first half again, so that nodes of the query's
            graph have several predecessors
  REPEAT2   one more of them, which grows a table made for N = 25 twice, the second time in the F phase
  TIES      6 queries of 25 symbols that tell the table's growth from a plain re-insertion (ReinsertTable below).  The two place the same cells,
            but where cells collide in other slots, and a row keeps the N cells of the largest (H, slot): searched were tails of 9 symbols
            after which a row of the true table keeps a cell that the other drops (one in about 150 tails at N = 8, 16, 25 and 48); in front
            of the tail stands the piece of the genome that continues that cell's string, so the best alignment runs through the cell"""
import numpy as np

from tests import util
from tests import sw_model as sw
from tests import swaln_model as swaln
from tests import swlocal_model as swlocal

GENOME_SEED, GENOME_LEN = 7, 30000
SCORES = dict(match=2, mis=1, gap_open=2, gap_ext=1, min_sc=10)
SCORES_TWICE = dict(SCORES, match=3)
SCORES_F = dict(SCORES, match=5, gap_open=1)
K, W = 25, 4                                             # hapdiv -a25 -w4
N_GROW = (1, 2, 4, 8, 16, 25, 32, 48, 64)                # 25 and 32 grow 128 -> 256 slots, 48 and 64 grow 256 -> 512 and leave LDS
N_STAY = (33, 65)                                        # one power of two more to start with: the control
N_LIST = tuple(sorted(N_GROW + N_STAY))
N_RECORDED = (1, 4, 25, 32, 33, 48, 64, 65)              # what tests/golden/DPTABLE_MANIFEST.json holds of the reference
LDS_SLOTS = 256                                          # HD_LDS_SLOTS
TAB_CAP_MIN = 2048                                       # hd_ws_size: the block's global table has at least that many slots, 8 times the first capacity
WINDOW_AT = ((11561, 25), (2793, 26), (20467, 27), (27418, 28), (24633, 29), (1270, 30), (19206, 31))
MUTATED, MUTATE_SEED = 3, 11
TWICE_AT = (23676, 6405, 14407, 16070)
FPHASE_AT = (20357, 26080, 6813, 26838)
REPEAT_AT = ((2566, 30), (7098, 26), (24017, 26), (17446, 31), (14357, 29), (4788, 26))
REPEAT2_AT = ((12907, 27),)
TIES = ("2131431411214342241424323", "3422242332212232121312443", "1433343211121341211312244", "2324221211143132243144422", "4413412443141411414434422",
        "2332232421432241431333334")                     # differ at n_best 8, 16 (in all three kernels), 16, 25, 25 and 48
TIES_N = (8, 16, 25, 48)

_CACHE = {}


def genome():
    if "genome" not in _CACHE:
        _CACHE["genome"] = util.random_genome(np.random.default_rng(GENOME_SEED), GENOME_LEN)
    return _CACHE["genome"]


def index_text():
    """both strands of the genome, each ended by a sentinel: what `build -d` indexes of the FASTA file"""
    return util.make_text([genome()])


def windows():
    g = genome()
    out = [g[s:s + n].copy() for s, n in WINDOW_AT]
    out[MUTATED] = util.mutate(np.random.default_rng(MUTATE_SEED), out[MUTATED], 0.05)
    return out


def twice():
    g = genome()
    return [g[s:s + K].copy() for s in TWICE_AT]


def fphase():
    g = genome()
    return [g[s:s + K].copy() for s in FPHASE_AT]


def repeats(at=REPEAT_AT):
    g = genome()
    return [np.concatenate([g[s:s + n // 2], g[s:s + n - n // 2]]) for s, n in at]


def repeat2():
    return repeats(REPEAT2_AT)


def ties():
    return [np.array([int(c) for c in t], dtype=np.uint8) for t in TIES]


class Case:
    """kernel: hapdiv, sw_e or sw_local; queries: a function; opt: the scores (and end_len); n_list: the n_best to run; file / args: the query
    fixture and the options of the command line that say the same; expect[N]: what the table of EVERY window or query of the case does at
    n_best N -- (growths, at least one of them in the F phase, slots at the start, slots at the end), None where it is not asked"""

    def __init__(self, name, kernel, queries, opt, n_list, file, args, expect):
        self.name, self.kernel, self.queries, self.opt, self.n_list, self.file, self.args, self.expect = name, kernel, queries, opt, n_list, file, args, expect

    def names(self):
        return query_names(self.file)


def _cap0(N):
    c = 4
    while c < 4 * N:
        c *= 2
    return c


def _score_args(o):
    return ["-A%d" % o["match"], "-B%d" % o["mis"], "-O%d" % o["gap_open"], "-E%d" % o["gap_ext"], "-m%d" % o["min_sc"]]


def _recipe_expect():
    e = {N: (1, False, _cap0(N), 2 * _cap0(N)) for N in N_GROW}
    e.update({N: (0, False, _cap0(N), _cap0(N)) for N in N_STAY})
    return e


HAPDIV_ARGS = ["-a%d" % K, "-w%d" % W]
CASES = [
    Case("hapdiv", "hapdiv", windows, SCORES, N_LIST, "dptable_windows.fa.gz", HAPDIV_ARGS + _score_args(SCORES), _recipe_expect()),
    Case("hapdiv-twice", "hapdiv", twice, SCORES_TWICE, (2,), "dptable_twice.fa.gz", HAPDIV_ARGS + _score_args(SCORES_TWICE), {2: (2, True, 8, 32)}),
    Case("hapdiv-f", "hapdiv", fphase, SCORES_F, (64,), "dptable_fphase.fa.gz", HAPDIV_ARGS + _score_args(SCORES_F), {64: (1, True, 256, 512)}),
    Case("sw_e", "sw_e", windows, dict(SCORES, end_len=1), N_LIST, "dptable_windows.fa.gz", ["-e"] + _score_args(SCORES), _recipe_expect()),
    Case("sw_e-twice", "sw_e", twice, dict(SCORES_TWICE, end_len=1), (2,), "dptable_twice.fa.gz", ["-e"] + _score_args(SCORES_TWICE), {2: (2, True, 8, 32)}),
    Case("sw_e-f", "sw_e", fphase, dict(SCORES_F, end_len=1), (64,), "dptable_fphase.fa.gz", ["-e"] + _score_args(SCORES_F), {64: (1, True, 256, 512)}),
    Case("hapdiv-ties", "hapdiv", ties, SCORES, TIES_N, "dptable_ties.fa.gz", HAPDIV_ARGS + _score_args(SCORES), {N: _recipe_expect()[N] for N in TIES_N}),
    Case("sw_e-ties", "sw_e", ties, dict(SCORES, end_len=1), TIES_N, "dptable_ties.fa.gz", ["-e"] + _score_args(SCORES), {N: _recipe_expect()[N] for N in TIES_N}),
    Case("sw_local-ties", "sw_local", ties, dict(SCORES, end_len=1), (16,), "dptable_ties.fa.gz", ["-k1"] + _score_args(SCORES), {16: (None, None, 64, None)}),
    # the graph of a query with a repeat gives a node the candidates of several rows: the small tables grow up to three times; only where they end is asked there
    Case("sw_local", "sw_local", repeats, dict(SCORES, end_len=1), N_LIST, "dptable_repeats.fa.gz", ["-k1"] + _score_args(SCORES),
         {N: _recipe_expect()[N] if N >= 32 else (None, None, _cap0(N), None) for N in N_LIST}),
    Case("sw_local-twice", "sw_local", repeat2, dict(SCORES, end_len=1), (25,), "dptable_repeat2.fa.gz", ["-k1"] + _score_args(SCORES), {25: (2, True, 128, 512)}),
]
BY_NAME = {c.name: c for c in CASES}
FILES = {"dptable_windows.fa.gz": windows, "dptable_twice.fa.gz": twice, "dptable_fphase.fa.gz": fphase, "dptable_repeats.fa.gz": repeats, "dptable_repeat2.fa.gz": repeat2,
         "dptable_ties.fa.gz": ties}
SENSITIVE = [("hapdiv-ties", N) for N in TIES_N] + [("sw_e-ties", N) for N in TIES_N] + [("sw_local-ties", 16)]   # where ReinsertTable gives another answer
GENOME_FILE, GENOME_NAME = "dptable_genome.fa.gz", "dptable"


def query_names(file):
    return ["%s%d" % (file[len("dptable_"):].split(".")[0], i) for i in range(len(FILES[file]()))]


class CountingTable(sw.SlotTable):
    """SlotTable that keeps what its growths were -- (slots before, slots after, whether the put that caused it came from the F phase) -- and the most
    puts of the F phase between two clears: at least as many as F parents were recorded, and with n_best more, as cells were on the stack"""
    made = []

    def __init__(self, want):
        super().__init__(want)
        self.start, self.growths, self.f_puts, self.max_f_puts, self._in_f = 1 << self.bits, [], 0, 0, False
        CountingTable.made.append(self)

    def clear(self):
        super().clear()
        self.f_puts = 0

    def put(self, cell):
        self._in_f = cell.H_from == sw.FROM_F
        if self._in_f:
            self.f_puts += 1
            self.max_f_puts = max(self.max_f_puts, self.f_puts)
        return super().put(cell)

    def _grow(self):
        self.growths.append((1 << self.bits, 2 << self.bits, self._in_f))
        super()._grow()

    def end(self):
        return 1 << self.bits


class ReinsertTable(CountingTable):
    """the deliberately WRONG growth: the old entries put into an empty table of twice the slots in slot order, without the in-place hand-over of
    displaced entries.  The same set of cells in other slots, so other winners among equal scores"""

    def _grow(self):
        self.growths.append((1 << self.bits, 2 << self.bits, self._in_f))
        old = [c for c in self.slots if c is not None]
        self.bits += 1
        self.slots = [None] * (1 << self.bits)
        mask = (1 << self.bits) - 1
        for c in old:
            i = sw.home_slot(sw.key_hash(c.lo, c.hi), self.bits)
            while self.slots[i] is not None:
                i = (i + 1) & mask
            self.slots[i] = c
        self.grown += 1


def model_index():
    """the plain BWT of index_text() and its BwtIndex (the host's suffix sorter; no device)"""
    if "index" not in _CACHE:
        from ropebwt3_amd import host
        bwt = host.build_bwt(index_text())
        _CACHE["index"] = (bwt, sw.BwtIndex(bwt))
    return _CACHE["index"]


def run_model(case, N, table=CountingTable):
    """(answers, tables) of the case at n_best N, computed once: hapdiv -- [(query, offset, nine numbers)]; sw_e -- the list of hits per query;
    sw_local -- (the hit or None, nodes) per query.  tables: the table of every window or query, in order.  Unrepresentable is not caught"""
    key = (case.name, N, table.__name__)
    if key not in _CACHE:
        ix = model_index()[1]
        qs = case.queries()
        o = dict(case.opt, n_best=N)
        keep, sw.SlotTable, CountingTable.made = sw.SlotTable, table, []
        try:
            if case.kernel == "hapdiv":
                ans = sw.hapdiv(ix, qs, K, W, o)
            elif case.kernel == "sw_e":
                ans = [swaln.align(ix, q, o) for q in qs]
            else:
                ans = []
                for q in qs:
                    hit = swlocal.align(ix, q, o)
                    ans.append((hit, swlocal.align.last["n_node"]))
            _CACHE[key] = (ans, CountingTable.made)
        finally:
            sw.SlotTable, CountingTable.made = keep, []
    return _CACHE[key]


def n_tier2(tables, lds_slots=LDS_SLOTS):
    """how many tables end in global memory: those that start above lds_slots or grow past it"""
    return sum(1 for t in tables if t.end() > lds_slots)
