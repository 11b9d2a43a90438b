"""Host model of the slot partition of the block array (rb3gpu_layout.h), numpy only, and plain sequences that hit one slot shape each.

The rule (k_decide, and its copies in k_reb_group and k_plane_group): the BWT of n symbols has (n >> 8) + 1 windows of 256 symbols and
(n >> 13) + 1 groups of 32 windows; the last group holds what is left of the windows (the window of position n included, so a total
that is a multiple of 256 ends in an empty window).  Inside a group, a block of 2^L aligned windows (L = 1..5) that lies wholly inside
the group's windows may be one run slot if at most 48 maximal equal-symbol runs intersect it; a window takes level L only if it took
every level below it; a single window is a bit-plane slot; a slot starts at every window w with w & ((1 << level) - 1) == 0."""
import numpy as np

WIN_BITS, GRP_BITS = 8, 13
WIN, GRP, GRP_WINS = 1 << WIN_BITS, 1 << GRP_BITS, 32
RLE_CODES = 48
GRP_ALLOC = 64 + 8      # RB3_GRP_ALLOC: a directory entry + its word of the compact copy
SLOT_BYTES = 128


def n_windows(n):
    return (n >> WIN_BITS) + 1


def n_groups(n):
    return (n >> GRP_BITS) + 1


def slot_masks(plain):
    """per group, the uint32 mask of the windows that start a slot (rb3_grp_t.mask)"""
    b = np.asarray(plain, dtype=np.uint8)
    n = b.size
    W, G = n_windows(n), n_groups(n)
    head = np.ones(n, dtype=bool)
    head[1:] = b[1:] != b[:-1]
    hw = np.bincount(np.flatnonzero(head) >> WIN_BITS, minlength=G * GRP_WINS).astype(np.int64)
    H = np.concatenate([[0], np.cumsum(hw)])                     # heads in the windows before window w
    wst = np.arange(G * GRP_WINS, dtype=np.int64) << WIN_BITS
    cont = np.zeros(G * GRP_WINS, dtype=np.int64)               # the window's first symbol continues the run before it
    inside = wst < n
    cont[inside] = ~head[wst[inside]]
    lane = np.arange(GRP_WINS)
    g0 = np.arange(G, dtype=np.int64)[:, None] * GRP_WINS
    nvw = np.minimum(W - g0, GRP_WINS)                          # (G, 1) windows of every group
    level = np.zeros((G, GRP_WINS), dtype=np.int64)
    for L in range(1, 6):
        a = g0 + (lane & ~((1 << L) - 1))[None, :]              # first window of the lane's block (global)
        e = a + (1 << L)
        ok = (e - g0 <= nvw) & (H[np.minimum(e, G * GRP_WINS)] - H[a] + cont[a] <= RLE_CODES)
        level = np.where(ok & (level == L - 1), L, level)
    start = (lane[None, :] < nvw) & ((lane[None, :] & ((1 << level) - 1)) == 0)
    return (start.astype(np.uint64) << lane[None, :].astype(np.uint64)).sum(axis=1).astype(np.uint32)


def slot_count(plain):
    """the number of slots of the block array of a plain BWT"""
    m = slot_masks(plain)
    return int(sum(bin(int(x)).count("1") for x in m))


def expected_bytes_index(plain):
    """stats()["bytes_index"] as index_install writes it"""
    n = np.asarray(plain).size
    return n_groups(n) * GRP_ALLOC + slot_count(plain) * SLOT_BYTES


def cum(plain):
    """the (n + 1, 6) int64 table of cumulative symbol counts: cum[k, a] = #{i < k : B[i] = a}"""
    b = np.asarray(plain, dtype=np.uint8)
    out = np.zeros((b.size + 1, 6), dtype=np.int64)
    for c in range(6):
        np.cumsum(b == c, out=out[1:, c])
    return out


# ---- deterministic edge cases: (name, plain) ----

def _runs_block(rng, length, nruns, first_not=None, syms=(1, 2, 3, 4)):
    """`length` symbols in exactly `nruns` maximal runs (adjacent runs differ; the first symbol differs from `first_not`)"""
    cuts = np.sort(rng.choice(np.arange(1, length), size=nruns - 1, replace=False)) if nruns > 1 else np.zeros(0, dtype=np.int64)
    lens = np.diff(np.concatenate([[0], cuts, [length]]))
    out, prev = [], first_not
    for l in lens:
        s = int(rng.choice([x for x in syms if x != prev]))
        out.append(np.full(int(l), s, dtype=np.uint8))
        prev = s
    return np.concatenate(out)


def _blocks(rng, nblocks, sz_win, nruns, syms=(1, 2, 3, 4)):
    """nblocks blocks of sz_win windows, each of exactly nruns runs, no run shared between blocks"""
    parts, last = [], None
    for _ in range(nblocks):
        p = _runs_block(rng, sz_win * WIN, nruns, last, syms)
        parts.append(p)
        last = int(p[-1])
    return np.concatenate(parts)


def _tail(rng, plain, n):
    """plain cut or padded (with random symbols) to n symbols"""
    if plain.size >= n:
        return plain[:n].copy()
    return np.concatenate([plain, rng.integers(0, 6, size=n - plain.size, dtype=np.uint8)])


def edge_cases():
    """each case names the slot shape it is built for; test_cpu_layout_model.py checks that the shape is there"""
    rng = np.random.default_rng(20261016)
    cases = []
    for L in range(1, 6):   # run slots of exactly 2^L windows: 40 runs per aligned block of 2^L windows, 80 in a block of twice that
        sz = 1 << L
        cases.append(("runslot_%dw" % sz, _blocks(rng, 6 * GRP_WINS // sz, sz, 40)))
    cases.append(("runs48_2w_slot", _blocks(rng, 3 * GRP_WINS // 2, 2, 48)))
    cases.append(("runs49_2w_planes", _blocks(rng, 3 * GRP_WINS // 2, 2, 49)))
    # runs that end exactly on window and group borders, then runs that cross several groups
    lens = [WIN] * 40 + [24 * WIN, GRP, GRP - WIN, WIN, 3 * GRP, 5 * GRP + 17, WIN - 17, 40000, 1, 8191, GRP + 1]
    parts, prev = [], 0
    for i, l in enumerate(lens):
        s = 1 + (prev % 4)
        parts.append(np.full(l, s, dtype=np.uint8))
        prev = s
    cases.append(("runs_on_window_and_group_borders", np.concatenate(parts)))
    # long runs of symbol 0 and of symbol 5 (the codes' symbol field at both ends)
    for s in (0, 5):
        p = []
        for i in range(12):
            p.append(np.full(int(rng.integers(300, 12000)), s, dtype=np.uint8))
            p.append(_runs_block(rng, int(rng.integers(50, 700)), int(rng.integers(2, 30)), s, syms=tuple(x for x in range(6) if x != s)))
        cases.append(("long_runs_of_symbol_%d" % s, np.concatenate(p)))
    cases.append(("dense_random_every_slot_a_plane", rng.integers(0, 6, size=5 * GRP + 1000, dtype=np.uint8)))
    # in every group: 16 random windows (planes), then 16 windows of long runs (run slots of 16, 8, ... windows)
    p = []
    for g in range(5):
        p.append(rng.integers(0, 6, size=16 * WIN, dtype=np.uint8))
        p.append(_runs_block(rng, 16 * WIN, 30 - 4 * g, None))
    cases.append(("planes_and_run_slots_in_one_group", np.concatenate(p)))
    base = np.concatenate([_blocks(rng, 4, 8, 30), rng.integers(0, 6, size=GRP, dtype=np.uint8), _blocks(rng, 16, 2, 45)])
    for g, r in ((3, 0), (3, 1), (4, 255), (4, 256), (5, 257), (0, 1), (0, 255), (0, 256), (0, 257)):
        cases.append(("total_8192x%d_plus_%d" % (g, r), _tail(rng, base, GRP * g + r)))
    return cases
