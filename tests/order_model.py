"""Python model of the sorted string orders of `build -s` (RLO) and `build -r` (RCLO).

The BWT the reference builds in such an order is the input-order BWT of the same collection with the strings
reordered so that their reversed contents ascend: $ < A < C < G < T < N for RLO, $ < T < G < C < A < N for RCLO
(a string that is a suffix of another first).  p0 is where the sentinels of a merged batch go: the number of index
strings that sort before each batch string (a new string before identical old ones)."""
import numpy as np

SO_IO, SO_RLO, SO_RCLO = 0, 1, 2
_RCLO_MAP = np.array([0, 4, 3, 2, 1, 5], dtype=np.uint8)   # T G C A -> A C G T, N last


def strings_of(text):
    """the strings of a batch text (every one terminated by 0), without their sentinels"""
    text = np.asarray(text, dtype=np.uint8)
    ends = np.flatnonzero(text == 0)
    starts = np.concatenate([[0], ends[:-1] + 1])
    return [text[b:e] for b, e in zip(starts, ends)]


def key(s, so):
    r = np.asarray(s, dtype=np.uint8)[::-1]
    if so == SO_RCLO:
        r = _RCLO_MAP[r]
    return r.tobytes()   # bytes compare like the order: a prefix sorts first


def ordered(strings, so):
    return sorted(strings, key=lambda s: key(s, so))


def text_of(strings):
    z = np.zeros(1, dtype=np.uint8)
    parts = []
    for s in strings:
        parts += [np.asarray(s, dtype=np.uint8), z]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def ordered_text(text, so):
    return text_of(ordered(strings_of(text), so))


def p0(index_strings, batch_strings, so):
    """the insertion point of the sentinel of every batch string among the index's strings"""
    import bisect
    ks = sorted(key(s, so) for s in index_strings)
    return np.array([bisect.bisect_left(ks, key(s, so)) for s in batch_strings], dtype=np.int64)


def random_collection(rng, n_strings, max_len=40, dup=0.2, suffix=0.1, n_rate=0.02):
    """short strings with duplicates, suffix relations, N and 1-symbol strings"""
    out = []
    for _ in range(n_strings):
        u = rng.random()
        if out and u < dup:
            out.append(out[rng.integers(len(out))].copy())
        elif out and u < dup + suffix:
            s = out[rng.integers(len(out))]
            out.append(s[rng.integers(len(s)):].copy())
        else:
            n = int(rng.integers(1, max_len + 1))
            s = rng.integers(1, 5, size=n, dtype=np.uint8)
            s[rng.random(n) < n_rate] = 5
            out.append(s)
    return out


def to_lines(strings):
    return "".join("".join("$ACGTN"[c] for c in s) + "\n" for s in strings)
