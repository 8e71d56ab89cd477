"""What the error-correction tests expect, from the reads alone (not a test module): the rule of include/bwtm.h restated as a brute force
over a Counter of windows, the collections it is run on with the reads they were drawn from, and a set of hand-made reads, one for every
branch of the rule.  Nothing here uses the library.  tests/test_correct_host.py checks the brute force itself."""
import functools
from collections import Counter

import numpy as np

import kmer_inputs

CLEAN, CORRECTED, FAILED, SHORT = 0, 1, 2, 3


def table_of(rows, k, skip=5):
    """Counter: the k symbols of a window as bytes -> its occurrences in `rows`; windows that hold `skip` are not k-mers."""
    table = Counter()
    for row in rows:
        b = bytes(bytearray(np.asarray(row, dtype=np.uint8).tolist()))
        for o in range(len(b) - k + 1):
            w = b[o: o + k]
            if skip not in w:
                table[w] += 1
    return table


def solid_count(table, t):
    return sum(1 for v in table.values() if v >= max(int(t), 1))


def correct(row, table, k, t, rounds, skip=5):
    """The rule, step by step as the header numbers it: (bytes, status, edits)."""
    S = bytes(bytearray(np.asarray(row, dtype=np.uint8).tolist()))
    m = len(S)
    t = max(int(t), 1)
    if m < k:
        return S, SHORT, 0
    kept = [c for c in range(1, 6) if c != skip]

    def solid(w):
        return skip not in w and table.get(bytes(w), 0) >= t

    W = bytearray(S)
    r = edits = 0
    while True:
        sol = [solid(W[o: o + k]) for o in range(m - k + 1)]
        uncovered = [i for i in range(m) if not any(sol[max(0, i - k + 1): min(i, m - k) + 1])]
        if not uncovered:
            return bytes(W), (CLEAN if edits == 0 else CORRECTED), edits
        if r == rounds:
            return S, FAILED, 0
        r += 1
        done = False
        for i in uncovered:
            starts = [max(0, i - k + 1)]
            if min(i, m - k) != starts[0]:
                starts.append(min(i, m - k))
            for o in starts:
                cands = []
                for c in kept:
                    if c == W[i]:
                        continue
                    w = bytearray(W[o: o + k]); w[i - o] = c
                    if solid(w):
                        cands.append(c)
                if len(cands) == 1:
                    W[i] = cands[0]; edits += 1; done = True
                    break
            if done:
                break
        if not done:
            return S, FAILED, 0


def correct_all(rows, k, t, rounds, skip=5, table=None):
    """(list of bytes, status uint8, edits uint32) of every row against the table of the rows themselves (or `table`)."""
    table = table_of(rows, k, skip) if table is None else table
    got = [correct(row, table, k, t, rounds, skip) for row in rows]
    return [g[0] for g in got], np.array([g[1] for g in got], dtype=np.uint8), np.array([g[2] for g in got], dtype=np.uint32)


def as_bytes(row):
    return bytes(bytearray(np.asarray(row, dtype=np.uint8).tolist()))


def genome_truth(seed=12):
    """The rows of kmer_inputs.genome_reads() before their errors: the same seed and the same draws, stopping there."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(1, 5, size=kmer_inputs.GENOME).astype(np.uint8)
    starts = rng.integers(0, kmer_inputs.GENOME - kmer_inputs.WIDTH + 1, size=kmer_inputs.READS)
    return genome[starts[:, None] + np.arange(kmer_inputs.WIDTH)[None, :]].copy()


LONG_GENOME = 4000
LONG_READS = 600


@functools.lru_cache(maxsize=None)
def _long_reads(seed):
    rng = np.random.default_rng(seed)
    genome = rng.integers(1, 5, size=LONG_GENOME).astype(np.uint8)
    rows, truth = [], []
    for _ in range(LONG_READS):
        n = int(rng.integers(10, 301))
        start = int(rng.random() * (LONG_GENOME - n + 1))
        true = genome[start: start + n].copy()
        row = true.copy()
        errors = rng.random(size=n) < 0.01
        row[errors] = ((row[errors] - 1 + rng.integers(1, 4, size=int(errors.sum()))) % 4 + 1).astype(np.uint8)
        row[rng.random(size=n) < 0.003] = 5
        rows.append(row); truth.append(true)
    return rows, truth


def long_reads(seed=21):
    """600 reads of 10 .. 300 symbols of one genome of 4 000 iid symbols 1..4 (coverage 23): every symbol substituted with probability
    1 %, then set to 5 (N) with probability 0.3 %.  Returns (rows, true rows), fresh copies."""
    rows, truth = _long_reads(seed)
    return [r.copy() for r in rows], [t.copy() for t in truth]


# ------------------------------------------------------------------------------------------------------------------------------------
# Hand-made reads: a genome of 64 symbols whose windows are all solid (three copies in the collection), two decoys that make a
# candidate ambiguous, and reads cut out of the genome with errors put where a branch of the rule wants them.

HAND_K = 8
HAND_T = 3
AMBIG_FIRST = 30           # at this position the window that ENDS there has a second solid candidate
AMBIG_BOTH = 45            # at this one the window that ends there and the one that starts there both have


def _other(*symbols):
    """The smallest symbol 1..4 that is none of `symbols`."""
    return min(c for c in range(1, 5) if c not in symbols)


@functools.lru_cache(maxsize=None)
def _hand():
    k = HAND_K
    rng = np.random.default_rng(5)
    while True:
        g = rng.integers(1, 5, size=64).astype(np.uint8)
        if len({bytes(g[o: o + k - 1].tolist()) for o in range(64 - k + 2)}) == 64 - k + 2:      # all (k - 1)-mers distinct: no accidental candidates
            break
    G = g.tolist()
    d1 = _other(G[AMBIG_FIRST])
    d2 = _other(G[AMBIG_BOTH])
    decoys = [G[AMBIG_FIRST - k + 1: AMBIG_FIRST] + [d1],                 # shares the k - 1 symbols before AMBIG_FIRST
              G[AMBIG_BOTH - k + 1: AMBIG_BOTH] + [d2],
              [d2] + G[AMBIG_BOTH + 1: AMBIG_BOTH + k]]                    # shares the k - 1 symbols behind AMBIG_BOTH
    collection = [np.array(G, dtype=np.uint8)] * 3 + [np.array(d, dtype=np.uint8) for d in decoys for _ in range(3)]

    def cut(a, b, errors=()):
        """(read, truth): G[a: b] with (position in the read, symbol) substitutions."""
        true = G[a: b]
        read = list(true)
        for p, s in errors:
            read[p] = s
        return np.array(read, dtype=np.uint8), bytes(bytearray(true))

    def wrong(pos, *avoid):
        return _other(G[pos], *avoid)

    cases = []

    def add(name, read_truth, rounds, status, edits, restored=True):
        read, true = read_truth
        text = true if status in (CLEAN, CORRECTED) and restored else as_bytes(read)
        cases.append((name, read, rounds, status, text, edits))

    add("shorter than k", cut(3, 3 + k - 1, [(2, wrong(5))]), 10, SHORT, 0)
    add("empty", cut(0, 0), 10, SHORT, 0)
    add("m == k, clean", cut(10, 10 + k), 10, CLEAN, 0)
    add("m == k, one error: the two windows coincide", cut(10, 10 + k, [(3, wrong(13))]), 10, CORRECTED, 1)
    add("m == k + 1, error at 0", cut(10, 11 + k, [(0, wrong(10))]), 10, CORRECTED, 1)
    add("error at position 0", cut(2, 28, [(0, wrong(2))]), 10, CORRECTED, 1)
    add("error at k - 2", cut(2, 28, [(k - 2, wrong(2 + k - 2))]), 10, CORRECTED, 1)
    add("error at m - 1", cut(2, 28, [(25, wrong(27))]), 10, CORRECTED, 1)
    two = [(9, wrong(11)), (12, wrong(14))]
    add("two errors closer than k: two rounds", cut(2, 28, two), 2, CORRECTED, 2)
    add("two errors, R too small", cut(2, 28, two), 1, FAILED, 0)
    add("R = 0 on a clean read", cut(2, 28), 0, CLEAN, 0)
    add("R = 0 on an error", cut(2, 28, [(9, wrong(11))]), 0, FAILED, 0)
    a = AMBIG_FIRST - 12
    add("ambiguous first window, resolved by the second", cut(a, a + 26, [(12, wrong(AMBIG_FIRST, d1))]), 10, CORRECTED, 1)
    a = AMBIG_BOTH - 12
    add("ambiguous in both windows", cut(a, a + 26, [(12, wrong(AMBIG_BOTH, d2))]), 10, FAILED, 0)
    add("N at the error position", cut(2, 28, [(9, 5)]), 10, CORRECTED, 1)
    add("N elsewhere in the only window", cut(10, 10 + k, [(3, wrong(13)), (5, 5)]), 10, FAILED, 0)
    return collection, cases


def hand_made():
    """(collection, cases): the rows the table is counted from, and (name, read, rounds, status, text, edits) per hand-made read,
    with k = HAND_K, t = HAND_T, skip = 5.  The expectations are written down here, not computed by the brute force."""
    collection, cases = _hand()
    return [r.copy() for r in collection], [(n, r.copy(), R, s, t, e) for n, r, R, s, t, e in cases]
