"""What the k-mer tests expect, from the reads alone (not a test module): two collections of 2 000 reads of 40 symbols and the distinct k-mers
of any list of reads with their counts and the first position of their BWT range -- a sliding window over the rows, np.unique on the codes,
windows that hold the skip symbol or an endmarker dropped; never the library's own search.  tests/test_kmers_host.py checks it against the oracle."""
import numpy as np

READS = 2000
WIDTH = 40
GENOME = 3000
RECORD = 128                       # positions per record (bwtm_device.h: REC_POS)
SUPER = 1 << 25                    # positions per super row (tests/boundary_inputs.py: SUPER)


def iid_reads(seed=11):
    """2 000 rows of 40 comp values, uniform over 1..4 with 1 % of 5 (N): most 12-mers occur once."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(1, 5, size=(READS, WIDTH)).astype(np.uint8)
    rows[rng.random(size=rows.shape) < 0.01] = 5
    return rows


def genome_reads(seed=12):
    """2 000 windows of 40 symbols of one genome of 3 000 symbols 1..4 (coverage 27), every symbol substituted with probability 1 %."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(1, 5, size=GENOME).astype(np.uint8)
    starts = rng.integers(0, GENOME - WIDTH + 1, size=READS)
    rows = genome[starts[:, None] + np.arange(WIDTH)[None, :]].copy()
    errors = rng.random(size=rows.shape) < 0.01
    rows[errors] = ((rows[errors] - 1 + rng.integers(1, 4, size=int(errors.sum()))) % 4 + 1).astype(np.uint8)
    return rows


def text_of(rows):
    """A list of rows (1-D arrays of comp values 1..5, any lengths) -> the text: every row followed by an endmarker 0."""
    parts = []
    for row in rows:
        parts.append(np.asarray(row, dtype=np.uint8)); parts.append(np.zeros(1, dtype=np.uint8))
    return np.concatenate(parts + [np.zeros(0, dtype=np.uint8)])


def kept_comps(skip):
    return np.array([c for c in range(1, 6) if c != skip], dtype=np.uint8)


def decode(codes, k, skip):
    """Codes -> rows of k comp values (the test's own decoder, not the binding's)."""
    codes = np.asarray(codes, dtype=np.uint64)
    shifts = np.array([2 * (k - 1 - j) for j in range(k)], dtype=np.uint64)
    return kept_comps(skip)[((codes[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.int64)]


def _keys(windows, k):
    return np.ascontiguousarray(windows).view("S%d" % k).ravel()


def brute(rows, k, skip, min_count=1):
    """(codes, counts, sp) of the k-mers of `rows` with count >= max(min_count, 1), ascending by code.
    Every position of the text starts a window of k symbols, cut behind its first endmarker (zeros from there on: the endmarker is the
    smallest symbol, and a k-mer holds none, so this is the order of the suffixes as far as a k-mer can tell).  A window without endmarker
    and without skip is an occurrence of a k-mer; sp = the number of windows that are smaller than the k-mer."""
    text = text_of(rows)
    n = text.size
    padded = np.concatenate([text, np.zeros(k, dtype=np.uint8)])
    windows = np.lib.stride_tricks.sliding_window_view(padded, k)[:n].copy()
    windows[np.cumsum(windows == 0, axis=1) > 0] = 0
    valid = ~((windows == 0) | (windows == skip)).any(axis=1)
    rank = np.zeros(6, dtype=np.uint64)
    rank[kept_comps(skip)] = np.arange(4, dtype=np.uint64)
    occ = windows[valid]
    codes = np.zeros(occ.shape[0], dtype=np.uint64)
    for j in range(k):
        codes |= rank[occ[:, j]] << np.uint64(2 * (k - 1 - j))
    codes, counts = np.unique(codes, return_counts=True)
    sorted_keys = np.sort(_keys(windows, k))
    sp = np.searchsorted(sorted_keys, _keys(decode(codes, k, skip), k), side="left")
    keep = counts >= max(int(min_count), 1)
    return codes[keep], counts[keep].astype(np.uint64), sp[keep].astype(np.uint64)


def brute_levels(rows, k, skip, min_count=1):
    """nodes[t] = distinct (t + 1)-mers with count >= min_count, t < k."""
    return np.array([brute(rows, t + 1, skip, min_count)[0].size for t in range(k)], dtype=np.uint64)


def folded_histogram(counts, bins):
    """np.bincount of the counts with everything from bins - 1 on folded into the last bin."""
    hist = np.bincount(np.minimum(np.asarray(counts, dtype=np.int64), bins - 1), minlength=bins)
    return hist.astype(np.uint64)


def peak_formula(levels):
    """The documented bound of bwtm_kmers_create's device memory beyond the index (include/bwtm.h): 240 P + 2^20, P = the largest level."""
    return 240 * int(max(levels.tolist() + [0])) + (1 << 20)
