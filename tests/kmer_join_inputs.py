"""What the k-mer join tests expect, from the reads alone (not a test module): two collections of 2 000 reads of 40 symbols cut with 1 % errors
from two genomes of 3 000 symbols -- the second genome is the first with about 1 % substitutions and one inserted stretch -- and, for any two
lists of reads, the k-mers of either with their count in each and their insertion point in each: sliding windows over the rows, np.unique on
the codes and np.searchsorted(..., side="left") on the sorted windows, which gives the position of an absent k-mer as well; never the library's
own search.  tests/test_kmer_join_host.py checks it against the oracle."""
import functools

import numpy as np

from kmer_inputs import _keys, decode, kept_comps, text_of

READS = 2000
WIDTH = 40
GENOME = 3000
INSERT_AT, INSERT = 1700, 120          # the stretch that only the second genome holds
NO_BOUND = (1 << 64) - 1


def _cut(genome, rng):
    starts = rng.integers(0, genome.size - WIDTH + 1, size=READS)
    rows = genome[starts[:, None] + np.arange(WIDTH)[None, :]].copy()
    errors = rng.random(size=rows.shape) < 0.01
    rows[errors] = ((rows[errors] - 1 + rng.integers(1, 4, size=int(errors.sum()))) % 4 + 1).astype(np.uint8)
    return rows


@functools.lru_cache(maxsize=None)
def _pair(seed):
    rng = np.random.default_rng(seed)
    first = rng.integers(1, 5, size=GENOME).astype(np.uint8)
    second = first.copy()
    changed = rng.random(size=GENOME) < 0.01
    second[changed] = ((second[changed] - 1 + rng.integers(1, 4, size=int(changed.sum()))) % 4 + 1).astype(np.uint8)
    second = np.concatenate([second[:INSERT_AT], rng.integers(1, 5, size=INSERT).astype(np.uint8), second[INSERT_AT:]])
    return _cut(first, rng), _cut(second, rng)


def pair_reads(seed=31):
    """(rows_a, rows_b): 2 000 x 40 comp values 1..4 each (coverage 27 and 26)."""
    a, b = _pair(seed)
    return a.copy(), b.copy()


def _side(rows, k, skip):
    """One collection: its sorted windows (the order of its suffixes as far as a k-mer can tell, kmer_inputs.brute) and its k-mers with counts."""
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
    return np.sort(_keys(windows, k)), codes, counts.astype(np.uint64)


def brute_pair(rows_a, rows_b, k, skip, min_a=0, max_a=None, min_b=0, max_b=None, min_sum=1):
    """(codes, count_a, count_b, sp_a, sp_b) of the k-mers that either list of rows holds and the bounds keep, ascending by code.
    sp_x = the number of windows of x that are smaller than the k-mer: the first position of its range, or its insertion point."""
    sides = [_side(list(rows), k, skip) for rows in (rows_a, rows_b)]
    codes = np.union1d(sides[0][1], sides[1][1])
    keys = _keys(decode(codes, k, skip), k)
    counts, sps = [], []
    for sorted_keys, own, own_counts in sides:
        c = np.zeros(codes.size, dtype=np.uint64)
        c[np.searchsorted(codes, own, side="left")] = own_counts
        counts.append(c)
        sps.append(np.searchsorted(sorted_keys, keys, side="left").astype(np.uint64))
    keep = (counts[0] >= np.uint64(min_a)) & (counts[1] >= np.uint64(min_b)) & (counts[0] + counts[1] >= np.uint64(max(int(min_sum), 1)))
    keep &= (counts[0] <= np.uint64(NO_BOUND if max_a is None else max_a)) & (counts[1] <= np.uint64(NO_BOUND if max_b is None else max_b))
    return codes[keep], counts[0][keep], counts[1][keep], sps[0][keep], sps[1][keep]


def brute_pair_levels(rows_a, rows_b, k, skip, min_a=0, max_a=None, min_b=0, max_b=None, min_sum=1):
    """nodes[t] for t < k - 1 = the (t + 1)-mers the lower bounds keep; nodes[k - 1] = the k-mers all bounds keep."""
    inner = [brute_pair(rows_a, rows_b, t + 1, skip, min_a, None, min_b, None, min_sum)[0].size for t in range(k - 1)]
    return np.array(inner + [brute_pair(rows_a, rows_b, k, skip, min_a, max_a, min_b, max_b, min_sum)[0].size], dtype=np.uint64)


def classes(want):
    """The seven numbers of bwtm_kmer_join_summary from a brute_pair result."""
    codes, ca, cb = want[0], want[1], want[2]
    only_a, only_b, both = (ca > 0) & (cb == 0), (ca == 0) & (cb > 0), (ca > 0) & (cb > 0)
    return [int(only_a.sum()), int(only_b.sum()), int(both.sum()), int(ca[only_a].sum()), int(cb[only_b].sum()), int(ca[both].sum()), int(cb[both].sum())]


def peak_formula(levels):
    """The documented bound of bwtm_kmer_join_create's device memory beyond the two indexes (include/bwtm.h): 392 P + 2^20, P = the largest level."""
    return 392 * int(max(levels.tolist() + [0])) + (1 << 20)
