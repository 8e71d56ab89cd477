"""What the edit-distance search tests expect, from the reads alone (not a test module): the hits of a pattern within Levenshtein distance e
by brute force -- the textbook full matrix of every distinct endmarker-free window of every length m - e .. m + e against the pattern,
vectorised over the windows; no band, no trie, never the library's own search, and no FM index.  tests/test_find_edit_host.py pins it to
the oracle and to the Hamming brute force of tests/approx_inputs.py, on whose Collection it is built.  The collections are those of the
k-mer tests (tests/kmer_inputs.py)."""
import functools

import numpy as np

from approx_inputs import Collection, _keys, cut_patterns, genome_reads, iid_reads, text_of          # noqa: F401  (the GPU tests take the collections from here)


def columns(windows, pattern):
    """D[w, i] = ed(windows[w], the LAST i symbols of the pattern), i = 0 .. m: the last row of the full Levenshtein matrix of the
    reversed window against the reversed pattern (cost 1 per insertion, deletion and substitution), one matrix per window, cell by cell."""
    p = np.asarray(pattern, dtype=np.uint8)[::-1]
    w = np.asarray(windows, dtype=np.uint8)[:, ::-1]
    count, length = w.shape
    m = int(p.size)
    cell = np.int8 if max(length, m) < 100 else np.int32                                  # no entry exceeds the longer of the two strings
    row = np.broadcast_to(np.arange(m + 1, dtype=cell), (count, m + 1)).copy(order="F")  # the empty window: i insertions
    for a in range(1, length + 1):
        new = np.empty_like(row)                                           # column-major: a cell of every window is one stretch of memory
        new[:, 0] = a
        for b in range(1, m + 1):
            new[:, b] = np.minimum(np.minimum(row[:, b - 1] + (w[:, a - 1] != p[b - 1]), row[:, b] + 1), new[:, b - 1] + 1)
        row = new
    return row


class EditCollection(Collection):
    """approx_inputs.Collection with, per length, the distinct endmarker-free windows, and per pattern the distances to them."""

    def __init__(self, rows):
        Collection.__init__(self, rows)
        self._distinct, self._sorted, self._columns = {}, {}, {}

    def distinct(self, length):
        """(strings [k, length] ascending, counts [k], inverse [occurrences] -> string, positions [occurrences] in the text)."""
        if length not in self._distinct:
            w, valid, sorted_keys = self.windows(length)
            del self._windows[length]                                     # n x length bytes each: only what is asked for again is kept
            self._sorted[length] = sorted_keys
            at = np.flatnonzero(valid)
            if at.size == 0:
                self._distinct[length] = (np.zeros((0, length), dtype=np.uint8), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), at)
            else:
                strings, inverse, counts = np.unique(w[at], axis=0, return_inverse=True, return_counts=True)
                self._distinct[length] = (strings, counts.astype(np.int64), np.asarray(inverse).ravel(), at)
        return self._distinct[length]

    def distances(self, pattern, length):
        """columns() of the distinct windows of one length against the pattern, computed once."""
        key = (np.asarray(pattern, dtype=np.uint8).tobytes(), length)
        if key not in self._columns:
            self._columns[key] = columns(self.distinct(length)[0], pattern)
        return self._columns[key]

    def edit_hits(self, pattern, e, want_occurrences=False):
        """(sp, count, edits, lengths, strings [list]) of the hits of `pattern` within edit distance e, in the documented order: shortest first,
        within a length ascending when the strings are compared from their last symbol backwards.  With want_occurrences also the set of
        (sequence, offset, edits, length) of all occurrences."""
        p = np.asarray(pattern, dtype=np.uint8)
        m = int(p.size)
        sp, count, edits, lengths, strings, occurrences = [], [], [], [], [], set()
        for length in range(max(0, m - e), m + e + 1):
            if length == 0:                                               # the empty string: everywhere, at the cost of m insertions
                sp.append(0); count.append(self.n); edits.append(m); lengths.append(0); strings.append(np.zeros(0, dtype=np.uint8))
                continue
            distinct, counts, inverse, at = self.distinct(length)
            if distinct.shape[0] == 0:
                continue
            dist = self.distances(p, length)[:, m]
            near = np.flatnonzero(dist <= e)
            if near.size == 0:
                continue
            found = distinct[near]
            first = np.searchsorted(self._sorted[length], _keys(found, length), side="left")
            assert np.array_equal(np.searchsorted(self._sorted[length], _keys(found, length), side="right") - first, counts[near])
            order = np.lexsort(found.T)                                   # the last key is the primary one: the last symbol, then the one before
            for j in order.tolist():
                sp.append(int(first[j])); count.append(int(counts[near[j]])); edits.append(int(dist[near[j]])); lengths.append(length); strings.append(found[j])
            if want_occurrences:
                is_near = np.zeros(distinct.shape[0], dtype=bool); is_near[near] = True
                for o in np.flatnonzero(is_near[inverse]).tolist():
                    i = int(at[o])
                    occurrences.add((int(self.seq_of[i]), int(self.off_of[i]), int(dist[inverse[o]]), length))
        out = (np.array(sp, dtype=np.uint64), np.array(count, dtype=np.uint64), np.array(edits, dtype=np.uint8), np.array(lengths, dtype=np.uint32), strings)
        return out + (occurrences,) if want_occurrences else out

    def edit_frontier(self, pattern, e):
        """nodes[t], t = 0 .. max(m + e, 1) - 1: the nodes of the search at depth t -- one root, then the distinct strings W of t symbols that occur
        inside a sequence and are viable: the least of ed(W, last i symbols of the pattern), i = 0 .. m, is <= e.  A node at depth m + e has
        no viable child and is not kept."""
        p = np.asarray(pattern, dtype=np.uint8)
        nodes = [1]
        for t in range(1, int(p.size) + e):
            if self.distinct(t)[0].shape[0] == 0:
                nodes.append(0)
            else:
                nodes.append(int((self.distances(p, t).min(axis=1) <= e).sum()))
        return nodes


@functools.lru_cache(maxsize=None)
def collection(name):
    return EditCollection(list({"iid": iid_reads, "genome": genome_reads}[name]()))


def expected(coll, patterns, e, max_hits=0):
    """(hit_offsets, sp, count, edits, lengths) of a whole call."""
    parts = [coll.edit_hits(p, e)[:4] for p in patterns]
    if max_hits > 0:
        parts = [tuple(a[:max_hits] for a in part) for part in parts]
    hit_offsets = np.zeros(len(patterns) + 1, dtype=np.uint64)
    hit_offsets[1:] = np.cumsum([part[0].size for part in parts])
    cat = lambda j, dtype: np.concatenate([part[j] for part in parts] + [np.zeros(0, dtype=dtype)]).astype(dtype)
    return hit_offsets, cat(0, np.uint64), cat(1, np.uint64), cat(2, np.uint8), cat(3, np.uint32)


def batch_peaks(coll, patterns, e):
    """(P, H, T) of the documented memory bound for one batch that holds all `patterns`: the largest frontier (all patterns advance together,
    one symbol per level; the first frontier has a root per pattern), the hits, the bytes of pattern text."""
    per_level = {}
    hits = 0
    for p in patterns:
        for t, nodes in enumerate(coll.edit_frontier(p, e)):
            per_level[t] = per_level.get(t, 0) + nodes
        hits += int(coll.edit_hits(p, e)[0].size)
    return max(per_level.values()), hits, sum(len(p) for p in patterns)


def peak_formula(P, H, T, e):
    """The documented bound of bwtm_find_edit_batch's device memory beyond the index (include/bwtm.h)."""
    return (308 + 34 * e) * P + 132 * H + 2 * T + (1 << 20)


def edited_patterns(rows, lengths, per_length, seed, edits=1):
    """per_length patterns of every length, cut from random rows at random offsets, each with `edits` random edits -- a substitution, an
    insertion or a deletion, equally likely -- and of exactly the asked length afterwards: the piece cut is longer by the deletions and
    shorter by the insertions; a piece beyond the row takes the whole row and continues with random symbols."""
    rng = np.random.default_rng(seed)
    out = []
    for m in lengths:
        for _ in range(per_length):
            ops = [int(rng.integers(0, 3)) for _ in range(edits if m > 0 else 0)]           # 0 substitution, 1 insertion, 2 deletion
            cut = max(m + ops.count(2) - ops.count(1), 0)
            row = np.asarray(rows[int(rng.integers(0, len(rows)))], dtype=np.uint8)
            if cut <= row.size:
                o = int(rng.integers(0, row.size - cut + 1))
                p = row[o: o + cut].copy()
            else:
                p = np.concatenate([row, rng.integers(1, 5, size=cut - row.size).astype(np.uint8)])
            for op in ops:
                if op == 1 or p.size == 0:
                    j = int(rng.integers(0, p.size + 1))
                    p = np.concatenate([p[:j], rng.integers(1, 5, size=1).astype(np.uint8), p[j:]])
                elif op == 2:
                    j = int(rng.integers(0, p.size))
                    p = np.concatenate([p[:j], p[j + 1:]])
                else:
                    j = int(rng.integers(0, p.size))
                    p[j] = (int(p[j]) - 1 + int(rng.integers(1, 4))) % 4 + 1
            p = p[:m] if p.size >= m else np.concatenate([p, rng.integers(1, 5, size=m - p.size).astype(np.uint8)])
            out.append(np.ascontiguousarray(p, dtype=np.uint8))
    return out


MIXED_LENGTHS = (0, 1, 2, 3, 12, 31, 40, 41)


def mixed_patterns(name):
    """The patterns of the mixed case, in mixed order, so that they finish at different levels: six of every length up to 12 and two of every
    longer one (the brute force pays for those) with one random edit each, four 12-mers with two, and two random strings."""
    rows, seed = collection(name).rows, (7 if name == "iid" else 8)
    patterns = edited_patterns(rows, MIXED_LENGTHS[:5], 6, seed) + edited_patterns(rows, MIXED_LENGTHS[5:], 2, seed + 10) + edited_patterns(rows, (12,), 4, seed + 20, edits=2)
    patterns += [np.random.default_rng(seed + 30).integers(1, 5, size=m).astype(np.uint8) for m in (31, 41)]     # not from any read: no hit within two edits
    order = np.random.default_rng(9).permutation(len(patterns))
    return [patterns[j] for j in order.tolist()]


def mixed_budget(patterns, e):
    """The patterns of the mixed case that run at budget e: all of them up to e = 2, those of at most 12 symbols at e = 3."""
    return [p for p in patterns if e <= 2 or len(p) <= 12]


@functools.lru_cache(maxsize=None)
def mixed_expected(name, e):
    return expected(collection(name), mixed_budget(mixed_patterns(name), e), e)


@functools.lru_cache(maxsize=None)
def mixed_peaks(name, e):
    return batch_peaks(collection(name), mixed_budget(mixed_patterns(name), e), e)


def memory_patterns():
    """The batch of the memory-bound test: eight 12-mers of the iid collection with one substitution each, searched at e = 3."""
    return cut_patterns(collection("iid").rows, (12,), 8, 41)


def within_one_edit(pattern):
    """Every string over comp values 1..5 within one edit of the pattern, with its distance: {bytes: 0 or 1}."""
    p = np.asarray(pattern, dtype=np.uint8)
    found = {p.tobytes(): 0}
    for j in range(p.size):
        found.setdefault(np.concatenate([p[:j], p[j + 1:]]).tobytes(), 1)
        for c in range(1, 6):
            q = p.copy(); q[j] = c
            found.setdefault(q.tobytes(), 1)
    for j in range(p.size + 1):
        for c in range(1, 6):
            found.setdefault(np.concatenate([p[:j], np.array([c], dtype=np.uint8), p[j:]]).tobytes(), 1)
    return found
