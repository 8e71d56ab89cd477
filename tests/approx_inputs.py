"""What the bounded-mismatch search tests expect, from the reads alone (not a test module): the hits of a pattern with up to d substitutions by
brute force over every window of the text -- never the library's own search, and no FM index.  tests/test_find_approx_host.py pins it to
the oracle.  The collections are those of the k-mer tests (tests/kmer_inputs.py)."""
import numpy as np

from kmer_inputs import genome_reads, iid_reads, text_of          # noqa: F401  (the GPU tests take the collections from here)


def _keys(windows, m):
    return np.ascontiguousarray(windows).view("S%d" % m).ravel()


class Collection:
    """The text of a list of rows and, per pattern length, its windows.  Every position of the text starts a window of m symbols, cut behind
    its first endmarker (zeros from there on: the endmarker is the smallest symbol and a hit holds none, so sorting the windows is the
    order of the suffixes as far as a string of m symbols can tell)."""

    def __init__(self, rows):
        self.rows = [np.asarray(r, dtype=np.uint8) for r in rows]
        self.text = text_of(self.rows)
        self.n = int(self.text.size)
        lens = np.array([r.size for r in self.rows], dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(lens + 1)[:-1]]).astype(np.int64)
        self.seq_of = np.repeat(np.arange(len(self.rows), dtype=np.int64), lens + 1)
        self.off_of = np.arange(self.n, dtype=np.int64) - starts[self.seq_of]
        self._windows = {}

    def windows(self, m):
        """(windows [n, m], valid [n]: the window holds no endmarker, the sorted keys of all windows)."""
        if m not in self._windows:
            padded = np.concatenate([self.text, np.zeros(m, dtype=np.uint8)])
            w = np.lib.stride_tricks.sliding_window_view(padded, m)[: self.n].copy()
            w[np.cumsum(w == 0, axis=1) > 0] = 0
            self._windows[m] = (w, ~(w == 0).any(axis=1), np.sort(_keys(w, m)))
        return self._windows[m]

    def hits(self, pattern, d, want_occurrences=False):
        """(sp, count, mismatches, strings [hits, m]) of the hits of `pattern` within Hamming distance d, in the documented order: ascending
        when the strings are compared from their last symbol backwards.  The windows without endmarker within distance d are the occurrences,
        the distinct ones the hits, sp = the number of windows smaller than the hit.  With want_occurrences also the set of
        (sequence, offset, mismatches) of all occurrences."""
        p = np.asarray(pattern, dtype=np.uint8)
        m = int(p.size)
        if m == 0:
            out = (np.zeros(1, dtype=np.uint64), np.full(1, self.n, dtype=np.uint64), np.zeros(1, dtype=np.uint8), np.zeros((1, 0), dtype=np.uint8))
            return out + (set(),) if want_occurrences else out
        w, valid, sorted_keys = self.windows(m)
        dist = (w != p[None, :]).sum(axis=1)
        occ = np.flatnonzero(valid & (dist <= d))
        if occ.size == 0:
            out = (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8), np.zeros((0, m), dtype=np.uint8))
            return out + (set(),) if want_occurrences else out
        strings, inverse = np.unique(w[occ], axis=0, return_inverse=True)
        inverse = np.asarray(inverse).ravel()
        count = np.bincount(inverse, minlength=strings.shape[0])
        sp = np.searchsorted(sorted_keys, _keys(strings, m), side="left")
        assert np.array_equal(np.searchsorted(sorted_keys, _keys(strings, m), side="right") - sp, count)
        order = np.lexsort(strings.T)                                    # the last key is the primary one: the last symbol, then the one before
        out = (sp[order].astype(np.uint64), count[order].astype(np.uint64), (strings[order] != p[None, :]).sum(axis=1).astype(np.uint8), strings[order])
        if want_occurrences:
            return out + ({(int(self.seq_of[i]), int(self.off_of[i]), int(dist[i])) for i in occ.tolist()},)
        return out

    def frontier(self, pattern, d):
        """nodes[t], t = 0 .. m - 1: the nodes of the search of `pattern` that have matched t symbols -- one root, then the distinct strings of t
        symbols that occur inside a sequence within distance d of the pattern's last t symbols."""
        p = np.asarray(pattern, dtype=np.uint8)
        nodes = [1]
        for t in range(1, int(p.size)):
            w, valid, _ = self.windows(t)
            near = w[valid & ((w != p[None, p.size - t:]).sum(axis=1) <= d)]
            nodes.append(int(np.unique(_keys(near, t)).size))
        return nodes


def expected(collection, patterns, d, max_hits=0):
    """(hit_offsets, sp, count, mismatches) of a whole call."""
    parts = [collection.hits(p, d)[:3] for p in patterns]
    if max_hits > 0:
        parts = [tuple(a[:max_hits] for a in part) for part in parts]
    hit_offsets = np.zeros(len(patterns) + 1, dtype=np.uint64)
    hit_offsets[1:] = np.cumsum([part[0].size for part in parts])
    cat = lambda j, dtype: np.concatenate([part[j] for part in parts] + [np.zeros(0, dtype=dtype)]).astype(dtype)
    return hit_offsets, cat(0, np.uint64), cat(1, np.uint64), cat(2, np.uint8)


def batch_peaks(collection, patterns, d):
    """(P, H, T) of the documented memory bound for one batch that holds all `patterns`: the largest frontier (all patterns advance together,
    one symbol per level; the first frontier has a root per pattern), the hits, the bytes of pattern text."""
    per_level = {}
    hits = 0
    for p in patterns:
        if len(p) == 0:
            per_level[0] = per_level.get(0, 0) + 1
            hits += 1
            continue
        for t, nodes in enumerate(collection.frontier(p, d)):
            per_level[t] = per_level.get(t, 0) + nodes
        hits += int(collection.hits(p, d)[0].size)
    return max(per_level.values()), hits, sum(len(p) for p in patterns)


def peak_formula(P, H, T):
    """The documented bound of bwtm_find_approx_batch's device memory beyond the index (include/bwtm.h)."""
    return 240 * P + 128 * H + 2 * T + (1 << 20)


def cut_patterns(rows, lengths, per_length, seed, substitutions=1):
    """per_length patterns of every length, cut from random rows at random offsets, each with `substitutions` random substitutions (1..4); a
    length beyond the row takes the whole row and continues with random symbols."""
    rng = np.random.default_rng(seed)
    out = []
    for m in lengths:
        for _ in range(per_length):
            row = np.asarray(rows[int(rng.integers(0, len(rows)))], dtype=np.uint8)
            if m <= row.size:
                o = int(rng.integers(0, row.size - m + 1))
                p = row[o: o + m].copy()
            else:
                p = np.concatenate([row, rng.integers(1, 5, size=m - row.size).astype(np.uint8)])
            for _ in range(substitutions if m > 0 else 0):
                j = int(rng.integers(0, m))
                p[j] = (int(p[j]) - 1 + int(rng.integers(1, 4))) % 4 + 1
            out.append(p)
    return out


def neighbours(pattern, d):
    """Every string within Hamming distance d of the pattern over comp values 1..5, with its distance: {bytes: distance}."""
    p = np.asarray(pattern, dtype=np.uint8)
    found = {p.tobytes(): 0}
    layer = [p]
    for dist in range(1, d + 1):
        nxt = []
        for q in layer:
            for j in range(q.size):
                for c in range(1, 6):
                    if c != q[j]:
                        r = q.copy(); r[j] = c
                        key = r.tobytes()
                        if key not in found:
                            found[key] = dist; nxt.append(r)
        layer = nxt
    return {k: int((np.frombuffer(k, dtype=np.uint8) != p).sum()) for k in found}
