"""What the matching-statistics and MEM tests expect, from the reads alone (not a test module): every substring of every row with its
count, the suffixes of the collection in the index's order, l(e) and the MEMs straight from their definitions -- plain Python over
the rows the test made, never the library's own search -- the patterns the tests search, and the calls of
bwtm_matching_stats_batch / bwtm_mem_batch on prefilled outputs with spare slots behind the end."""
import bisect

import numpy as np

from locate_inputs import FILL, SPARE

FILL32 = 0xEEEEEEEE


class Brute:
    """rows: the reads as sequences of comp values 1..5.  A substring W "occurs" when it is a substring of a row (nothing spans an
    endmarker); count(W) = its occurrences; sp(W) = the suffixes of the collection, endmarker suffixes included, that are smaller than W
    in the index's order: a suffix is a row's tail followed by the endmarker 0, which is below every symbol, so a tail that is a proper
    prefix of W is smaller than W and a tail that starts with W is not (the order among equal tails does not matter to a count)."""

    def __init__(self, rows):
        self.rows = [bytes(int(v) for v in r) for r in rows]
        self.counts = {}
        for r in self.rows:
            for o in range(len(r)):
                for e in range(o + 1, len(r) + 1):
                    w = r[o:e]
                    self.counts[w] = self.counts.get(w, 0) + 1
        self.suffixes = sorted(r[o:] + b"\x00" for r in self.rows for o in range(len(r) + 1))

    def occurs(self, w):
        return bytes(w) in self.counts

    def count(self, w):
        return self.counts.get(bytes(w), 0)

    def sp(self, w):
        return bisect.bisect_left(self.suffixes, bytes(w))

    def lengths(self, p):
        """[l(1), .., l(m)]: the largest l <= e such that p[e-l: e] occurs."""
        p = bytes(int(v) for v in p)
        return [next((l for l in range(e, 0, -1) if p[e - l:e] in self.counts), 0) for e in range(1, len(p) + 1)]

    def stats(self, p):
        """[(l, sp, count)] per symbol of p; (0, 0, 0) where l = 0."""
        p = bytes(int(v) for v in p)
        out = []
        for e, l in enumerate(self.lengths(p), start=1):
            w = p[e - l:e]
            out.append((l, self.sp(w), self.counts[w]) if l > 0 else (0, 0, 0))
        return out

    def mems(self, p, min_length=1):
        """[(b, l, sp, count)] by the three conditions: p[b: b+l] occurs, b == 0 or p[b-1: b+l] does not, b + l == m or p[b: b+l+1] does
        not; ascending b.  (The inner loop stops at the first l that does not occur: no longer one from the same b can.)"""
        p = bytes(int(v) for v in p)
        m, out = len(p), []
        for b in range(m):
            for l in range(1, m - b + 1):
                w = p[b:b + l]
                if w not in self.counts:
                    break
                if l >= min_length and (b == 0 or p[b - 1:b + l] not in self.counts) and (b + l == m or p[b:b + l + 1] not in self.counts):
                    out.append((b, l, self.sp(w), self.counts[w]))
        return out


def rule_mems(lengths, min_length=1):
    """[(b, l)] by the rule on matching statistics: end e gives one iff l(e) >= min_length and (e == m or l(e+1) <= l(e))."""
    m = len(lengths)
    return [(e - lengths[e - 1], lengths[e - 1]) for e in range(1, m + 1)
            if lengths[e - 1] >= max(min_length, 1) and (e == m or lengths[e] <= lengths[e - 1])]


def expected_stats(brute, patterns):
    """(lengths uint32, sp, count) over all symbols of the patterns."""
    rows = [s for p in patterns for s in brute.stats(p)]
    return (np.array([r[0] for r in rows], dtype=np.uint32), np.array([r[1] for r in rows], dtype=np.uint64), np.array([r[2] for r in rows], dtype=np.uint64))


def expected_mems(brute, patterns, min_length=1):
    """(hit_offsets, begin uint32, length uint32, sp, count) of a list of patterns."""
    hit_offsets, rows = [0], []
    for p in patterns:
        rows.extend(brute.mems(p, min_length))
        hit_offsets.append(len(rows))
    return (np.array(hit_offsets, dtype=np.uint64), np.array([r[0] for r in rows], dtype=np.uint32), np.array([r[1] for r in rows], dtype=np.uint32),
            np.array([r[2] for r in rows], dtype=np.uint64), np.array([r[3] for r in rows], dtype=np.uint64))


def varied_patterns(rows, seed):
    """Every non-empty read with one substitution, with a symbol before and behind it, and joined to the next read (longer than any
    sequence: its matches end at the endmarker between the two)."""
    rng = np.random.default_rng(seed)
    out = []
    full = [r for r in rows if len(r) > 0]
    for k, r in enumerate(full):
        r = list(r)
        s = list(r)
        i = int(rng.integers(0, len(s)))
        s[i] = 1 + (s[i] - 1 + int(rng.integers(1, 4))) % 4
        out.append(tuple(s))
        out.append((int(rng.integers(1, 5)),) + tuple(r) + (int(rng.integers(1, 5)),))
        out.append(tuple(r) + tuple(full[(k + 1) % len(full)]))
    return out


def special_patterns(rows, seed):
    """The batch of edge cases: empty patterns at the front, in the middle and at the end, one-symbol patterns, a pattern of the largest
    symbol only, the lexicographically largest suffix of the collection alone and behind every symbol (the search's range ends at the
    last position of the index: rank(n, .) from C), a pattern of a symbol the reads do not hold, and a 100-symbol pattern that ends in a
    whole read."""
    rng = np.random.default_rng(seed)
    largest = max(tuple(r[o:]) for r in rows for o in range(len(r) + 1))
    top = max(v for r in rows for v in r)
    assert top == 4 and len(largest) >= 1
    whole = next(tuple(r) for r in rows if len(r) == 40)
    long_one = tuple(int(v) for v in rng.integers(1, 5, size=60)) + whole
    assert len(long_one) == 100
    out = [(), (), (1,), (2,), (3,), (4,), (5,), (top,) * 37, largest, (), ()]
    out += [(c,) + largest for c in (1, 2, 3, 4, 5)]
    out += [(5,) * 9, (5, 5) + tuple(rows[1][:7]) + (5,) + tuple(rows[2][:3]), long_one, long_one[:77], (), ()]
    return out


def pack(gpu, patterns):
    """(text, offsets, their ctypes pointers) of a list of patterns."""
    offsets = np.zeros(len(patterns) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(p) for p in patterns])
    text = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.uint8) for p in patterns] + [np.zeros(0, dtype=np.uint8)]))
    return text, offsets, text.ctypes.data_as(gpu.capi.p_u8), offsets.ctypes.data_as(gpu.capi.p_u64)


def stats_raw(gpu, x, patterns):
    """bwtm_matching_stats_batch on outputs prefilled with 0xEE.. and SPARE entries longer than needed."""
    text, offsets, tp, op = pack(gpu, patterns)
    total = int(offsets[-1])
    lengths = np.full(total + SPARE, FILL32, dtype=np.uint32)
    sp = np.full(total + SPARE, FILL, dtype=np.uint64)
    count = np.full(total + SPARE, FILL, dtype=np.uint64)
    gpu.capi.check(gpu.capi.lib().bwtm_matching_stats_batch(x.h, tp, op, len(patterns), lengths.ctypes.data_as(gpu.capi.p_u32), sp.ctypes.data_as(gpu.capi.p_u64),
                                                            count.ctypes.data_as(gpu.capi.p_u64)))
    assert np.all(lengths[total:] == FILL32) and np.all(sp[total:] == FILL) and np.all(count[total:] == FILL), "entries behind the last symbol were written"
    return lengths[:total], sp[:total], count[:total]


def mems_raw(gpu, x, patterns, min_length, spare=SPARE):
    """The sizing call and the filling call of bwtm_mem_batch, outputs prefilled with 0xEE.. and `spare` slots longer than needed (the
    capacity passed is the exact one when spare == 0, and the guard slots are then beyond it)."""
    lib, p_u64, p_u32 = gpu.capi.lib(), gpu.capi.p_u64, gpu.capi.p_u32
    text, offsets, tp, op = pack(gpu, patterns)
    hit_offsets = np.full(len(patterns) + 1, FILL, dtype=np.uint64)
    gpu.capi.check(lib.bwtm_mem_batch(x.h, tp, op, len(patterns), int(min_length), hit_offsets.ctypes.data_as(p_u64), None, None, None, None, 0))
    sized = hit_offsets.copy()
    total = int(hit_offsets[-1])
    begin = np.full(total + SPARE, FILL32, dtype=np.uint32)
    length = np.full(total + SPARE, FILL32, dtype=np.uint32)
    sp = np.full(total + SPARE, FILL, dtype=np.uint64)
    count = np.full(total + SPARE, FILL, dtype=np.uint64)
    hit_offsets[:] = FILL
    gpu.capi.check(lib.bwtm_mem_batch(x.h, tp, op, len(patterns), int(min_length), hit_offsets.ctypes.data_as(p_u64), begin.ctypes.data_as(p_u32), length.ctypes.data_as(p_u32),
                                      sp.ctypes.data_as(p_u64), count.ctypes.data_as(p_u64), total + spare))
    assert np.array_equal(hit_offsets, sized), "the sizing call and the filling call disagree about the hit offsets"
    assert np.all(begin[total:] == FILL32) and np.all(length[total:] == FILL32) and np.all(sp[total:] == FILL) and np.all(count[total:] == FILL), \
        "slots behind hit_offsets[count] were written"
    return hit_offsets, begin[:total], length[:total], sp[:total], count[:total]


def same(got, want):
    return len(got) == len(want) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
