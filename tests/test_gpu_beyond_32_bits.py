"""Every query family on indexes of more than 2^25 and of more than 2^32 positions (the product's own sizes: BASELINE config 2 is n = 5.05e9).

The collection R x c holds every read of a small collection R c times in a row.  Its BWT is the BWT of R with every symbol repeated c
times (oracle.FMI.from_runs states such an index in a few hundred kilobytes), and every query result on it is an exact arithmetic
image of the result on R: tests/scaled_inputs.py states the rules, tests/test_scaled_inputs_host.py pins them without a GPU, and the
brute forces of the families' own tests compute the result on R.  Two sizes: "super" puts n' a little above 2^25 positions, so that a
second row of the super table is read; "wide" puts n' beyond 2^32 with 2^32 inside the class of one symbol, so that positions, ranges,
insertion points and prefix sums on both sides of 2^32 and ranges that straddle it come back.  Before it looks at the library, every
test asserts on its expected values alone that they hold such values: a change of c or of the patterns that loses them fails loudly.

R is overlap_inputs.overlap_reads(320) -- ragged lengths 0 .. 40, empty reads, exact duplicates, a tandem repeat, a homopolymer --
with six symbols set to 5, followed by 1 000 copies of one read W of 40 symbols whose 5-mers are all distinct.  The copies are there
for one condition: a unitig's occurrences are at most the k-mer windows of the collection, so one unitig can only pass 2^32 when
it holds most windows of an index of no more than 3 GiB of records: W's 35 6-mers do, as one unitig."""
import functools

import numpy as np
import pytest

import scaled_inputs as si
from approx_inputs import cut_patterns
from approx_inputs import expected as approx_expected
from correct_inputs import correct, solid_count
from correct_inputs import table_of as correct_table
from edit_inputs import EditCollection, edited_patterns
from edit_inputs import expected as edit_expected
from kmer_inputs import brute
from kmer_join_inputs import brute_pair
from locate_inputs import locate_raw, ranges_raw, suffix_order
from mem_inputs import Brute, expected_mems, expected_stats, mems_raw, special_patterns, stats_raw, varied_patterns
from mem_inputs import same as mem_same
from overlap_inputs import expected as overlap_expected
from overlap_inputs import patterns_raw, prefix_table, rows_of, sequences_raw
from overlap_inputs import same as overlap_same
from test_gpu_find_approx import raw as approx_raw
from test_gpu_find_edit import GUARDS
from test_gpu_find_edit import raw as edit_raw
from test_gpu_sequences import extract_raw
from test_gpu_unitigs import absent_codes
from unitig_inputs import NONE, Graph
from unitig_inputs import table_of as unitig_table

pytestmark = pytest.mark.gpu

BASE_READS, W_COPIES = 320, 1000
# name -> (the edge, c of R, c of Q): n' = c n.  R has n = 46 560 positions, Q 6 097 (asserted in small()).
SIZES = {"super": (1 << 25, 1201, 8803), "wide": (1 << 32, 125003, 715003)}
KNOBS = ("approx_batch", "mem_batch", "locate_batch", "overlap_batch", "extract_batch", "correct_batch", "unitig_launch")
GUARD64 = GUARDS[0]
CORRECT_K, CORRECT_T, ROUNDS = 12, 2, 10
W_THRESHOLD = 500                          # only W's k-mers are that frequent in R


class Remembered(EditCollection):
    """The brute forces of tests/approx_inputs.py and tests/edit_inputs.py, each (pattern, budget) computed once: max_hits only cuts the result."""

    def __init__(self, rows):
        EditCollection.__init__(self, rows)
        self._hits, self._edit_hits = {}, {}

    def hits(self, pattern, d):
        key = (np.asarray(pattern, dtype=np.uint8).tobytes(), d)
        if key not in self._hits:
            self._hits[key] = EditCollection.hits(self, pattern, d)
        return self._hits[key]

    def edit_hits(self, pattern, e):
        key = (np.asarray(pattern, dtype=np.uint8).tobytes(), e)
        if key not in self._edit_hits:
            self._edit_hits[key] = EditCollection.edit_hits(self, pattern, e)
        return self._edit_hits[key]


class Small:
    """R and Q; what a brute force needs of R is made when a test first asks for it, once."""
    ids_offs = functools.cached_property(lambda s: suffix_order(s.reads, s.lengths))
    ids = property(lambda s: s.ids_offs[0])
    offs = property(lambda s: s.ids_offs[1])
    coll = functools.cached_property(lambda s: Remembered(s.arrays))
    brute = functools.cached_property(lambda s: Brute(s.rows))
    table = functools.cached_property(lambda s: prefix_table(s.rows))
    position_of = functools.cached_property(lambda s: {(int(j), int(o)): p for p, (j, o) in enumerate(zip(s.ids, s.offs))})      # (row, offset) -> BWT position of R


def distinct_read(seed, length, k):
    """A read of symbols 1..4 whose k-mers are all distinct."""
    rng = np.random.default_rng(seed)
    while True:
        w = rng.integers(1, 5, size=length).astype(np.uint8)
        if len({w[o: o + k].tobytes() for o in range(length - k + 1)}) == length - k + 1:
            return w


@functools.lru_cache(maxsize=None)
def small():
    """R and Q, computed once and not to be changed."""
    s = Small()
    reads, lengths, clean = si.small_collection(BASE_READS, 7)
    w = distinct_read(70, 40, 5)
    s.reads = np.concatenate([reads, np.tile(w, (W_COPIES, 1))])
    s.lengths = np.concatenate([lengths, np.full(W_COPIES, 40, dtype=lengths.dtype)])
    s.rows = rows_of(s.reads, s.lengths)
    s.clean_rows = rows_of(np.concatenate([clean, np.tile(w, (W_COPIES, 1))]), s.lengths)
    s.arrays = [np.array(r, dtype=np.uint8) for r in s.rows]
    s.w = tuple(int(v) for v in w)
    s.m, s.n = len(s.rows), sum(len(r) + 1 for r in s.rows)
    text = np.concatenate([np.array(r + (0,), dtype=np.uint8) for r in s.rows])
    s.C = np.concatenate([[0], np.cumsum(np.bincount(text, minlength=6))]).astype(np.int64)          # C[s] = symbols below s; C[6] = n
    other, other_lengths, _ = si.small_collection(200, 8, n_at=((5, 2), (47, 30)))
    s.q_rows = s.rows[100:250] + rows_of(other, other_lengths)                                      # shares k-mers with R, at other counts
    s.q_n = sum(len(r) + 1 for r in s.q_rows)
    assert (s.m, s.n, len(s.q_rows), s.q_n) == (1320, 46560, 350, 6097), (s.m, s.n, len(s.q_rows), s.q_n)
    assert sum(5 in r for r in s.rows) == 6 and sum(len(r) == 0 for r in s.rows) == 40 and s.rows[24:32] == s.rows[16:24]
    return s


def suffix_at(s, position):
    """(row, offset) of the suffix at one BWT position of R: the order of locate_inputs.suffix_order by one np.lexsort over the suffixes padded
    with endmarkers, equal ones by row (test_locator_and_positions holds it to suffix_order itself, which takes a third of a second)."""
    lengths = s.lengths.astype(np.int64)
    seq = np.repeat(np.arange(s.m), lengths + 1)
    off = np.arange(seq.size) - np.repeat(np.cumsum(lengths + 1) - (lengths + 1), lengths + 1)
    at = off[:, None] + np.arange(s.reads.shape[1])[None, :]
    padded = np.where(at < lengths[seq][:, None], s.reads[seq[:, None], np.minimum(at, s.reads.shape[1] - 1)], 0)
    order = np.lexsort((seq,) + tuple(padded[:, j] for j in range(padded.shape[1] - 1, -1, -1)))
    return int(seq[order[position]]), int(off[order[position]])


def text_of(rows):
    return np.concatenate([np.array(tuple(r) + (0,), dtype=np.uint8) for r in rows])


class Plan:
    """One size, as far as the CPU knows it: the copy counts, the edge and where it falls in R."""

    def __init__(self, name):
        s = small()
        self.name = name
        self.edge, self.c, self.cq = SIZES[name]
        self.n, self.m, self.q_n = self.c * s.n, self.c * s.m, self.cq * s.q_n
        self.p0 = self.edge // self.c                                                                  # the position of R that holds the edge
        self.row0, self.off0 = suffix_at(s, self.p0)
        self.straddler = s.rows[self.row0][self.off0:]                                                 # the suffix there: its prefixes' ranges straddle the edge
        sizes_are_what_the_file_says(self)


class Big(Plan):
    """One size: R x c and Q x cq on the device."""

    def __init__(self, gpu, oracle, name):
        Plan.__init__(self, name)
        self.gpu, self.oracle, self.handles = gpu, oracle, []
        self._y = self._loc = self._km = None
        self.x = self.uploaded(oracle, small().rows, self.c)
        assert (self.x.bases, self.x.sequences) == (self.n, self.m)

    def uploaded(self, oracle, rows, c):
        sym = oracle.FMI.from_text(text_of(rows)).symbols.astype(np.uint64)
        f = oracle.FMI.from_runs(sym, np.full(sym.size, c, dtype=np.uint64))
        x = self.gpu.Index.upload(f.data, f.sequences, f.bases)
        self.handles.append(x)
        return x

    @property
    def y(self):
        if self._y is None:
            self._y = self.uploaded(self.oracle, small().q_rows, self.cq)
            assert self._y.bases == self.q_n
        return self._y

    @property
    def loc(self):
        if self._loc is None:
            self._loc = self.x.locator()
            self.handles.append(self._loc)
        return self._loc

    @property
    def km(self):
        """The k-mers of CORRECT_K symbols, of every count: the corrector's and the unitigs' handle."""
        if self._km is None:
            self._km = self.x.kmers(CORRECT_K)
            self.handles.append(self._km)
        return self._km

    def free(self):
        for h in reversed(self.handles):
            h.free()
        self.handles = []


def sizes_are_what_the_file_says(b):
    """The conditions on the sizes themselves, from the numbers alone."""
    s = small()
    if b.name == "super":
        assert (1 << 25) + (1 << 20) < b.n < (1 << 26) and (1 << 25) + (1 << 20) < b.q_n < (1 << 26)
    else:
        assert b.n > (1 << 32) + (1 << 25) and b.q_n > (1 << 32) + (1 << 25) and b.c != b.cq
        assert 64 * (b.n // 128) < 3 << 30                                                             # the records of an index: at most 3 GiB
    inside = [sym for sym in range(1, 5) if b.c * int(s.C[sym]) < b.edge < b.c * int(s.C[sym + 1])]
    assert len(inside) == 1, "the edge lies in the class of no symbol 1..4"
    b.edge_symbol = inside[0]
    assert len(b.straddler) >= 12 and b.straddler[0] == b.edge_symbol and 5 not in b.straddler and b.c * b.p0 < b.edge


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    bwtm.trim()
    held = bwtm.pool_stats()["held_bytes"]
    yield bwtm
    bwtm.trim()
    assert bwtm.pool_stats()["held_bytes"] == held, "device memory did not return to what it was"


@pytest.fixture(scope="module", params=list(SIZES))
def big(gpu, oracle, request):
    held = gpu.pool_stats()["held_bytes"]
    b = Big(gpu, oracle, request.param)
    yield b
    b.free()
    gpu.trim()
    assert gpu.pool_stats()["held_bytes"] == held, "device memory did not return to what it was"


@pytest.fixture(autouse=True)
def knobs_back_to_their_defaults(gpu):
    yield
    for k in KNOBS:
        gpu.tune(k, 0)


# -------------------------------------------------------------------------------------------------------------------------- conditions

def both_sides(edge, values, what):
    """The expected values hold a coordinate at or beyond the edge and one below it."""
    values = np.asarray(values, dtype=np.uint64)
    assert values.size and int(values.max()) >= edge and int(values.min()) < edge, what


def straddles(edge, sp, count, what):
    """At least one non-empty range [sp, sp + count - 1] begins below the edge and ends at or beyond it."""
    sp, count = np.asarray(sp, dtype=np.uint64), np.asarray(count, dtype=np.uint64)
    over = (count > 0) & (sp < np.uint64(edge)) & (sp + count - np.uint64(1) >= np.uint64(edge))
    assert over.any(), what
    return int(over.sum())


def search_patterns(b):
    """Patterns cut from R without and with substitutions, the empty pattern, the one-symbol pattern of the class that holds the edge and
    prefixes of the suffix that holds it."""
    s = small()
    cut = cut_patterns(s.arrays[:BASE_READS + 2], (1, 2, 3, 12, 31, 40), 2, 21, substitutions=0) + cut_patterns(s.arrays[:BASE_READS + 2], (2, 3, 12, 40, 41), 2, 22)
    special = [np.zeros(0, dtype=np.uint8), np.array([b.edge_symbol], dtype=np.uint8)]
    special += [np.array(b.straddler[:l], dtype=np.uint8) for l in (2, 3, 6, 12, len(b.straddler))]
    special += [np.array([1], dtype=np.uint8), np.array([4], dtype=np.uint8), next(a[:12] for a in s.arrays if a.size >= 12 and a[0] == 4)]   # below and beyond either edge
    return cut[:12] + special + cut[12:]


# -------------------------------------------------------------------------------------------------------------------------- find, approx, edit

def filled(raw, gpu, x, patterns, budget, max_hits, want):
    """The sizing call and the filling call of raw (test_gpu_find_approx.raw or test_gpu_find_edit.raw) with three guard slots behind the end."""
    total = int(want[0][-1])
    sized = raw(gpu, x, patterns, budget, max_hits, 0, total + 3)
    assert sized[0] == 0 and np.array_equal(sized[1], want[0])
    assert all(np.all(a == g) for a, g in zip(sized[2:], GUARDS)), "the sizing call wrote hits"
    got = raw(gpu, x, patterns, budget, max_hits, total, total + 3)
    assert got[0] == 0
    assert all(np.all(a[total:] == g) for a, g in zip(got[2:], GUARDS)), "slots behind hit_offsets[count] were written"
    return (got[1],) + tuple(a[:total] for a in got[2:])


def same(got, want, what):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, j, np.flatnonzero(g[: w.size] != w[: g.size])[:5])


def test_find_and_find_approx(gpu, big):
    s, b = small(), big
    patterns = search_patterns(b)
    wants = {(d, mh): si.approx_hits(approx_expected(s.coll, patterns, d, mh), b.c) for d in (0, 1, 2) for mh in (0, 1)}
    for key, want in wants.items():
        both_sides(b.edge, want[1], key)
        straddles(b.edge, want[1], want[2], key)
    exact = [s.coll.hits(p, 0) for p in patterns]
    ranges = [si.find_range(int(h[0][0]), int(h[0][0] + h[1][0]) - 1, b.c) if h[0].size else si.EMPTY for h in exact]
    assert ranges[12] == (0, b.n - 1) and sum(r == si.EMPTY for r in ranges) >= 3 and sum(sp < b.edge <= ep for sp, ep in ranges) >= 5
    empty = int(wants[1, 0][0][12])
    assert [int(wants[1, 0][j][empty]) for j in (1, 2, 3)] == [0, b.n, 0]
    sp, ep = b.x.find(patterns)
    for j, (wsp, wep) in enumerate(ranges):
        assert (int(sp[j]), int(ep[j])) == (wsp, wep) if wsp <= wep else int(sp[j]) > int(ep[j]), j
    for (d, mh), want in wants.items():
        same(filled(approx_raw, gpu, b.x, patterns, d, mh, want), want, (d, mh))
    gpu.tune("approx_batch", 7)
    try:
        same(filled(approx_raw, gpu, b.x, patterns, 1, 0, wants[1, 0]), wants[1, 0], "approx_batch = 7")
    finally:
        gpu.tune("approx_batch", 0)


def test_find_edit(gpu, big):
    s, b = small(), big
    patterns = search_patterns(b)[6:8] + search_patterns(b)[12:28] + edited_patterns(s.arrays[:BASE_READS + 2], (2, 12), 3, 23)     # few lengths: the brute force pays per length
    wants = {(e, mh): si.edit_hits(edit_expected(s.coll, patterns, e, mh), b.c) for e in (0, 1, 2) for mh in (0, 1)}
    for key, want in wants.items():
        both_sides(b.edge, want[1], key)
        straddles(b.edge, want[1], want[2], key)
    assert int(wants[2, 0][4].min()) == 0 and int(wants[2, 0][2].max()) == b.n                       # the empty string, everywhere
    for (e, mh), want in wants.items():
        same(filled(edit_raw, gpu, b.x, patterns, e, mh, want), want, (e, mh))
    gpu.tune("approx_batch", 7)
    try:
        same(filled(edit_raw, gpu, b.x, patterns, 1, 0, wants[1, 0]), wants[1, 0], "approx_batch = 7")
    finally:
        gpu.tune("approx_batch", 0)


# -------------------------------------------------------------------------------------------------------------------------- statistics, MEMs

def mem_patterns(b):
    s = small()
    return special_patterns(s.clean_rows, 5) + varied_patterns(s.rows[:BASE_READS + 2], 6)[::9] + [b.straddler, (1,) + b.straddler + (5,)]


def test_matching_statistics_and_mems(gpu, big):
    s, b = small(), big
    patterns = mem_patterns(b)
    want_stats = si.stats(expected_stats(s.brute, patterns), b.c)
    both_sides(b.edge, want_stats[1][want_stats[0] > 0], "statistics")
    straddles(b.edge, want_stats[1], want_stats[2], "statistics")
    want_mems = {l: si.mems(expected_mems(s.brute, patterns, l), b.c) for l in (1, 12)}
    for l, want in want_mems.items():
        both_sides(b.edge, want[3], l)
        straddles(b.edge, want[3], want[4], l)
    assert mem_same(stats_raw(gpu, b.x, patterns), want_stats)
    for l, want in want_mems.items():
        assert mem_same(mems_raw(gpu, b.x, patterns, l), want), l
    gpu.tune("mem_batch", 7)
    try:
        assert mem_same(mems_raw(gpu, b.x, patterns, 12), want_mems[12])
        assert gpu.mem_stats()["batches"] == -(-len(patterns) // 7)
        assert mem_same(stats_raw(gpu, b.x, patterns), want_stats)
    finally:
        gpu.tune("mem_batch", 0)


# -------------------------------------------------------------------------------------------------------------------------- locate

def test_locator_and_positions(gpu, big):
    s, b = small(), big
    rng = np.random.default_rng(31)
    p = rng.integers(0, s.n, 3000).astype(np.uint64)
    t = rng.integers(0, b.c, 3000).astype(np.uint64)
    t[:500], t[500:1000] = 0, b.c - 1
    near = np.arange(b.edge - 130, b.edge + 131, dtype=np.uint64)
    positions = np.concatenate([p * np.uint64(b.c) + t, near, np.array([0, b.m - 1, b.m, b.n - 1], dtype=np.uint64)])
    both_sides(b.edge, positions, "positions")
    want = si.locate(s.ids, s.offs, positions, b.c)
    assert (int(s.ids[b.p0]), int(s.offs[b.p0])) == (b.row0, b.off0)
    assert b.loc.nbytes == 8 * b.m
    got = locate_raw(gpu, b.loc, positions)
    same(got, want, "positions")


def test_locate_ranges(gpu, big):
    s, b = small(), big
    e, c = b.edge, b.c
    first, last = c * int(s.C[b.edge_symbol]), c * int(s.C[b.edge_symbol + 1]) - 1                     # the class that holds the edge
    sp = [e - 7, e, e - 1, e - 300, c * b.p0 - 2, 9, 7, first, 0, b.n - 3]
    ep = [e + 9, e, e - 1, e + 300, c * b.p0 + c + 1, 2, 7, last, b.n - 1, b.n - 1]
    assert sum(a < e <= z for a, z in zip(sp, ep)) >= 5
    sizes = si.range_sizes(sp, ep)
    assert int(sizes[-1]) >= e and int(sizes[-1]) > b.n                                                # a prefix sum beyond the edge
    hit_offsets = np.full(len(sp) + 1, GUARD64, dtype=np.uint64)
    spa, epa = np.array(sp, dtype=np.uint64), np.array(ep, dtype=np.uint64)
    p_u64 = gpu.capi.p_u64
    gpu.capi.check(gpu.capi.lib().bwtm_locate_ranges(b.loc.h, spa.ctypes.data_as(p_u64), epa.ctypes.data_as(p_u64), spa.size, 0, hit_offsets.ctypes.data_as(p_u64), None, None, 0))
    assert np.array_equal(hit_offsets, sizes)                                                          # max_hits = 0: sizes only
    for max_hits in (1, 5):
        want = si.locate_ranges(s.ids, s.offs, sp, ep, c, max_hits)
        assert int(want[0][-1]) == sum(min(max_hits, max(z - a + 1, 0)) for a, z in zip(sp, ep))
        same(ranges_raw(gpu, b.loc, sp, ep, max_hits), want, max_hits)
    small_sp, small_ep = sp[:7], ep[:7]                                                                # whole small ranges around the edge
    want = si.locate_ranges(s.ids, s.offs, small_sp, small_ep, c)
    assert int(want[0][-1]) == 17 + 1 + 1 + 601 + c + 4 + 0 + 1
    got = ranges_raw(gpu, b.loc, small_sp, small_ep)
    same(got, want, "whole ranges")
    for r in range(len(small_sp)):                                                                      # each position against the rule
        a, z = int(got[0][r]), int(got[0][r + 1])
        ids, offs = si.locate(s.ids, s.offs, np.arange(small_sp[r], small_sp[r] + z - a, dtype=np.uint64), c)
        assert np.array_equal(got[1][a:z], ids) and np.array_equal(got[2][a:z], offs), r


def test_locate_mems_and_patterns(gpu, big):
    """The two paths tied: the ranges of a search, located with max_hits, are the rule's hits of the scaled ranges."""
    s, b = small(), big
    patterns = mem_patterns(b)[-12:]
    mems = si.mems(expected_mems(s.brute, patterns, 12), b.c)
    both_sides(b.edge, mems[3], "MEMs")
    want = si.locate_ranges(s.ids, s.offs, mems[3], mems[3] + mems[4] - np.uint64(1), b.c, 3)
    got = b.loc.locate_mems(patterns, 12, max_hits=3)
    same(got[:5], mems, "mems")
    same(got[5:], want, "their occurrences")
    found = search_patterns(b)[:19]
    exact = [s.coll.hits(p, 0) for p in found]
    ranges = [si.find_range(int(h[0][0]), int(h[0][0] + h[1][0]) - 1, b.c) if h[0].size else si.EMPTY for h in exact]
    assert sum(sp < b.edge <= ep for sp, ep in ranges) >= 5
    want = si.locate_ranges(s.ids, s.offs, [r[0] for r in ranges], [r[1] for r in ranges], b.c, 3)
    same(b.loc.locate_patterns(found, max_hits=3), want, "patterns")


# -------------------------------------------------------------------------------------------------------------------------- sequences

def edge_ids(b, rows_picked):
    """Ids at both ends of the id space and around the first copy of some rows: c j - 1, c j and c j + 1."""
    ids = [0, 1, b.c - 1, b.c, b.c + 1, b.m - 2, b.m - 1]
    for j in rows_picked:
        ids += [b.c * j - 1, b.c * j, b.c * j + 1]
    return ids


def walked(b, ids):
    """The BWT positions of R x c that hold a suffix of the sequences `ids`: what a walk over them reads, by the locate rule turned round."""
    s = small()
    return np.array([b.c * s.position_of[si.sequence_row(i, b.c), o] + i % b.c for i in ids for o in range(len(s.rows[si.sequence_row(i, b.c)]) + 1)], dtype=np.uint64)


def test_sequences_extract(gpu, big):
    s, b = small(), big
    picked = [1, 3, 5, 8, 13, 16, 24, 37, 47, 48, 200, BASE_READS - 1, BASE_READS, s.m - 1]          # reads with N, empty ones, duplicates, the first W
    ids = edge_ids(b, picked)
    assert max(ids) == b.m - 1
    for wanted in (ids, range(b.c * 47 - 3, b.c * 47 + 4), range(b.m - 5, b.m)):
        both_sides(b.edge, walked(b, wanted), "the positions the walks read")
    for got, wanted in ((extract_raw(gpu, b.x, ids=np.array(ids, dtype=np.uint64)), ids),
                        (extract_raw(gpu, b.x, first=b.c * 47 - 3, count=7), range(b.c * 47 - 3, b.c * 47 + 4)),
                        (extract_raw(gpu, b.x, first=b.m - 5, count=5), range(b.m - 5, b.m))):
        rows = [s.rows[si.sequence_row(i, b.c)] for i in wanted]
        assert got[0].tolist() == [0] + list(np.cumsum([len(r) for r in rows]))
        assert got[1].tolist() == [v for r in rows for v in r]
    assert s.rows[46] != s.rows[47] and len(s.rows[48]) == 0


# -------------------------------------------------------------------------------------------------------------------------- overlaps

def sizes_only(gpu, call, count):
    hit_offsets = np.full(count + 1, GUARD64, dtype=np.uint64)
    gpu.capi.check(call(hit_offsets.ctypes.data_as(gpu.capi.p_u64), None, None, 0))
    return hit_offsets


def test_overlaps(gpu, big):
    s, b = small(), big
    w_ids = [b.c * (BASE_READS + 20 * j) + j for j in range(40)]                                       # copies of W: c 000 hits each, so that the sizes pass the edge
    seq_ids = edge_ids(b, [1, 3, 16, 17, 24, 25, 47, 200, BASE_READS, s.m - 1]) + [b.c * j + j for j in range(40, 160)] + w_ids
    by_id = si.overlap_queries(s.rows, seq_ids, b.c)
    as_patterns = [s.rows[j] for j in range(0, BASE_READS + 2, 2)] + [s.w[5:] + (2, 2), s.w[20:]] + [s.w] * 40
    bases = {tau: (overlap_expected(s.table, by_id, tau), overlap_expected(s.table, as_patterns, tau)) for tau in (1, 12)}
    for tau, pair in bases.items():
        for base in pair:                                                                              # the sizing call without max_hits: every count times c
            sizes = si.overlap_offsets(base, b.c)
            assert int(sizes[-1]) >= b.edge and int(sizes[1:].min()) < b.edge, tau
    lib, p_u64, p_u8 = gpu.capi.lib(), gpu.capi.p_u64, gpu.capi.p_u8
    ida = np.array(seq_ids, dtype=np.uint64)
    offsets = np.zeros(len(as_patterns) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(p) for p in as_patterns])
    text = np.ascontiguousarray(np.concatenate([np.array(p, dtype=np.uint8) for p in as_patterns]))
    for tau, (base_ids, base_patterns) in bases.items():
        got = sizes_only(gpu, lambda ho, oi, ol, cap: lib.bwtm_overlap_sequences(b.loc.h, ida.ctypes.data_as(p_u64), 0, ida.size, tau, 0, ho, oi, ol, cap), ida.size)
        assert np.array_equal(got, si.overlap_offsets(base_ids, b.c)), tau
        got = sizes_only(gpu, lambda ho, oi, ol, cap: lib.bwtm_overlap_batch(b.loc.h, text.ctypes.data_as(p_u8), offsets.ctypes.data_as(p_u64), len(as_patterns), tau, 0, ho, oi, ol, cap),
                         len(as_patterns))
        assert np.array_equal(got, si.overlap_offsets(base_patterns, b.c)), tau
        for max_hits in (1, 5):
            want_ids, want_patterns = si.overlaps(base_ids, b.c, max_hits), si.overlaps(base_patterns, b.c, max_hits)
            assert overlap_same(sequences_raw(gpu, b.loc, tau, ids=ida, max_hits=max_hits), want_ids), (tau, max_hits)
            assert overlap_same(patterns_raw(gpu, b.loc, tau, as_patterns, max_hits=max_hits), want_patterns), (tau, max_hits)
    want_ids, want_patterns = si.overlaps(bases[12][0], b.c, 5), si.overlaps(bases[12][1], b.c, 5)
    gpu.tune("overlap_batch", 64); gpu.tune("locate_batch", 64)
    try:
        assert len(seq_ids) > 128 and len(as_patterns) > 128
        assert overlap_same(sequences_raw(gpu, b.loc, 12, ids=ida, max_hits=5), want_ids)
        assert overlap_same(patterns_raw(gpu, b.loc, 12, as_patterns, max_hits=5), want_patterns)
    finally:
        gpu.tune("overlap_batch", 0); gpu.tune("locate_batch", 0)


# -------------------------------------------------------------------------------------------------------------------------- k-mers

@functools.lru_cache(maxsize=None)
def small_kmers(k):
    return brute(small().arrays, k, 5, 1)


@pytest.mark.parametrize("k", [1, 6, 12, 21])
def test_kmers(gpu, big, k):
    s, b = small(), big
    base = small_kmers(k)
    wants = {min_count: si.kmers(base, b.c, min_count) for min_count in (1, 2 * b.c, 2 * b.c + 1)}
    for min_count, want in wants.items():
        both_sides(b.edge, want[2], (k, min_count))
        if k <= 6:
            straddles(b.edge, want[2], want[1], (k, min_count))
            assert si.kmer_total(want, 1) >= b.edge                                                    # a large sum
    for min_count, want in wants.items():
        km = b.km if (k, min_count) == (CORRECT_K, 1) else b.x.kmers(k, min_count=min_count)
        try:
            assert km.distinct == want[0].size
            same(km.download(), want, (k, min_count))
            assert km.total == si.kmer_total(want, 1) == int(want[1].sum())
            assert np.array_equal(km.levels(), si.kmer_levels(s.arrays, k, 5, b.c, min_count, brute=lambda rows, k, skip, least: small_kmers(k))), (k, min_count)
            kept = (want[1] // np.uint64(b.c)).astype(np.int64)
            for bins in (2, 3 * b.c, 3 * b.c + 1, 4096):
                assert np.array_equal(km.histogram(bins), si.histogram(np.bincount(kept), b.c, bins)), (k, min_count, bins)
        finally:
            if km is not b._km:
                km.free()
    assert k == 1 or want[0].size < base[0].size and int(base[1].min()) == 1                                   # the last threshold drops the k-mers of count 1 and 2


# -------------------------------------------------------------------------------------------------------------------------- k-mer join

@functools.lru_cache(maxsize=None)
def small_pair(k, swapped):
    s = small()
    return brute_pair(s.q_rows if swapped else s.rows, s.rows if swapped else s.q_rows, k, 5)


@pytest.mark.parametrize("k", [6, 12])
def test_kmer_join(gpu, big, k):
    s, b = small(), big
    cases = []
    for swapped in (False, True):
        ca, cb = (b.cq, b.c) if swapped else (b.c, b.cq)
        for bounds in ({}, {"max_a": 0}) if not swapped else ({}, {"min_a": 2 * ca, "min_sum": 2 * ca + cb + 1}):
            want = si.join(small_pair(k, swapped), ca, cb, **bounds)
            both_sides(b.edge, want[3], "sp_a")
            both_sides(b.edge, want[4], "sp_b")
            if bounds == {"max_a": 0}:
                assert want[0].size > 20 and not want[1].any() and int(want[3].max()) >= b.edge         # absent from a: insertion points alone
            cases.append((swapped, ca, cb, bounds, want))
    for swapped, ca, cb, bounds, want in cases:
        xa, xb = (b.y, b.x) if swapped else (b.x, b.y)
        rows_a, rows_b = (s.q_rows, s.rows) if swapped else (s.rows, s.q_rows)                      # what small_pair(k, swapped) is the brute force of
        j = xa.kmer_join(xb, k, **bounds)
        try:
            assert j.distinct == want[0].size
            same(j.download(), want, (k, swapped, bounds))
            assert list(j.summary().values()) == si.join_summary(want)
            assert np.array_equal(j.levels(), si.join_levels(rows_a, rows_b, k, 5, ca, cb, brute_pair=lambda a, b, k, skip: small_pair(k, swapped), **bounds)), (k, swapped, bounds)
        finally:
            j.free()


# -------------------------------------------------------------------------------------------------------------------------- corrector, unitigs

@functools.lru_cache(maxsize=None)
def small_table():
    return correct_table(small().arrays, CORRECT_K)


def test_corrector_at_the_threshold_edges(gpu, big):
    s, b = small(), big
    table, t = small_table(), CORRECT_T
    ids = edge_ids(b, [3, 5, 13, 15, 23, 37, 46, 47, 55, 63, 71, 200, 263, BASE_READS])
    picks = [si.sequence_row(i, b.c) for i in ids]
    got_rows = [correct(s.arrays[j], table, CORRECT_K, t, ROUNDS) for j in picks]
    want_text = [g[0] for g in got_rows]
    want_status, want_edits = np.array([g[1] for g in got_rows], dtype=np.uint8), np.array([g[2] for g in got_rows], dtype=np.uint32)
    assert len(set(want_status.tolist())) >= 3 and solid_count(table, t) < solid_count(table, t - 1)
    both_sides(b.edge, walked(b, ids), "the positions the walks read")
    both_sides(b.edge, walked(b, range(b.c * 47 - 3, b.c * 47 + 4)), "the positions the window's walks read")
    thresholds = (b.c * t, b.c * t - 1, b.c * (t - 1) + 1)
    assert all(si.small_threshold(T, b.c) == t for T in thresholds) and si.small_threshold(b.c * (t - 1), b.c) == t - 1
    for n, T in enumerate(thresholds):
        cor = b.km.corrector(T)
        try:
            assert (cor.solid, cor.k) == (solid_count(table, t), CORRECT_K)
            if n == 2:
                gpu.tune("correct_batch", 7)
            offsets, text, status, edits = cor.correct_sequences(b.x, ids=np.array(ids, dtype=np.uint64), max_rounds=ROUNDS)
            assert [bytes(bytearray(text[int(offsets[j]): int(offsets[j + 1])].tolist())) for j in range(len(ids))] == want_text
            assert np.array_equal(status, want_status) and np.array_equal(edits, want_edits)
            _, none, status, edits = cor.correct_sequences(b.x, ids=np.array(ids, dtype=np.uint64), max_rounds=ROUNDS, text=False)
            assert none is None and np.array_equal(status, want_status) and np.array_equal(edits, want_edits)
            first = b.c * 47 - 3
            window = cor.correct_sequences(b.x, first=first, count=7, max_rounds=ROUNDS, text=False)
            assert window[2].tolist() == [correct(s.arrays[si.sequence_row(i, b.c)], table, CORRECT_K, t, ROUNDS)[1] for i in range(first, first + 7)]
        finally:
            gpu.tune("correct_batch", 0)
            cor.free()
    below = b.km.corrector(b.c * (t - 1))
    try:
        assert below.solid == solid_count(table, t - 1)
    finally:
        below.free()


def same_graph(u, g, c):
    """What test_gpu_unitigs.same checks, with the occurrences multiplied by c."""
    assert (u.count, u.nodes, u.symbols, u.k) == (g.U, g.S, g.symbols, g.k)
    got, want = u.download(), si.unitig_arrays(g.arrays(), c)
    for name, a, w in zip(("offsets", "text", "nodes", "occurrences", "flags", "links"), got, want):
        assert a.dtype == w.dtype and np.array_equal(a.ravel(), w), (name, np.flatnonzero(a.ravel()[: w.size] != w[: a.size])[:10])
    codes = np.concatenate([np.array(g.nodes, dtype=np.uint64), absent_codes(g)])
    pu, po = u.place(codes)
    wu, wo = g.place(codes)
    assert np.array_equal(pu, wu) and np.array_equal(po, wo)
    assert (pu[g.S:] == NONE).all() and (po[g.S:] == NONE).all()
    return want


def test_unitigs(gpu, big):
    s, b = small(), big
    t = CORRECT_T
    g = Graph(unitig_table(s.arrays, CORRECT_K), CORRECT_K, t)
    assert g.U > 10 and g.S == solid_count(small_table(), t)
    for T in (b.c * t, b.c * (t - 1) + 1):                                                              # from the corrector's handle
        u = b.km.unitigs(T)
        try:
            same_graph(u, g, b.c)
        finally:
            u.free()
    km = b.x.kmers(6)
    try:
        for t6 in (W_THRESHOLD, 3):
            g6 = Graph(unitig_table(s.arrays, 6), 6, t6)
            occurrences = si.unitig_arrays(g6.arrays(), b.c)[3]
            if t6 == W_THRESHOLD:
                assert g6.U == 1 and g6.S == 35 and int(occurrences[0]) >= b.edge                      # W alone: one unitig of most windows
            else:
                assert g6.U > 50 and int(occurrences.min()) < b.edge                                         # a branching graph, W's path cut by the genome's
            u = km.unitigs(b.c * t6)
            try:
                same_graph(u, g6, b.c)
            finally:
                u.free()
    finally:
        km.free()
