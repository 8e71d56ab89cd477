"""The rules of tests/scaled_inputs.py without a GPU: R x c is built explicitly as rows, every brute force the GPU tests use is run on it, and
the result is compared with the scaled result of the same brute force on R -- at c = 3, and once at c = 1, where every rule must be the
identity.  A wrong rule is caught here, not on the GPU, where tests/test_gpu_beyond_32_bits.py relies on them at the copy counts of its SIZES."""
import numpy as np
import pytest

import scaled_inputs as si
from approx_inputs import Collection, cut_patterns
from approx_inputs import expected as approx_expected
from correct_inputs import correct_all, solid_count
from correct_inputs import table_of as correct_table
from edit_inputs import EditCollection, edited_patterns
from edit_inputs import expected as edit_expected
from kmer_inputs import brute, brute_levels, folded_histogram, text_of
from kmer_join_inputs import brute_pair, brute_pair_levels, classes
from locate_inputs import suffix_order
from mem_inputs import Brute, expected_mems, expected_stats, special_patterns, varied_patterns
from overlap_inputs import expected as overlap_expected
from overlap_inputs import prefix_table, rows_of
from unitig_inputs import Graph
from unitig_inputs import table_of as unitig_table

READS = 200
COPIES = [3, 1]


class Small:
    pass


@pytest.fixture(scope="module")
def small():
    s = Small()
    s.reads, s.lengths, clean = si.small_collection(READS, 3)
    s.rows = rows_of(s.reads, s.lengths)
    s.clean_rows = rows_of(clean, s.lengths)
    q_reads, q_lengths, _ = si.small_collection(READS - 40, 4)
    s.q_rows = rows_of(q_reads, q_lengths)
    assert sum(5 in r for r in s.rows) == 6 and any(len(r) == 0 for r in s.rows) and s.rows[24:32] == s.rows[16:24]
    return s


def same(got, want):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), j


def patterns_of(rows):
    cut = cut_patterns(rows, (1, 2, 3, 12, 31, 40, 41), 3, 11, substitutions=0) + cut_patterns(rows, (0, 1, 2, 3, 12, 31, 40), 3, 12)
    return cut + cut_patterns(rows, (12,), 3, 13, substitutions=2)


@pytest.mark.parametrize("c", COPIES)
def test_from_runs_is_the_index_of_the_expanded_text(oracle, small, c):
    f = oracle.FMI.from_text(text_of(small.rows))
    sym = f.symbols
    runs = oracle.FMI.from_runs(sym.astype(np.uint64), np.full(sym.size, c, dtype=np.uint64))
    whole = oracle.FMI.from_text(text_of(si.expand(small.rows, c)))
    assert np.array_equal(runs.symbols, whole.symbols) and np.array_equal(runs.symbols, np.repeat(sym, c))
    assert np.array_equal(runs.C, whole.C) and np.array_equal(runs.C, f.C * np.uint64(c))
    assert (runs.sequences, runs.bases) == (whole.sequences, whole.bases) == (c * f.sequences, c * f.bases)
    rng = np.random.default_rng(1)
    for p in rng.integers(0, whole.bases + 1, 300).tolist() + [0, whole.bases]:
        for s in range(6):
            assert si.rank(sym, p, s, c) == whole.rank(p, s), (p, s)
    for p in patterns_of(small.rows) + [np.zeros(0, dtype=np.uint8)]:
        sp, ep = f.find(p)
        wsp, wep = whole.find(p)
        assert si.find_range(sp, ep, c) == ((wsp, wep) if wsp <= wep else si.EMPTY)
    assert si.find_range(0, f.bases - 1, c) == (0, whole.bases - 1)


@pytest.mark.parametrize("c", COPIES)
def test_approx_and_edit_hits(small, c):
    patterns = patterns_of(small.rows)
    one, many = Collection(small.rows), Collection(si.expand(small.rows, c))
    hits = 0
    for d in (0, 1, 2):
        for max_hits in (0, 1):
            want = approx_expected(many, patterns, d, max_hits)
            same(si.approx_hits(approx_expected(one, patterns, d, max_hits), c), want)
            hits += int(want[0][-1])
    assert hits > 6 * len(patterns)
    empty = si.approx_hits(approx_expected(one, [np.zeros(0, dtype=np.uint8)], 1), c)
    assert (int(empty[1][0]), int(empty[2][0]), int(empty[3][0])) == (0, many.n, 0) and many.n == c * one.n
    patterns = patterns[::3] + edited_patterns(small.rows, (0, 1, 2, 12, 31), 2, 14)
    one, many = EditCollection(small.rows), EditCollection(si.expand(small.rows, c))
    for e in (0, 1, 2):
        for max_hits in (0, 1):
            want = edit_expected(many, patterns, e, max_hits)
            same(si.edit_hits(edit_expected(one, patterns, e, max_hits), c), want)
    assert int(want[4].min()) == 0 and int(want[0][-1]) > 0


@pytest.mark.parametrize("c", COPIES)
def test_statistics_and_mems(small, c):
    patterns = special_patterns(small.clean_rows, 5) + varied_patterns(small.rows, 6)[::5]
    one, many = Brute(small.rows), Brute(si.expand(small.rows, c))
    same(si.stats(expected_stats(one, patterns), c), expected_stats(many, patterns))
    for min_length in (1, 12):
        want = expected_mems(many, patterns, min_length)
        same(si.mems(expected_mems(one, patterns, min_length), c), want)
        assert int(want[0][-1]) > 20


@pytest.mark.parametrize("c", COPIES)
def test_locate_and_sequences(small, c):
    ids, offs = suffix_order(small.reads, small.lengths)
    big_reads, big_lengths = si.expand_reads(small.reads, small.lengths, c)
    want_ids, want_offs = suffix_order(big_reads, big_lengths)
    n = want_ids.size
    assert n == c * ids.size
    same(si.locate(ids, offs, np.arange(n), c), (want_ids, want_offs))
    sp = [0, 5, c * 40 + 1, n - 4, 7, 9]
    ep = [n - 1, 5, c * 43, n - 1, 6, 2]
    for max_hits in (0, 1, 5):
        ho, gi, go = si.locate_ranges(ids, offs, sp, ep, c, max_hits)
        assert np.array_equal(ho, si.range_sizes(sp, ep, max_hits))
        for r, (s, e) in enumerate(zip(sp, ep)):
            k = max(e - s + 1, 0) if max_hits == 0 else min(max(e - s + 1, 0), max_hits)
            a = int(ho[r])
            assert int(ho[r + 1]) - a == k and np.array_equal(gi[a: a + k], want_ids[s: s + k]) and np.array_equal(go[a: a + k], want_offs[s: s + k])
    big_rows = rows_of(big_reads, big_lengths)
    assert all(big_rows[i] == small.rows[si.sequence_row(i, c)] for i in range(len(big_rows))) and big_rows == si.expand(small.rows, c)


@pytest.mark.parametrize("c", COPIES)
def test_overlaps(small, c):
    big_rows = si.expand(small.rows, c)
    table, big_table = prefix_table(small.rows), prefix_table(big_rows)
    seq_ids = [0, 1, c - 1, c, c * 17 + 1, c * 24, c * 25 - 1, len(big_rows) - 1] + list(range(c * 40, c * 60, 7))
    for queries, big_queries in ((small.rows, small.rows), (si.overlap_queries(small.rows, seq_ids, c), [big_rows[i] for i in seq_ids])):
        assert list(queries) == list(big_queries)
        for tau in (1, 12):
            base = overlap_expected(table, queries, tau)
            for max_hits in (0, 1, 5):
                want = overlap_expected(big_table, big_queries, tau, max_hits)
                same(si.overlaps(base, c, max_hits), want)
                assert np.array_equal(si.overlap_offsets(base, c, max_hits), want[0])
            assert int(base[0][-1]) > len(queries) // 2


@pytest.mark.parametrize("c", COPIES)
def test_kmers(small, c):
    big_rows = si.expand(small.rows, c)
    for k, min_count in ((1, 1), (6, 1), (6, 2 * c), (6, 2 * c + 1), (12, c + 1), (21, 0)):
        base = brute(small.rows, k, 5, 1)
        want = brute(big_rows, k, 5, min_count)
        got = si.kmers(base, c, min_count)
        same(got, want)
        assert np.array_equal(si.kmer_levels(small.rows, k, 5, c, min_count), brute_levels(big_rows, k, 5, min_count))
        assert si.kmer_total(si.kmers(base, 1, si.small_threshold(min_count, c)), c) == int(want[1].sum())
        kept = si.kmers(base, 1, si.small_threshold(min_count, c))[1]
        for bins in (2, 3 * c, 3 * c + 1, 4096):
            assert np.array_equal(si.histogram(np.bincount(kept.astype(np.int64)), c, bins), folded_histogram(want[1], bins)), (k, bins)
    assert want[0].size > 100


@pytest.mark.parametrize("ca,cb", [(3, 2), (1, 1)])
def test_kmer_join(small, ca, cb):
    big_a, big_b = si.expand(small.rows, ca), si.expand(small.q_rows, cb)
    for rows_a, rows_b, xa, xb, ya, yb in ((small.rows, small.q_rows, big_a, big_b, ca, cb), (small.q_rows, small.rows, big_b, big_a, cb, ca)):
        for k in (6, 12):
            base = brute_pair(rows_a, rows_b, k, 5)
            for bounds in ({}, {"max_a": 0}, {"min_a": 2 * ya, "max_b": 3 * yb}, {"min_sum": 2 * ya + yb + 1}, {"min_b": yb + 1, "max_a": 2 * ya - 1}):
                want = brute_pair(xa, xb, k, 5, **bounds)
                got = si.join(base, ya, yb, **bounds)
                same(got, want)
                assert si.join_summary(got) == classes(want)
                assert np.array_equal(si.join_levels(rows_a, rows_b, k, 5, ya, yb, **bounds), brute_pair_levels(xa, xb, k, 5, **bounds)), (k, bounds)
            assert want[0].size > 0
    absent = brute_pair(big_a, big_b, 12, 5, max_a=0)
    assert absent[0].size > 50 and not absent[1].any() and absent[3].any()                 # insertion points of absent k-mers are scaled too


@pytest.mark.parametrize("c", COPIES)
def test_corrector_and_unitigs(small, c):
    big_rows = si.expand(small.rows, c)
    k, t = 8, 2
    table, big_table = correct_table(small.rows, k), correct_table(big_rows, k)
    thresholds = [c * t, c * t - 1, c * (t - 1) + 1] if c > 1 else [t]
    assert all(si.small_threshold(T, c) == t for T in thresholds)
    assert si.small_threshold(c * t + 1, c) == t + 1 and si.small_threshold(c * (t - 1), c) == max(t - 1, 1)
    want = correct_all(small.rows, k, t, 10, table=table)
    assert {0, 1, 2, 3} == set(want[1].tolist())
    for T in thresholds:
        assert solid_count(big_table, T) == solid_count(table, t) < solid_count(table, t - 1)
        texts, status, edits = correct_all(big_rows, k, T, 10, table=big_table)
        picks = [si.sequence_row(i, c) for i in range(len(big_rows))]
        assert texts == [want[0][j] for j in picks] and np.array_equal(status, want[1][picks]) and np.array_equal(edits, want[2][picks])
    for k in (6, 12):
        g = Graph(unitig_table(small.rows, k), k, t)
        for T in thresholds:
            big = Graph(unitig_table(big_rows, k), k, T)
            same(si.unitig_arrays(g.arrays(), c), big.arrays())
            assert big.nodes == g.nodes and big.members == g.members and big.where == g.where
        assert g.U > 10
