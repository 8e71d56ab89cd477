"""The expected values of tests/test_gpu_walks.py (tests/walk_inputs.py), without a GPU: the suffix array and the LF model against the
oracle's BWT of the long collection, the prefix-function overlaps against the all-pairs comparison, and the scrambled streams held to
the properties the GPU cases rely on.  Every position a model walk visits is below n and every table index below m; the kernels make
exactly these loads, so the GPU cases provoke no out-of-range access by construction."""
import time

import numpy as np
import pytest

import walk_inputs as wi
from overlap_inputs import all_pairs_hits, overlap_reads, rows_of
from test_gpu_sequences import text_of


@pytest.fixture(scope="module")
def long_case(oracle):
    t0 = time.process_time()
    rows, text = wi.long_collection(wi.LONG_SEED)
    sa, ids, offs, bwt = wi.suffix_array(text)
    print("suffix_array of %d positions: %.2f s of CPU time" % (text.size, time.process_time() - t0))
    return rows, text, sa, ids, offs, bwt


def test_long_collection_is_what_the_issue_states(long_case):
    rows, text, sa, ids, offs, bwt = long_case
    assert tuple(len(r) for r in rows) == wi.LONG_LENGTHS == (0, 65535, 3, 65536, 1, 65537, 129, 128, 127, 40)
    assert text.size == sum(wi.LONG_LENGTHS) + 10 == 197046 and int((text == 0).sum()) == 10
    assert all(r.size == 0 or (r.min() >= 1 and r.max() <= 5) for r in rows)
    assert np.array_equal(rows[3][-4000:], rows[5][:4000]) and np.array_equal(rows[1][-129:], rows[6])
    again, _ = wi.long_collection(wi.LONG_SEED)
    assert all(np.array_equal(a, b) for a, b in zip(rows, again))


def test_suffix_array_spells_the_oracles_bwt(oracle, long_case):
    rows, text, sa, ids, offs, bwt = long_case
    n = text.size
    assert np.array_equal(np.sort(sa), np.arange(n))
    assert np.array_equal(bwt, np.asarray(oracle.FMI.from_text(text).symbols))
    assert np.array_equal(ids[:10], np.arange(10)) and offs[:10].tolist() == list(wi.LONG_LENGTHS)      # position p < m: (p, length of p)
    got = set(zip(ids.tolist(), offs.tolist()))
    assert len(got) == n and all((j, o) in got for j in range(10) for o in (0, len(rows[j])))
    # neighbours in the order are ascending as strings up to the first endmarker (a sample; the oracle's BWT above pins all of it)
    for p in np.random.default_rng(1).integers(1, n, size=200).tolist():
        a, b = int(sa[p - 1]), int(sa[p])
        k = 0
        while text[a + k] == text[b + k] and text[a + k] != 0:
            k += 1
        assert (text[a + k], ids[p - 1]) < (text[b + k], ids[p]), p


def test_lf_model_gives_back_the_rows_and_the_suffix_arrays_pairs(long_case):
    rows, text, sa, ids, offs, bwt = long_case
    t0 = time.process_time()
    M = wi.lf_model(bwt)
    print("lf_model of %d positions: %.2f s of CPU time" % (bwt.size, time.process_time() - t0))
    assert M.m == 10 and M.n == text.size and M.cycle.size == 0
    assert M.lengths.tolist() == list(wi.LONG_LENGTHS)
    assert all(np.array_equal(M.sequences[j], rows[j]) for j in range(10))
    assert sorted(M.table.tolist()) == list(range(10))
    assert np.array_equal(M.ids, ids.astype(np.int64)) and np.array_equal(M.offs, offs.astype(np.int64))
    assert 0 <= M.visited_max < M.n and 0 <= M.table_max < M.m
    assert M.fails(range(10), 65536) == 5 and M.fails(range(10), 65537) is None and M.fails([9, 3, 5, 1], 65535) == 1
    assert M.fails([0, 1, 2, 4, 6, 7, 8, 9], 65535) is None and M.fails([0, 1, 2, 4, 6, 7, 8, 9], 65534) == 1


def test_borders_agree_with_the_all_pairs_comparison():
    """Every read of the 300-read overlap input as a query, thresholds 1 and 5: the same hits in the same order."""
    reads, lengths = overlap_reads(300, 1)
    rows = rows_of(reads, lengths)
    t0 = time.process_time()
    total = 0
    for q in range(300):
        want = all_pairs_hits(rows, rows[q], 1)
        got = wi.border_hits(rows, rows[q], 1)
        assert got == want, q
        assert wi.border_hits(rows, rows[q], 5) == [h for h in want if h[1] >= 5] == all_pairs_hits(rows, rows[q], 5), q
        total += len(want)
    print("300 x 300 pairs, %d hits: %.2f s of CPU time" % (total, time.process_time() - t0))
    assert total > 5000
    assert wi.borders((1, 2, 1, 2, 1), (3, 1, 2, 1, 2, 1)) == [5, 3, 1] and wi.borders((), (1, 2)) == [] and wi.borders((1, 2), ()) == []
    assert wi.borders((1, 2, 3), (1, 2, 3)) == [3] and wi.borders((2, 2, 2, 2), (2, 2)) == [2, 1]


def test_long_overlaps_by_borders(long_case):
    """The expected hits of the long queries: the planted overlaps are there, longest first, and the helpers stay within their time."""
    rows = long_case[0]
    t0 = time.process_time()
    per_query = [wi.border_hits(rows, rows[q], 1) for q in range(10)]
    spent = time.process_time() - t0
    print("borders of all ten queries against all ten targets: %.2f s of CPU time" % spent)
    assert per_query[3][:2] == [(3, 65536), (5, 4000)] and per_query[1][:2] == [(1, 65535), (6, 129)]
    assert per_query[5][0] == (5, 65537) and per_query[6][0] == (6, 129) and per_query[0] == []
    assert [h for h in per_query[3] if h[1] >= 100] == [(3, 65536), (5, 4000)]
    assert [h for h in per_query[1] if h[1] >= 100] == [(1, 65535), (6, 129)]
    for q in range(10):
        for t, l in per_query[q]:
            assert np.array_equal(rows[t][:l], rows[q][len(rows[q]) - l:]), (q, t, l)
        assert [l for _, l in per_query[q]] == sorted((l for _, l in per_query[q]), reverse=True)
    ho, ids, lens = wi.hits_arrays(per_query, max_hits=1)
    assert ho.tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9] and ids.tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert spent < 20


def test_overlap_model_on_a_real_bwt(oracle):
    """On a BWT the model of the backward search is the all-pairs comparison, order and cut included."""
    reads, lengths = overlap_reads(300, 1)
    rows = rows_of(reads, lengths)
    bwt = np.asarray(oracle.FMI.from_text(text_of(reads, lengths)).symbols)
    M = wi.lf_model(bwt)
    assert M.cycle.size == 0 and all(tuple(M.sequences[j].tolist()) == rows[j] for j in range(300))
    for q in range(0, 300, 7):
        for tau, max_hits in ((1, 0), (5, 0), (5, 2)):
            want = all_pairs_hits(rows, rows[q], tau)
            assert wi.overlap_model(bwt, M.table, rows[q], tau, max_hits) == (want[:max_hits] if max_hits else want), (q, tau, max_hits)


@pytest.mark.parametrize("name", sorted(wi.SCRAMBLED))
def test_scrambled_streams_have_the_properties_the_gpu_cases_need(name):
    S = wi.SCRAMBLED[name]
    n, m = S["n"], S["m"]
    symbols = wi.scrambled_stream(S["seed"], n, m)
    assert symbols.size == n and int((symbols == 0).sum()) == m and symbols.max() == 5
    assert np.array_equal(symbols, wi.scrambled_stream(S["seed"], n, m))
    M = wi.lf_model(symbols)                                               # asserts that all m walks end, each at a zero of its own
    cyc = M.cycle
    thirds = [int(((cyc >= a * n // 3) & (cyc < (a + 1) * n // 3)).sum()) for a in range(3)]
    print("%s: longest walk %d (sequence %d), median %.1f, %d cycle positions %s, the first at %d" % (name, M.lengths.max(), M.lengths.argmax(),
          float(np.median(M.lengths)), cyc.size, thirds, cyc[0]))
    assert M.m == m and sorted(M.table.tolist()) == list(range(m))
    assert int(M.lengths.max()) == S["longest"] and int(M.lengths.argmax()) == S["longest_id"]
    assert int((M.lengths == M.lengths.max()).sum()) == 1                  # the refusal at max_len - 1 names one id
    assert cyc.size == S["cycle"] >= 8 and int(cyc[0]) == S["first_cycle"] and min(thirds) >= 1
    assert int(M.lengths.sum()) + m + cyc.size == n                        # every position is on exactly one walk or on a cycle
    assert M.fails(range(m), S["longest"]) is None and M.fails(range(m), S["longest"] - 1) == S["longest_id"]
    # what the kernels load: positions below n, table entries below m -- on the walks and on the cycles up to the largest bound in use
    assert 0 <= M.visited_max < n and 0 <= M.table_max < m
    assert all(wi.cycle_walk_stays_inside(M, int(p), S["longest"] + 1) for p in cyc)
    assert np.all(M.lf[symbols > 0] >= m) and np.all(M.lf < n)
    assert wi.cycle_walk_stays_inside(M, int(cyc[0]), 65538)
    for p in cyc[:8].tolist():                                             # a cycle position returns to itself
        q, steps = int(M.lf[p]), 1
        while q != p:
            q = int(M.lf[q]); steps += 1
            assert steps <= cyc.size
    # the sequences of the model spell their own walks
    j = S["longest_id"]
    p = j
    for c in M.sequences[j][::-1].tolist():
        assert symbols[p] == c
        p = int(M.lf[p])
    assert symbols[p] == 0 and p == M.ends[j] and M.pair(j) == (j, S["longest"]) and M.pair(int(cyc[0])) is None
    # the overlap model's own loads (it asserts e1 <= n and z1 <= m at every step)
    for seq in M.sequences[:20]:
        wi.overlap_model(symbols, M.table, seq, 1, 0)
