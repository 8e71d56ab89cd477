"""The LF-walk kernels (k_seq_lengths, k_seq_emit, k_locate_build, k_locate, k_overlap_scan, k_overlap_expand) on the two kinds of input
the read-like cases never give them: sequences around the default bound of 2^16 symbols, and streams with consistent counts that are the
BWT of nothing, where the m walks from the endmarker suffixes still end and every other position lies on a cycle that must be refused.
Expected values come from the rows, a suffix array, the prefix function and a numpy LF model (tests/walk_inputs.py, pinned without a
GPU in tests/test_walk_inputs_host.py), never from the library.  No existing test covers one of the tiny collections exactly (the
smallest sequences / locate / overlap inputs elsewhere hold 300 reads), so all four are here."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import walk_inputs as wi
from locate_inputs import FILL, locate_raw, pairs, ranges_raw, suffix_order
from overlap_inputs import all_pairs_hits, patterns_raw, rows_of, same, sequences_raw
from test_gpu_sequences import extract_raw, uploaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
EINVAL = 1
LONG = (1, 3, 5)                                   # the sequences of 65 535, 65 536 and 65 537 symbols

_cases = {}


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    yield bwtm
    for case in _cases.values():
        for h in case.handles:
            h.free()
    _cases.clear()


class Case:
    pass


def long_case(gpu, oracle):
    """The long collection, uploaded once: rows, the suffix array's (ids, offsets) per BWT position, the position of every suffix."""
    if "long" not in _cases:
        c = Case()
        c.rows, text = wi.long_collection(wi.LONG_SEED)
        sa, c.ids, c.offs, bwt = wi.suffix_array(text)
        c.n = text.size
        inv = np.empty(c.n, dtype=np.int64)
        inv[sa] = np.arange(c.n)
        starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in c.rows])[:-1]])
        c.position_of = lambda j, o: int(inv[int(starts[j]) + o])
        f = oracle.FMI.from_text(text)
        assert f.sequences == 10 and f.bases == c.n
        c.x = gpu.Index.upload(f.data, f.sequences, f.bases)
        c.handles = [c.x]
        c.loc = None
        _cases["long"] = c
    return _cases["long"]


def long_locator(gpu, oracle):
    c = long_case(gpu, oracle)
    if c.loc is None:
        c.loc = c.x.locator(max_len=65537)
        c.handles.insert(0, c.loc)
    return c.loc


def scrambled_case(gpu, oracle, name):
    """A scrambled stream, uploaded once from the oracle's encoding of its symbols, with the LF model and a locator at the longest walk."""
    if name not in _cases:
        S = wi.SCRAMBLED[name]
        c = Case()
        c.S = S
        c.symbols = wi.scrambled_stream(S["seed"], S["n"], S["m"])
        c.M = wi.lf_model(c.symbols)
        f = oracle.FMI.from_symbols(c.symbols)
        assert f.sequences == S["m"] and f.bases == S["n"]
        c.x = gpu.Index.upload(f.data, f.sequences, f.bases)
        assert np.array_equal(c.x.C.astype(np.int64), c.M.C)
        c.loc = c.x.locator(max_len=S["longest"])                           # exactly the longest walk's symbols pass
        c.good = np.nonzero(c.M.ids >= 0)[0]
        c.handles = [c.loc, c.x]
        _cases[name] = c
    return _cases[name]


def refused(gpu, call, pattern):
    with pytest.raises(gpu.BwtmError) as e:
        call()
    assert re.search(pattern, str(e.value)), str(e.value)


# ---------------------------------------------------------------------------- long sequences

@pytest.mark.parametrize("batch", [0, 4])
def test_long_sequences_around_the_default_bound(gpu, oracle, batch):
    """max_len = 0 is the default bound 2^16: the sequence of 65 537 symbols is refused by name, the one of 65 536 passes.  Every refusal
    names the first offender in list order.  With extract_batch = 4 the three long sequences fall into batches 0, 0 and 1, the refused one
    is number 1 of the second batch, and the first batch's text has already reached the caller while the failed batch's has not."""
    c = long_case(gpu, oracle)
    x, rows = c.x, c.rows
    lib, p_u64, p_u8 = gpu.capi.lib(), gpu.capi.p_u64, gpu.capi.p_u8
    without_5 = [0, 1, 2, 3, 4, 6, 7, 8, 9]
    gpu.tune("extract_batch", batch)
    try:
        refused(gpu, lambda: x.sequences(first=0, count=10), r"sequence 5 is longer than max_len = 65536 ")
        got = extract_raw(gpu, x, ids=without_5)
        want = wi.expected_text(rows, without_5)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        offsets, text = extract_raw(gpu, x, first=0, count=10, max_len=65537)            # also: the bytes behind the end keep 0xEE
        want = wi.expected_text(rows, range(10))
        assert np.array_equal(offsets, want[0])
        for k in range(10):
            assert np.array_equal(text[int(offsets[k]): int(offsets[k + 1])], rows[k]), k
        assert np.array_equal(text, want[1])
        refused(gpu, lambda: x.sequences(first=0, count=10, max_len=65536), r"sequence 5 is longer than max_len = 65536 ")
        refused(gpu, lambda: x.sequences(ids=np.array([9, 3, 5, 1]), max_len=65535), r"sequence 3 is longer than max_len = 65535 ")
        got = extract_raw(gpu, x, ids=[9, 1], max_len=65535)                             # exactly max_len symbols pass
        assert np.array_equal(got[1], np.concatenate([rows[9], rows[1]]))
        # the extracting call without a sizing call before it: what the failed batch and the later ones would have written stays untouched
        offsets = np.full(11, FILL, dtype=np.uint64)
        text = np.full(int(want[0][-1]) + 64, 0xEE, dtype=np.uint8)
        rc = lib.bwtm_sequences_extract(x.h, None, 0, 10, 65536, offsets.ctypes.data_as(p_u64), text.ctypes.data_as(p_u8), text.size)
        assert rc == EINVAL and b"sequence 5 is longer than max_len = 65536 " in lib.bwtm_last_error()
        reached = int(want[0][4]) if batch == 4 else 0                                   # sequences 0..3: the batch before the failed one
        assert np.array_equal(text[:reached], want[1][:reached]) and np.all(text[reached:] == 0xEE)
        got = extract_raw(gpu, x, ids=[5], max_len=65537)                                # the index still answers
        assert np.array_equal(got[1], rows[5])
    finally:
        gpu.tune("extract_batch", 0)


def test_long_locate(gpu, oracle):
    """A locator is refused at the default bound and builds at 65 537.  The endmarker suffixes, both ends of every long sequence (walks of 0,
    1, len - 1 and len steps from offsets 0, 1, len - 1 and len), 4 096 random positions and 64 ranges of 32 positions across record edges
    locate to the suffix array's (id, offset), as positions and as ranges alike; a pattern cut from the planted stretch is found in both
    sequences that hold it."""
    c = long_case(gpu, oracle)
    x, rows, n = c.x, c.rows, c.n
    refused(gpu, lambda: x.locator(), r"sequence 5 is longer than max_len = 65536 ")
    refused(gpu, lambda: x.locator(max_len=65536), r"sequence 5 is longer than max_len = 65536 ")
    loc = long_locator(gpu, oracle)
    assert loc.nbytes == 80
    ends = [c.position_of(j, o) for j in LONG for o in (0, 1, len(rows[j]) - 1, len(rows[j]))]
    assert [c.position_of(j, len(rows[j])) for j in range(10)] == list(range(10))
    rng = np.random.default_rng(21)
    positions = np.concatenate([np.arange(10), ends, rng.integers(0, n, size=4096)]).astype(np.uint64)
    t0 = time.perf_counter()
    ids, offs = locate_raw(gpu, loc, positions)
    print("bwtm_locate_batch of %d positions of the long collection: %.3f s" % (positions.size, time.perf_counter() - t0))
    assert np.array_equal(ids, c.ids[positions]) and np.array_equal(offs, c.offs[positions])
    assert ids[:10].tolist() == list(range(10)) and offs[:10].tolist() == list(wi.LONG_LENGTHS)
    assert pairs(ids[10:22], offs[10:22]) == [(j, o) for j in LONG for o in (0, 1, len(rows[j]) - 1, len(rows[j]))]
    hit_offsets, rids, roffs = ranges_raw(gpu, loc, positions, positions)                # every position as a range of its own
    assert np.array_equal(hit_offsets, np.arange(positions.size + 1)) and np.array_equal(rids, ids) and np.array_equal(roffs, offs)
    edges = 128 * rng.choice(np.arange(1, n // 128), size=64, replace=False)
    sp = (edges - 16).astype(np.uint64)
    inside = (sp[:, None] + np.arange(32, dtype=np.uint64)[None, :]).reshape(-1)
    hit_offsets, rids, roffs = ranges_raw(gpu, loc, sp, sp + np.uint64(31))
    assert np.array_equal(hit_offsets, 32 * np.arange(65)) and np.array_equal(rids, c.ids[inside]) and np.array_equal(roffs, c.offs[inside])
    ids, offs = locate_raw(gpu, loc, inside)
    assert np.array_equal(ids, rids) and np.array_equal(offs, roffs)
    pattern = rows[5][100:160]
    want = sorted((j, o) for j in range(10) if len(rows[j]) >= 60
                  for o in np.nonzero(np.all(np.lib.stride_tricks.sliding_window_view(rows[j], 60) == pattern[None, :], axis=1))[0].tolist())
    assert want == [(3, 65536 - 4000 + 100), (5, 100)]
    hit_offsets, ids, offs = loc.locate_patterns([pattern])
    assert hit_offsets.tolist() == [0, 2] and sorted(pairs(ids, offs)) == want


def test_long_overlaps(gpu, oracle):
    """Searches of 65 535 to 65 537 symbols: the three long sequences and sequence 6 as queries, then all ten, thresholds 1 and 100, equal
    to the borders over all targets.  Query 3 finds (5, 4000) and query 1 finds (6, 129) behind the query itself, which overlaps itself
    over its whole length and so comes first; the planted tails as patterns of their own have no such hit, and max_hits = 1 keeps exactly the
    planted overlap."""
    c = long_case(gpu, oracle)
    rows = c.rows
    loc = long_locator(gpu, oracle)
    t0 = time.process_time()
    per_query = [wi.border_hits(rows, rows[q], 1) for q in range(10)]
    print("borders of ten queries against ten targets: %.2f s of CPU time" % (time.process_time() - t0))
    for tau in (1, 100):
        kept = [[h for h in hits if h[1] >= tau] for hits in per_query]
        for max_hits in (0, 1):                                                           # max_hits = 1: every query keeps itself alone
            got = sequences_raw(gpu, loc, tau, ids=[1, 3, 5, 6], max_hits=max_hits)
            assert same(got, wi.hits_arrays([kept[q] for q in (1, 3, 5, 6)], max_hits)), (tau, max_hits)
        got = sequences_raw(gpu, loc, tau, first=0, count=10)
        assert same(got, wi.hits_arrays(kept))
        mine = lambda q: pairs(got[1][int(got[0][q]): int(got[0][q + 1])], got[2][int(got[0][q]): int(got[0][q + 1])])
        assert mine(3)[:2] == [(3, 65536), (5, 4000)] and mine(1)[:2] == [(1, 65535), (6, 129)] and mine(5)[0] == (5, 65537) and mine(0) == []
        if tau == 1:
            assert same(patterns_raw(gpu, loc, tau, [rows[q] for q in (1, 3, 5, 6)]), wi.hits_arrays([kept[q] for q in (1, 3, 5, 6)]))
        tails = [rows[3][-5000:], rows[1][-200:]]
        want = [[h for h in wi.border_hits(rows, t, tau)] for t in tails]
        assert want[0][0] == (5, 4000) and want[1][0] == (6, 129)
        assert same(patterns_raw(gpu, loc, tau, tails), wi.hits_arrays(want))
        cut = patterns_raw(gpu, loc, tau, tails, max_hits=1)
        assert cut[0].tolist() == [0, 1, 2] and pairs(cut[1], cut[2]) == [(5, 4000), (6, 129)]


# ---------------------------------------------------------------------------- tiny collections

def tiny_rows(name):
    one = tuple(np.random.default_rng(31).integers(1, 6, size=300).tolist())
    return {"one sequence of 300": [one], "one empty sequence": [()], "two, one of them empty": [(), one[:17]], "three empty sequences": [(), (), ()]}[name]


@pytest.mark.parametrize("name", ["one sequence of 300", "one empty sequence", "two, one of them empty", "three empty sequences"])
def test_tiny_collections(gpu, oracle, name):
    rows = tiny_rows(name)
    m, n = len(rows), sum(len(r) for r in rows) + len(rows)
    lengths = np.array([len(r) for r in rows], dtype=np.uint32)
    reads = np.zeros((m, max(1, int(lengths.max()))), dtype=np.uint8)
    for j, r in enumerate(rows):
        reads[j, : len(r)] = r
    x = uploaded(gpu, oracle, reads, lengths)
    assert x.bases == n and x.sequences == m
    offsets, text = extract_raw(gpu, x, first=0, count=m)
    want = wi.expected_text(rows, range(m))
    assert np.array_equal(offsets, want[0]) and np.array_equal(text, want[1])
    loc = x.locator()
    assert loc.nbytes == 8 * m
    want_ids, want_offs = suffix_order(reads, lengths)
    ids, offs = locate_raw(gpu, loc, np.arange(n))
    assert np.array_equal(ids, want_ids) and np.array_equal(offs, want_offs)
    hit_offsets, rids, roffs = ranges_raw(gpu, loc, [0], [n - 1])
    assert hit_offsets.tolist() == [0, n] and np.array_equal(rids, want_ids) and np.array_equal(roffs, want_offs)
    assert rows_of(reads, lengths) == [tuple(r) for r in rows]
    for tau in (1, 17):
        want = wi.hits_arrays([all_pairs_hits(rows, rows[q], tau) for q in range(m)])
        assert same(sequences_raw(gpu, loc, tau, first=0, count=m), want), tau
        assert same(patterns_raw(gpu, loc, tau, rows), want), tau
    loc.free()
    x.free()


# ---------------------------------------------------------------------------- streams that are no BWT

def maximal_ranges(good):
    """The maximal runs of consecutive positions in the ascending array `good`, as closed ranges (sp, ep)."""
    cuts = np.nonzero(np.diff(good) != 1)[0]
    return np.concatenate([[good[0]], good[cuts + 1]]).astype(np.uint64), np.concatenate([good[cuts], [good[-1]]]).astype(np.uint64)


@pytest.mark.parametrize("name", ["small", "large"])
def test_scrambled_sequences_and_locations(gpu, oracle, name):
    """The m walks from the endmarker suffixes end on any stream with consistent counts: sequences, the locator's build and every position
    on one of the walks are those of the LF model.  One symbol less than the unique longest walk and k_seq_lengths / k_locate_build refuse
    that id."""
    c = scrambled_case(gpu, oracle, name)
    x, M, S, m = c.x, c.M, c.S, c.S["m"]
    want = wi.expected_text(M.sequences, range(m))
    for max_len in (S["longest"], 0):
        offsets, text = extract_raw(gpu, x, first=0, count=m, max_len=max_len)
        assert np.array_equal(offsets, want[0]) and np.array_equal(text, want[1])
    message = r"sequence %d is longer than max_len = %d " % (S["longest_id"], S["longest"] - 1)
    refused(gpu, lambda: x.sequences(first=0, count=m, max_len=S["longest"] - 1), message)
    refused(gpu, lambda: x.locator(max_len=S["longest"] - 1), message)
    ids, offs = locate_raw(gpu, c.loc, c.good)
    assert np.array_equal(ids.astype(np.int64), M.ids[c.good]) and np.array_equal(offs.astype(np.int64), M.offs[c.good])
    assert np.array_equal(ids[:m], np.arange(m)) and np.array_equal(offs[:m].astype(np.int64), M.lengths)
    sp, ep = maximal_ranges(c.good)
    assert sp.size >= 8 and int((ep - sp + np.uint64(1)).sum()) == c.good.size
    hit_offsets, rids, roffs = ranges_raw(gpu, c.loc, sp, ep)
    assert int(hit_offsets[-1]) == c.good.size and np.array_equal(rids, ids) and np.array_equal(roffs, offs)


def check_still_answers(c):
    probe = c.good[:: max(1, c.good.size // 50)]
    ids, offs = c.loc.locate(probe)
    assert np.array_equal(ids.astype(np.int64), c.M.ids[probe]) and np.array_equal(offs.astype(np.int64), c.M.offs[probe])


@pytest.mark.parametrize("name", ["small", "large"])
def test_scrambled_refusals(gpu, oracle, name):
    """A position on a pure cycle never meets an endmarker: locate_walk gives up at d == max_len, k_locate names the slot, and the API
    names the position (bwtm_locate_batch) or the hit (bwtm_locate_ranges).  With locate_batch = 64 the batches before the failed one have
    reached the caller, the failed batch and the later ones have not, and the name is the first failure of the first failed batch."""
    c = scrambled_case(gpu, oracle, name)
    M, n = c.M, c.S["n"]
    lib, p_u64 = gpu.capi.lib(), gpu.capi.p_u64
    cyc = M.cycle
    rng = np.random.default_rng(41)
    positions = rng.choice(c.good, size=400, replace=False).astype(np.uint64)
    positions[200] = cyc[cyc.size // 2]                 # the first cycle position of the list, in batch 3 (slots 192 .. 255)
    positions[230] = cyc[0]                             # the same batch, a smaller position behind it
    positions[300] = cyc[-1]                            # a later batch
    gpu.tune("locate_batch", 64)
    try:
        ids = np.full(400, FILL, dtype=np.uint64); offs = np.full(400, FILL, dtype=np.uint64)
        rc = lib.bwtm_locate_batch(c.loc.h, positions.ctypes.data_as(p_u64), 400, ids.ctypes.data_as(p_u64), offs.ctypes.data_as(p_u64))
        assert rc == EINVAL
        assert ("bwtm_locate_batch: position %d reaches no start of a sequence" % int(positions[200])) in lib.bwtm_last_error().decode()
        assert np.array_equal(ids[:192].astype(np.int64), M.ids[positions[:192]]) and np.array_equal(offs[:192].astype(np.int64), M.offs[positions[:192]])
        assert np.all(ids[192:] == FILL) and np.all(offs[192:] == FILL)
        check_still_answers(c)
        sp = np.zeros(1, dtype=np.uint64); ep = np.full(1, n - 1, dtype=np.uint64)
        hit_offsets = np.full(2, FILL, dtype=np.uint64)
        gpu.capi.check(lib.bwtm_locate_ranges(c.loc.h, sp.ctypes.data_as(p_u64), ep.ctypes.data_as(p_u64), 1, 0, hit_offsets.ctypes.data_as(p_u64), None, None, 0))
        assert hit_offsets.tolist() == [0, n]
        ids = np.full(n, FILL, dtype=np.uint64); offs = np.full(n, FILL, dtype=np.uint64)
        rc = lib.bwtm_locate_ranges(c.loc.h, sp.ctypes.data_as(p_u64), ep.ctypes.data_as(p_u64), 1, 0, hit_offsets.ctypes.data_as(p_u64), ids.ctypes.data_as(p_u64),
                                    offs.ctypes.data_as(p_u64), n)
        assert rc == EINVAL
        assert ("bwtm_locate_ranges: hit %d reaches no start of a sequence" % int(cyc[0])) in lib.bwtm_last_error().decode()
        reached = 64 * (int(cyc[0]) // 64)
        assert reached >= 64 and np.array_equal(ids[:reached].astype(np.int64), M.ids[:reached]) and np.array_equal(offs[:reached].astype(np.int64), M.offs[:reached])
        assert np.all(ids[reached:] == FILL) and np.all(offs[reached:] == FILL)
        check_still_answers(c)
    finally:
        gpu.tune("locate_batch", 0)
    # the default batch: one launch, the smallest failing slot of the whole list
    refused(gpu, lambda: c.loc.locate(positions), r"position %d reaches no start" % int(positions[200]))
    refused(gpu, lambda: c.loc.locate_ranges([0], [n - 1]), r"hit %d reaches no start" % int(cyc[0]))
    first = int(cyc[3]) - 2                              # an empty range, then five positions around a cycle position: the first of them on a cycle
    refused(gpu, lambda: c.loc.locate_ranges([5, first], [4, first + 4]), r"hit %d reaches no start" % next(k for k in range(5) if M.ids[first + k] < 0))
    check_still_answers(c)


def test_a_walk_that_never_ends_stops_at_the_bound(gpu, oracle):
    """A locator of max_len = 65 537 on the small stream: the walk from a cycle position takes all 65 537 steps before k_locate gives up."""
    c = scrambled_case(gpu, oracle, "small")
    loc = c.x.locator(max_len=65537)
    try:
        p = int(c.M.cycle[0])
        t0 = time.perf_counter()
        refused(gpu, lambda: loc.locate(np.array([3, p, 4])), r"position %d reaches no start" % p)
        print("a refused walk of 65 537 steps: %.3f s" % (time.perf_counter() - t0))
        ids, offs = loc.locate(c.good)
        assert np.array_equal(ids.astype(np.int64), c.M.ids[c.good]) and np.array_equal(offs.astype(np.int64), c.M.offs[c.good])
    finally:
        loc.free()


@pytest.mark.parametrize("name", ["small", "large"])
def test_scrambled_overlaps(gpu, oracle, name):
    """The backward search on a stream that is no BWT against its numpy model: the model's own sequences and 50 random patterns."""
    c = scrambled_case(gpu, oracle, name)
    M, m = c.M, c.S["m"]
    rng = np.random.default_rng(51)
    queries = list(M.sequences) + [rng.integers(1, 6, size=int(rng.integers(1, 13))).astype(np.uint8) for _ in range(50)]
    for tau in (1, 5):
        for max_hits in (0, 2):
            want = wi.hits_arrays([wi.overlap_model(c.symbols, M.table, q, tau, max_hits) for q in queries])
            assert int(want[0][-1]) >= 50
            assert same(patterns_raw(gpu, c.loc, tau, queries, max_hits=max_hits), want), (tau, max_hits)
            assert same(c.loc.overlap_patterns(queries, tau, max_hits), want)                # the binding's own wrapper
            by_id = sequences_raw(gpu, c.loc, tau, first=0, count=m, max_hits=max_hits)
            assert np.array_equal(by_id[0], want[0][: m + 1]) and np.array_equal(by_id[1], want[1][: int(want[0][m])]) and np.array_equal(by_id[2], want[2][: int(want[0][m])])


def test_on_a_poisoned_pool(bwtm):
    """The long-sequence extraction and the scrambled refusals in a fresh process whose pool hands out blocks filled with 0xA5A5A5A5:
    every length, byte of text, table entry and output that is read was written by the kernels, and a refused batch leaves nothing behind."""
    env = dict(os.environ, BWTM_POOL_POISON="0xA5A5A5A5")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "walks_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), "exit status %s\n%s%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
    assert got and int(got.group(1)) > 0 and int(got.group(2)) >= 256 * int(got.group(1)), out.stdout[-3000:]
