"""Suffix-prefix overlaps on the GPU (bwtm_overlap_sequences, bwtm_overlap_batch, Locator.overlaps, Locator.overlap_patterns).
Expected values are always computed from the reads the test itself made -- a string comparison of the rows (tests/overlap_inputs.py,
checked against the oracle in tests/test_overlap_host.py) -- never the library's own search or extraction."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from locate_inputs import FILL
from overlap_inputs import WIDTH, expected, overlap_reads, patterns_raw, prefix_table, rows_of, same, sequences_raw, table_hits
from test_gpu_sequences import text_of, uploaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TAU = 5


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    return bwtm


def collection(gpu, oracle, m, seed):
    """(index, locator, rows, prefix table) of the overlap input; no read is longer than the locator's max_len = 40."""
    reads, lengths = overlap_reads(m, seed)
    x = uploaded(gpu, oracle, reads, lengths)
    rows = rows_of(reads, lengths)
    return x, x.locator(max_len=WIDTH), rows, prefix_table(rows)


@pytest.fixture(scope="module")
def three_hundred(gpu, oracle):
    x, loc, rows, table = collection(gpu, oracle, 300, 1)
    yield x, loc, rows, table
    loc.free()
    x.free()


@pytest.fixture(scope="module")
def thousand(gpu, oracle):
    x, loc, rows, table = collection(gpu, oracle, 1000, 2)
    yield x, loc, rows, table
    loc.free()
    x.free()


def test_all_reads_as_queries(gpu, oracle):
    """The 300 reads, every one a query: by id range, as patterns, and by a shuffled id list with repeats -- exactly the all-pairs hits,
    order included.  Empty reads have no hits and are nobody's target."""
    x, loc, rows, table = collection(gpu, oracle, 300, 1)
    want = expected(table, rows, TAU)
    assert int(want[0][-1]) > 2000
    got = sequences_raw(gpu, loc, TAU, first=0, count=300)
    assert same(got, want)
    assert same(patterns_raw(gpu, loc, TAU, rows), want)
    ids = np.random.default_rng(3).permutation(300)
    ids = np.concatenate([ids, ids[:40], [7, 7, 7]])
    assert same(sequences_raw(gpu, loc, TAU, ids=ids), expected(table, [rows[int(j)] for j in ids], TAU))
    per_query = np.diff(got[0].astype(np.int64))
    assert all(per_query[q] == 0 for q in range(300) if len(rows[q]) < TAU) and any(len(r) == 0 for r in rows)
    assert got[2].min() >= TAU and all(len(rows[int(t)]) >= int(l) for t, l in zip(got[1], got[2]))
    # the binding's own wrappers, and the self hit filtered on the host
    assert same(loc.overlaps(min_overlap=TAU), want) and same(loc.overlap_patterns(rows, TAU), want)
    assert same(loc.overlaps(first=100, count=50, min_overlap=TAU), expected(table, rows[100:150], TAU))
    skipped = loc.overlaps(min_overlap=TAU, skip_self=True)
    keep = [[(t, l) for t, l in table_hits(table, rows[q], TAU) if not (t == q and l == len(rows[q]))] for q in range(300)]
    assert skipped[0].tolist() == [0] + list(np.cumsum([len(k) for k in keep]))
    assert list(zip(skipped[1].tolist(), skipped[2].tolist())) == [h for k in keep for h in k]
    assert sum(1 for q in range(300) for t, l in keep[q] if t == q) >= 1                     # a periodic read still overlaps itself
    loc.free()
    x.free()


@pytest.mark.parametrize("tau", [1, 12, 40, 41])
def test_thresholds(gpu, three_hundred, tau):
    x, loc, rows, table = three_hundred
    want = expected(table, rows, tau)
    got = sequences_raw(gpu, loc, tau, first=0, count=300)
    assert same(got, want)
    if tau == 41:
        assert got[1].size == 0 and not got[0].any()
    if tau == 40:
        assert got[1].size >= 300 // 8 and np.all(got[2] == 40) and all(len(rows[int(t)]) == 40 for t in got[1])
    if tau == 1:
        assert got[2].min() == 1


def test_counts_per_length_equal_find_with_an_endmarker(gpu, thousand):
    """The existing backward search on (0,) + suffix counts the reads that start with the suffix: per query and per length, as many hits."""
    x, loc, rows, table = thousand
    queries = [q for q in np.random.default_rng(4).permutation(1000).tolist() if len(rows[q]) > 0][:50]
    hit_offsets, ids, lengths = sequences_raw(gpu, loc, 1, ids=queries)
    patterns, owner = [], []
    for k, q in enumerate(queries):
        for l in range(1, len(rows[q]) + 1):
            patterns.append(np.array((0,) + rows[q][len(rows[q]) - l:], dtype=np.uint8)); owner.append((k, l))
    sp, ep = x.find(patterns)
    for (k, l), s, e in zip(owner, sp.tolist(), ep.tolist()):
        mine = lengths[int(hit_offsets[k]): int(hit_offsets[k + 1])]
        assert int(np.sum(mine == l)) == (e - s + 1 if s <= e else 0), (queries[k], l)


def test_patterns_that_are_not_reads(gpu, three_hundred):
    x, loc, rows, table = three_hundred
    into_repeat = (4, 3, 3, 4) + (1, 2) * 7                                # its suffix runs into the tandem repeat
    absent = (1, 2, 1, 2, 3, 3, 5, 5)                                      # the reads hold no 5: no suffix of it starts a read
    long_one = tuple(np.random.default_rng(5).integers(1, 5, size=60).tolist()) + next(r for r in rows if len(r) == 40)
    patterns = [into_repeat, absent, long_one, (3,), (), long_one[:77]]
    for tau in (1, 2):
        want = expected(table, patterns, tau)
        assert same(patterns_raw(gpu, loc, tau, patterns), want)
    want = expected(table, patterns, 2)
    per = np.diff(want[0].astype(np.int64)).tolist()
    assert per[0] >= 10 and per[1] == 0 and per[2] >= 1 and per[3] == 0 and per[4] == 0
    assert int(want[2][int(want[0][2])]) == 40 and len(long_one) == 100 > WIDTH      # the 40-symbol read at the long pattern's end
    one = expected(table, [(3,)], 1)
    assert same(patterns_raw(gpu, loc, 1, [(3,)]), one) and one[1].size >= 10 and np.all(one[2] == 1)


@pytest.mark.parametrize("max_hits", [1, 2, 1 << 20])
def test_max_hits_keeps_the_longest(gpu, three_hundred, max_hits):
    x, loc, rows, table = three_hundred
    full = sequences_raw(gpu, loc, TAU, first=0, count=300)
    cut = sequences_raw(gpu, loc, TAU, first=0, count=300, max_hits=max_hits)
    assert same(cut, expected(table, rows, TAU, max_hits))
    assert max(np.diff(full[0].astype(np.int64)).tolist()) > 2                               # the small limits do cut
    for q in range(300):
        a, b = int(cut[0][q]), int(cut[0][q + 1])
        fa, fb = int(full[0][q]), int(full[0][q + 1])
        assert b - a == min(fb - fa, max_hits)
        assert np.array_equal(cut[1][a:b], full[1][fa: fa + b - a]) and np.array_equal(cut[2][a:b], full[2][fa: fa + b - a]), q
    if max_hits == 1 << 20:
        assert same(cut, full)
    assert same(patterns_raw(gpu, loc, TAU, rows, max_hits=max_hits), cut)


@pytest.mark.parametrize("count", [1, 3, 4, 5, 63, 64, 65, 257])
def test_counts_that_leave_partial_quads_waves_and_blocks(gpu, thousand, count):
    x, loc, rows, table = thousand
    for first in (0, 1000 - count, 333):
        assert same(sequences_raw(gpu, loc, TAU, first=first, count=count), expected(table, rows[first: first + count], TAU)), first
    ids = np.random.default_rng(count).integers(0, 1000, size=count)
    want = expected(table, [rows[int(j)] for j in ids], TAU)
    assert same(sequences_raw(gpu, loc, TAU, ids=ids), want)
    assert same(patterns_raw(gpu, loc, TAU, [rows[int(j)] for j in ids]), want)


def test_batches_give_the_same_result(gpu, oracle):
    """overlap_batch = 64 and locate_batch = 64 on the 1 000 reads: sixteen query batches, every one counted twice, hundreds of hit
    batches, one query's hits across several of them and many queries inside one; equal to the default batch's results and to the rows."""
    x, loc, rows, table = collection(gpu, oracle, 1000, 2)
    want = expected(table, rows, TAU)
    per = np.diff(want[0].astype(np.int64))
    assert int(want[0][-1]) > 20000 and per.max() > 3 * 64 and np.sum((per >= 1) & (per <= 8)) > 64
    whole = sequences_raw(gpu, loc, TAU, first=0, count=1000)
    cut = sequences_raw(gpu, loc, TAU, first=0, count=1000, max_hits=70)
    gpu.tune("overlap_batch", 64)
    gpu.tune("locate_batch", 64)
    try:
        small = sequences_raw(gpu, loc, TAU, first=0, count=1000)
        small_patterns = patterns_raw(gpu, loc, TAU, rows)
        small_cut = sequences_raw(gpu, loc, TAU, first=0, count=1000, max_hits=70)
    finally:
        gpu.tune("overlap_batch", 0)
        gpu.tune("locate_batch", 0)
    assert same(whole, want) and same(small, want) and same(small_patterns, want)
    assert same(cut, expected(table, rows, TAU, 70)) and same(small_cut, cut)
    loc.free()
    x.free()


def test_the_two_rounds_of_a_call_of_many_batches(gpu, three_hundred):
    """overlap_batch = 64, so that bwtm_overlap_batch counts every batch twice: the sizing call, a capacity one short, the exact capacity;
    a batch of sixty-four queries shorter than min_overlap in the middle contributes nothing."""
    x, loc, rows, table = three_hundred
    lib, p_u64, p_u8 = gpu.capi.lib(), gpu.capi.p_u64, gpu.capi.p_u8
    short = [tuple(r[-(TAU - 1):]) for r in rows if len(r) >= TAU][:64]
    queries = rows[:64] + short + rows[64:164]
    want = expected(table, queries, TAU)
    per = np.diff(want[0].astype(np.int64))
    total = int(want[0][-1])
    assert len(short) == 64 and len(queries) == 228 and not per[64:128].any() and per[:64].sum() > 64 and per[128:].sum() > 100
    assert np.all(want[0][64:129] == want[0][64])                                 # flat across the second batch
    offsets = np.zeros(len(queries) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(q) for q in queries])
    text = np.ascontiguousarray(np.concatenate([np.asarray(q, dtype=np.uint8) for q in queries]))

    def call(capacity):
        hit_offsets = np.full(len(queries) + 1, FILL, dtype=np.uint64)
        ids, lens = np.full(total + 3, FILL, dtype=np.uint64), np.full(total + 3, FILL, dtype=np.uint64)
        rc = lib.bwtm_overlap_batch(loc.h, text.ctypes.data_as(p_u8), offsets.ctypes.data_as(p_u64), len(queries), TAU, 0, hit_offsets.ctypes.data_as(p_u64),
                                    ids.ctypes.data_as(p_u64), lens.ctypes.data_as(p_u64), capacity)
        return rc, hit_offsets, ids, lens

    try:
        gpu.tune("overlap_batch", 64)
        rc, ho, ids, lens = call(0)
        assert rc == 0 and np.array_equal(ho, want[0]) and np.all(ids == FILL) and np.all(lens == FILL)
        rc, ho, ids, lens = call(total - 1)
        assert rc == 1 and "bwtm_overlap_batch: capacity %d is too small (%d hits)" % (total - 1, total) in lib.bwtm_last_error().decode()
        assert np.array_equal(ho, want[0]) and np.all(ids == FILL) and np.all(lens == FILL)
        rc, ho, ids, lens = call(total)
    finally:
        gpu.tune("overlap_batch", 0)
    assert rc == 0 and same((ho, ids[:total], lens[:total]), want) and np.all(ids[total:] == FILL) and np.all(lens[total:] == FILL)


def test_every_form_of_an_index(gpu, oracle):
    """An uploaded native stream, the result of a merge (ids >= a.sequences are b's reads; a read planted in both sides overlaps across
    them), a builder's result (records only)."""
    ra, la = overlap_reads(400, 3)
    rb, lb = overlap_reads(270, 4)
    assert la[15] == 40 and lb[7] == 40
    rb[7] = ra[15]
    fa = oracle.FMI.from_text(text_of(ra, la))
    A = gpu.Index.upload(fa.data, fa.sequences, fa.bases); B = uploaded(gpu, oracle, rb, lb)
    both, both_len = np.concatenate([ra, rb]), np.concatenate([la, lb])

    def whole_check(index, reads, lengths):
        rows = rows_of(reads, lengths)
        loc = index.locator(max_len=WIDTH)
        want = expected(prefix_table(rows), rows, TAU)
        got = sequences_raw(gpu, loc, TAU, first=0, count=len(rows))
        assert same(got, want) and same(patterns_raw(gpu, loc, TAU, rows), want)
        loc.free()
        return got

    whole_check(A, ra, la)
    M = gpu.merge(A, B)
    assert M.sequences == 670
    hit_offsets, ids, lengths = whole_check(M, both, both_len)
    mine = list(zip(ids[int(hit_offsets[15]): int(hit_offsets[16])].tolist(), lengths[int(hit_offsets[15]): int(hit_offsets[16])].tolist()))
    assert mine[:2] == [(15, 40), (407, 40)]                             # equal reads in the order of their ids, across the two sides
    assert any(t >= 400 for t in ids[: int(hit_offsets[400])].tolist()) and any(t < 400 for t in ids[int(hit_offsets[400]):].tolist())
    bld = gpu.Builder(128)
    bld.add(both, both_len)
    X = bld.finish()
    assert X.nbytes == 0                                                  # not encoded: records and super table only
    whole_check(X, both, both_len)
    for h in (X, M, A, B):
        h.free()


def test_record_and_super_row_boundaries(gpu):
    """One index of more than 2^25 positions (340 000 iid reads of 100 bp): the searches cross records and read the super table's second
    row.  4 096 sampled reads as queries, threshold 10: every hit spells, the counts per query and length are those of the regenerated
    rows (packed prefixes of all reads, sorted and searched per length), and every query finds itself over its whole length."""
    import torch
    from bwt_merge_amd import synth
    n, L, seed, tau, K, Q = 340_000, 100, 7106, 10, 21, 4096
    assert n * (L + 1) > (1 << 25)
    sym = synth.leaf_bwt(synth.generate_reads(seed, 0, n, L, device=torch.device("cuda", 0))).contiguous()
    torch.cuda.synchronize()
    x = gpu.Index.from_symbols_device(sym.data_ptr(), sym.numel())
    del sym
    assert x.sequences == n and x.bases == n * (L + 1)
    loc = x.locator(max_len=L)
    queries = np.random.default_rng(14).integers(0, n, size=Q)
    hit_offsets, ids, lengths = sequences_raw(gpu, loc, tau, ids=queries)
    per_query = np.diff(hit_offsets.astype(np.int64))
    owner = np.repeat(np.arange(Q), per_query)
    rows = synth.generate_reads(seed, 0, n, L).numpy()
    qrows = rows[queries]
    # every hit spells: the first l symbols of the target are the last l symbols of the query
    l = lengths.astype(np.int64)
    assert l.min() >= tau and l.max() <= L
    cols = np.arange(L)[None, :]
    mask = cols < l[:, None]
    tail = qrows[owner[:, None], np.minimum(L - l[:, None] + cols, L - 1)]
    assert np.array_equal(np.where(mask, rows[ids.astype(np.int64)], 0), np.where(mask, tail, 0))
    # order: lengths descending within a query
    inside = owner[1:] == owner[:-1]
    assert np.all(l[1:][inside] <= l[:-1][inside])
    first_hit = hit_offsets[:-1].astype(np.int64)
    assert np.all(per_query >= 1) and np.all(l[first_hit] == L)
    assert all(int(queries[k]) in ids[int(hit_offsets[k]): int(hit_offsets[k + 1])][lengths[int(hit_offsets[k]): int(hit_offsets[k + 1])] == L] for k in range(Q))
    # expected counts per (query, length): K = 21 symbols of 3 bits in one 64-bit key, first symbol highest
    weights = (np.uint64(1) << (np.uint64(3) * np.arange(K - 1, -1, -1, dtype=np.uint64)))
    keys = (rows[:, :K].astype(np.uint64) * weights[None, :]).sum(axis=1, dtype=np.uint64)
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    want = np.zeros((Q, L + 1), dtype=np.int64)
    for length in range(tau, L + 1):
        head = min(length, K)
        suffix = qrows[:, L - length:]
        v = (suffix[:, :head].astype(np.uint64) * weights[None, K - head:]).sum(axis=1, dtype=np.uint64)
        shift = np.uint64(3 * (K - head))
        lo = np.searchsorted(keys, v << shift, side="left")
        hi = np.searchsorted(keys, ((v + np.uint64(1)) << shift) - np.uint64(1), side="right")
        if length <= K:
            want[:, length] = hi - lo
        else:
            for k in np.nonzero(hi > lo)[0].tolist():                       # candidates that share the key are compared in full
                cand = order[lo[k]: hi[k]]
                want[k, length] = int(np.sum(np.all(rows[cand, :length] == suffix[k][None, :], axis=1)))
    got = np.zeros((Q, L + 1), dtype=np.int64)
    np.add.at(got, (owner, l), 1)
    assert np.array_equal(got, want)
    assert want[:, tau: L].sum() > Q // 8                                                    # overlaps beyond the reads themselves exist
    loc.free()
    x.free()


def test_errors_without_hangs(gpu, oracle):
    x, loc, rows, table = collection(gpu, oracle, 300, 1)
    lib, p_u64, p_u8 = gpu.capi.lib(), gpu.capi.p_u64, gpu.capi.p_u8
    want = expected(table, rows, TAU)

    def batch_rc(text, offsets, tau=TAU):
        text = np.ascontiguousarray(text, dtype=np.uint8); offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        hit_offsets = np.zeros(offsets.size, dtype=np.uint64)
        rc = lib.bwtm_overlap_batch(loc.h, text.ctypes.data_as(p_u8), offsets.ctypes.data_as(p_u64), offsets.size - 1, tau, 0, hit_offsets.ctypes.data_as(p_u64), None, None, 0)
        return rc, lib.bwtm_last_error().decode()

    with pytest.raises(gpu.BwtmError) as e:
        loc.overlaps(min_overlap=0)
    assert "min_overlap" in str(e.value)
    with pytest.raises(gpu.BwtmError) as e:
        loc.overlap_patterns([(1, 2, 3)], 0)
    assert "min_overlap" in str(e.value)
    rc, msg = batch_rc([1, 2, 3, 4, 1, 0, 2, 3], [0, 3, 8])
    assert rc == 1 and "query 1 holds the symbol 0 at offset 2" in msg, msg
    rc, msg = batch_rc([1, 2, 6, 4, 1, 1, 2, 3], [0, 3, 8])
    assert rc == 1 and "query 0 holds the symbol 6 at offset 2" in msg, msg
    rc, msg = batch_rc([1, 2, 3, 4, 1, 1, 2, 3], [0, 5, 3, 8])
    assert rc == 1 and "offsets must not decrease (query 1)" in msg, msg
    rc, msg = batch_rc([0, 2, 3, 4, 1, 1, 2, 3], [0, 3, 5, 4])                   # two faults: the offsets are looked at before any text is read through them
    assert rc == 1 and "offsets must not decrease (query 2)" in msg, msg
    with pytest.raises(gpu.BwtmError) as e:
        loc.overlaps(ids=[3, 300, 4], min_overlap=TAU)
    assert "sequence 300 out of range (300 sequences)" in str(e.value)
    with pytest.raises(gpu.BwtmError) as e:
        loc.overlaps(first=299, count=2, min_overlap=TAU)
    assert "sequence 300 out of range" in str(e.value)
    total = int(want[0][-1])
    hit_offsets = np.zeros(301, dtype=np.uint64)
    ids = np.full(total, FILL, dtype=np.uint64); lens = np.full(total, FILL, dtype=np.uint64)
    rc = lib.bwtm_overlap_sequences(loc.h, None, 0, 300, TAU, 0, hit_offsets.ctypes.data_as(p_u64), ids.ctypes.data_as(p_u64), lens.ctypes.data_as(p_u64), total - 1)   # one slot short
    assert rc == 1 and b"capacity" in lib.bwtm_last_error()
    assert np.array_equal(hit_offsets, want[0]) and np.all(ids == FILL) and np.all(lens == FILL)
    for call in (lambda ho: lib.bwtm_overlap_sequences(loc.h, None, 0, 0, TAU, 0, ho, None, None, 0), lambda ho: lib.bwtm_overlap_batch(loc.h, None, None, 0, TAU, 0, ho, None, None, 0)):
        hit_offsets = np.full(1, 99, dtype=np.uint64)
        gpu.capi.check(call(hit_offsets.ctypes.data_as(p_u64)))          # count == 0
        assert hit_offsets.tolist() == [0]
    got = loc.overlaps(ids=[], min_overlap=TAU)
    assert got[0].tolist() == [0] and got[1].size == 0
    assert same(sequences_raw(gpu, loc, TAU, first=0, count=300), want)   # the locator still answers
    # a read longer than the locator's bound cannot pass its build; the locator of a smaller bound is refused, not half built
    with pytest.raises(gpu.BwtmError) as e:
        x.locator(max_len=20)
    assert re.search(r"longer than max_len = 20", str(e.value))
    loc.free()
    with pytest.raises(gpu.BwtmError):
        loc.overlaps(min_overlap=TAU)
    off, text = x.sequences(first=0, count=300)                           # the index still answers
    assert np.array_equal(text, np.array([v for r in rows for v in r], dtype=np.uint8))
    x.free()


def test_on_a_poisoned_pool(bwtm):
    """The all-reads case and the batching case in a fresh process whose pool hands out blocks filled with 0xA5A5A5A5: every count, base,
    record and output that is read was written by the kernels."""
    env = dict(os.environ, BWTM_POOL_POISON="0xA5A5A5A5")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "overlap_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), "exit status %s\n%s%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
    assert got and int(got.group(1)) > 0 and int(got.group(2)) >= 256 * int(got.group(1)), out.stdout[-3000:]
