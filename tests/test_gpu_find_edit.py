"""Patterns within edit distance e on the GPU (bwtm_find_edit_batch, Index.find_edit, Locator.locate_edit).  Every case is exact: hit_offsets,
sp, count, edits, lengths and the order.  Expected values come from the reads the test itself made -- the full Levenshtein matrix of every
distinct window of the text (tests/edit_inputs.py, pinned to the oracle in tests/test_find_edit_host.py) -- never the library's own search."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from approx_inputs import cut_patterns
from approx_inputs import expected as hamming_expected
from edit_inputs import (EditCollection, batch_peaks, collection, expected, genome_reads, memory_patterns, mixed_budget, mixed_expected, mixed_patterns,
                         mixed_peaks, peak_formula, text_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RECORD = 128
NAMES = ("hit_offsets", "sp", "count", "edits", "lengths")


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    return bwtm


def uploaded(gpu, oracle, rows):
    f = oracle.FMI.from_text(text_of(list(rows)))
    assert f.sequences == len(rows)
    return gpu.Index.upload(f.data, f.sequences, f.bases)


@pytest.fixture(scope="module")
def indexes(gpu, oracle):
    made = {name: uploaded(gpu, oracle, collection(name).rows) for name in ("iid", "genome")}
    yield made
    for x in made.values():
        x.free()


def same(got, want):
    assert len(got) == 5
    for g, w, what in zip(got, want, NAMES):
        assert g.dtype == w.dtype and np.array_equal(g, w), what


def pack(patterns):
    offsets = np.zeros(len(patterns) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(p) for p in patterns])
    text = np.concatenate([np.asarray(p, dtype=np.uint8) for p in patterns] + [np.zeros(0, dtype=np.uint8)])
    return np.ascontiguousarray(text), offsets


GUARD64, GUARD32, GUARD8 = 0xFEEDFACECAFEBEEF, 0xDEADBEEF, 0xEE
GUARDS = (GUARD64, GUARD64, GUARD8, GUARD32)


def raw(gpu, x, patterns, e, max_hits, capacity, size, fill=(True, True, True, True), hit_offsets=True, text_offsets=None):
    """One C call with arrays of `size` entries filled with guard values; returns (rc, hit_offsets, sp, count, edits, lengths)."""
    p_u8, p_u32, p_u64 = gpu.capi.p_u8, gpu.capi.p_u32, gpu.capi.p_u64
    text, offsets = pack(patterns) if text_offsets is None else text_offsets
    ho = np.full(offsets.size, GUARD64, dtype=np.uint64)
    sp, cnt = np.full(size, GUARD64, dtype=np.uint64), np.full(size, GUARD64, dtype=np.uint64)
    ed, ln = np.full(size, GUARD8, dtype=np.uint8), np.full(size, GUARD32, dtype=np.uint32)
    rc = gpu.capi.lib().bwtm_find_edit_batch(x.h, text.ctypes.data_as(p_u8), offsets.ctypes.data_as(p_u64), offsets.size - 1, e, max_hits,
                                             ho.ctypes.data_as(p_u64) if hit_offsets else None,
                                             sp.ctypes.data_as(p_u64) if fill[0] else None, cnt.ctypes.data_as(p_u64) if fill[1] else None,
                                             ed.ctypes.data_as(p_u8) if fill[2] else None, ln.ctypes.data_as(p_u32) if fill[3] else None, capacity)
    return rc, ho, sp, cnt, ed, ln


def last_error(gpu):
    return gpu.capi.lib().bwtm_last_error().decode()


def per_pattern(got, j):
    a, b = int(got[0][j]), int(got[0][j + 1])
    return tuple(arr[a:b].tolist() for arr in got[1:])


@pytest.mark.parametrize("e", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["iid", "genome"])
def test_mixed_lengths_and_budgets(gpu, indexes, name, e):
    patterns = mixed_budget(mixed_patterns(name), e)
    want = mixed_expected(name, e)
    got = indexes[name].find_edit(patterns, e)
    same(got, want)
    P, H, T = mixed_peaks(name, e)
    stats = gpu.find_edit_stats()
    longest = max(len(p) for p in patterns)
    assert 1 <= stats["levels"] <= longest + e and stats["frontier_peak"] == P and stats["batch_hits"] == H == int(want[0][-1])
    for j, p in enumerate(patterns):
        if len(p) <= e:                                                           # the empty string comes first: everywhere, at the cost of the whole pattern
            h = int(want[0][j])
            assert (int(got[1][h]), int(got[2][h]), int(got[3][h]), int(got[4][h])) == (0, indexes[name].bases, len(p), 0)
    if e == 3:
        assert stats["frontier_peak"] > 20 * 256                                  # many workgroups, crossed raggedly


@pytest.mark.parametrize("name", ["iid", "genome"])
def test_budget_zero_is_find(gpu, indexes, name):
    x, coll = indexes[name], collection(name)
    patterns = [p for p in cut_patterns(coll.rows, (1, 2, 3, 12, 31, 40, 41), 8, 21, substitutions=0) + mixed_patterns(name) if len(p) > 0]
    fsp, fep = x.find(patterns)
    got = x.find_edit(patterns, 0)
    hit_offsets, sp, count, edits, lengths = got
    found = 0
    for j in range(len(patterns)):
        a, b = int(hit_offsets[j]), int(hit_offsets[j + 1])
        if int(fsp[j]) <= int(fep[j]) and int(fep[j]) < x.bases:
            assert b - a == 1 and (int(sp[a]), int(sp[a] + count[a]) - 1, int(edits[a]), int(lengths[a])) == (int(fsp[j]), int(fep[j]), 0, len(patterns[j])), j
            found += 1
        else:
            assert b == a, j
    assert 40 <= found < len(patterns)
    approx = x.find_approx(patterns, 0)
    assert all(np.array_equal(g, w) for g, w in zip(got[:4], approx))
    same(got, expected(coll, patterns, 0))
    assert all(np.array_equal(g, w) for g, w in zip(got[:4], hamming_expected(coll, patterns, 0)))


@pytest.mark.parametrize("m", [1, 2])
def test_budget_that_covers_the_pattern(gpu, indexes, m):
    """e = 7 >= m: every distinct string of 0 .. m + 7 symbols within distance is a hit, the empty one first."""
    coll = collection("iid")
    p = cut_patterns(coll.rows, (m,), 1, 30 + m)[0]
    got = indexes["iid"].find_edit([p], 7)
    same(got, expected(coll, [p], 7))
    hit_offsets, sp, count, edits, lengths = got
    assert (int(sp[0]), int(count[0]), int(edits[0]), int(lengths[0])) == (0, indexes["iid"].bases, m, 0)
    assert sorted(set(lengths.tolist())) == list(range(0, m + 8)) and int(edits.max()) == 7
    ones = lengths == 1                                                           # every string of one symbol is within 7 edits of one or two
    assert int(ones.sum()) == 5 and int(count[ones].sum()) == int(sum(r.size for r in coll.rows))
    for length in (1, 2, 3, 4):                                                   # every distinct string of these lengths: the budget covers them all
        assert int((lengths == length).sum()) == coll.distinct(length)[0].shape[0]


def test_a_hit_that_is_also_a_parent(gpu, oracle):
    """W and cW are both hits: both are reported, and the search goes on beneath cW."""
    rows = [np.array([1, 2, 3, 4, 1, 1, 2, 2, 3, 3], dtype=np.uint8), np.array([4, 3, 2, 3, 4, 1, 1, 2, 2], dtype=np.uint8), np.array([2, 3, 4, 1, 1, 2], dtype=np.uint8)]
    coll = EditCollection(rows)
    x = uploaded(gpu, oracle, rows)
    p = np.array([3, 4, 1, 1, 2], dtype=np.uint8)
    for e in (1, 2):
        got = x.find_edit([p], e)
        same(got, expected(coll, [p], e))
        strings = [s.tobytes() for s in coll.edit_hits(p, e)[4]]
        w, cw, ccw = bytes([4, 1, 1, 2]), bytes([3, 4, 1, 1, 2]), bytes([2, 3, 4, 1, 1, 2])
        assert w in strings and cw in strings and ccw in strings                  # a hit, its child, and a hit beneath that one
        at = [strings.index(s) for s in (w, cw, ccw)]
        assert got[3][at].tolist() == [1, 0, 1] and got[4][at].tolist() == [4, 5, 6]
        assert got[2][at].tolist() == [3, 3, 3]                                   # each of the three reads holds all of them once
    x.free()


def test_n_is_a_symbol_and_repeats_get_equal_results(gpu, indexes):
    coll = collection("iid")
    with_n = [r for r in coll.rows if (r[10:22] == 5).any()][:10]
    assert len(with_n) == 10
    patterns = [r[10:22].copy() for r in with_n] + [r[5:17].copy() for r in coll.rows[:10]]
    for p in patterns[10:]:
        p[4] = 5                                                                  # an N the read does not have: found at the cost of one edit
    patterns = patterns + [patterns[3], patterns[12]] + [patterns[3], patterns[12]]
    for e in (0, 1, 2):
        got = indexes["iid"].find_edit(patterns, e)
        same(got, expected(coll, patterns, e))
        per = [per_pattern(got, j) for j in range(len(patterns))]
        assert per[3] == per[20] == per[22] and per[12] == per[21] == per[23]
        assert all(len(per[j][0]) >= 1 for j in range(10)) and (e == 0 or all(len(per[j][0]) >= 1 for j in range(10, 20)))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_ranges_that_end_at_n_on_a_record_edge(gpu, oracle, delta):
    """n = 32 records exactly (128 reads of 31 symbols and their endmarkers), one less and one more; patterns that match the largest suffixes."""
    rng = np.random.default_rng(60 + delta)
    rows = [rng.integers(1, 5, size=31).astype(np.uint8) for _ in range(128)]
    rows[5] = rng.integers(1, 5, size=31 + delta).astype(np.uint8)
    rows[77][-4:] = 4
    rows[3][:6] = 4
    x = uploaded(gpu, oracle, rows)
    n = x.bases
    assert n == 32 * RECORD + delta
    coll = EditCollection(rows)
    patterns = [np.full(m, 4, dtype=np.uint8) for m in (1, 2, 3, 4, 6)] + [np.array([4, 4, 3, 4], dtype=np.uint8), np.array([1, 4, 4, 4, 4], dtype=np.uint8), rows[3][:9].copy()]
    for e in (0, 1, 2):
        got = x.find_edit(patterns, e)
        same(got, expected(coll, patterns, e))
        ends = got[1] + got[2]
        assert int(ends.max()) == n and int((ends == n).sum()) >= 5               # the all-4 strings: their ranges end at n
    x.free()


def test_batches_give_the_same_result(gpu, indexes):
    patterns = mixed_patterns("genome")
    want = mixed_expected("genome", 2)
    try:
        for batch in (7, 1):
            gpu.tune("approx_batch", batch)
            same(indexes["genome"].find_edit(patterns, 2), want)
            same(indexes["genome"].find_edit(patterns, 2, max_hits=2), expected(collection("genome"), patterns, 2, max_hits=2))
    finally:
        gpu.tune("approx_batch", 0)
    same(indexes["genome"].find_edit(patterns, 2), want)


def batched_patterns():
    """33 patterns for approx_batch = 7, five batches: seven mixed ones; the seven empty ones, which the empty string and every single symbol
    are within one edit of (the batch has no text); seven mixed; seven random 20-mers that nothing in the reads is near (no hit: the batch
    contributes nothing); five mixed."""
    mixed = [p for p in mixed_patterns("genome") if 0 < len(p) <= 12]
    none = [np.random.default_rng(70 + j).integers(1, 5, size=20).astype(np.uint8) for j in range(7)]
    return mixed[:7] + [np.zeros(0, dtype=np.uint8)] * 7 + mixed[7:14] + none + mixed[14:19]


def test_the_two_rounds_of_a_call_of_many_batches(gpu, indexes):
    """approx_batch = 7, so that the call searches every batch twice: the sizing call, a capacity one short, the exact capacity; the
    statistics of the filling call are those of the sizing call; a batch of empty patterns and a batch without hits in the middle."""
    x, coll, patterns = indexes["genome"], collection("genome"), batched_patterns()
    want = expected(coll, patterns, 1)
    per = np.diff(want[0].astype(np.int64))
    total = int(want[0][-1])
    assert len(patterns) == 33 and len(set(per[7:14].tolist())) == 1 and per[7] >= 2 and not per[21:28].any() and per[:7].sum() > 7 and per[28:].sum() > 5
    assert np.all(want[0][21:29] == want[0][21])                                  # flat across the fourth batch
    untouched = lambda arrays: all(np.all(a == g) for a, g in zip(arrays, GUARDS))
    try:
        gpu.tune("approx_batch", 7)
        rc, ho, *arrays = raw(gpu, x, patterns, 1, 0, 0, total + 3)
        sized = gpu.find_edit_stats()
        assert rc == 0 and np.array_equal(ho, want[0]) and untouched(arrays)
        rc, ho, *arrays = raw(gpu, x, patterns, 1, 0, total - 1, total + 3)
        assert rc == 1 and "bwtm_find_edit_batch: capacity %d is too small (%d hits)" % (total - 1, total) in last_error(gpu)
        assert np.array_equal(ho, want[0]) and untouched(arrays)
        rc, ho, *arrays = raw(gpu, x, patterns, 1, 0, total, total + 3)
        filled = gpu.find_edit_stats()
    finally:
        gpu.tune("approx_batch", 0)
    assert rc == 0
    same((ho,) + tuple(a[:total] for a in arrays), want)
    assert untouched([a[total:] for a in arrays])
    assert filled == sized and sized["expanded"] > len(patterns) and sized["frontier_peak"] >= 7      # the second round leaves no trace
    h = int(want[0][7])
    assert (int(arrays[0][h]), int(arrays[1][h]), int(arrays[2][h]), int(arrays[3][h])) == (0, x.bases, 0, 0)    # the empty string first


def test_max_hits_sizes_capacity_and_null_arrays(gpu, indexes):
    x, coll, patterns = indexes["iid"], collection("iid"), mixed_patterns("iid")
    full = mixed_expected("iid", 2)
    most = int(np.diff(full[0]).max())
    assert most > 2
    for max_hits in (1, 2, most + 5):
        want = expected(coll, patterns, 2, max_hits=max_hits)
        same(x.find_edit(patterns, 2, max_hits=max_hits), want)
        for j in range(len(patterns)):                                            # the prefix of the full list
            a, k = int(full[0][j]), int(want[0][j + 1] - want[0][j])
            assert k == min(int(full[0][j + 1]) - a, max_hits)
            assert all(np.array_equal(w[int(want[0][j]): int(want[0][j + 1])], f[a: a + k]) for w, f in zip(want[1:], full[1:]))
    total = int(full[0][-1])
    untouched = lambda arrays: all(np.all(a == g) for a, g in zip(arrays, GUARDS))
    # sizes only: capacity 0, or no arrays
    for capacity, fill in ((0, (True, True, True, True)), (total, (False, False, False, False))):
        rc, ho, *arrays = raw(gpu, x, patterns, 2, 0, capacity, total + 3, fill=fill)
        assert rc == 0 and np.array_equal(ho, full[0]) and untouched(arrays)
    # one short
    rc, ho, *arrays = raw(gpu, x, patterns, 2, 0, total - 1, total + 3)
    assert rc != 0 and "capacity %d is too small (%d hits)" % (total - 1, total) in last_error(gpu)
    assert untouched(arrays)
    with pytest.raises(gpu.BwtmError):
        gpu.capi.check(rc)
    # exact and generous capacities; nothing behind hit_offsets[count] is touched
    for capacity in (total, total + 3):
        rc, ho, *arrays = raw(gpu, x, patterns, 2, 0, capacity, total + 3)
        assert rc == 0
        same((ho,) + tuple(a[:total] for a in arrays), full)
        assert untouched([a[total:] for a in arrays])
    # any one of the arrays missing
    for missing in range(4):
        fill = tuple(j != missing for j in range(4))
        rc, ho, *arrays = raw(gpu, x, patterns, 2, 0, total, total + 3, fill=fill)
        assert rc == 0 and np.array_equal(ho, full[0])
        for j, (got, want, guard) in enumerate(zip(arrays, full[1:], GUARDS)):
            if j == missing:
                assert np.all(got == guard)
            else:
                assert np.array_equal(got[:total], want) and np.all(got[total:] == guard)
    # no patterns at all
    rc, ho, *arrays = raw(gpu, x, [], 2, 0, 0, 3)
    assert rc == 0 and ho.tolist() == [0] and untouched(arrays)


def test_argument_errors(gpu, oracle, indexes):
    x = indexes["iid"]
    ones = lambda m: np.ones(m, dtype=np.uint8)
    good = [ones(3), ones(4)]

    def refused(what, **kw):
        args = dict(patterns=good, e=1, max_hits=0, capacity=0, size=1)
        args.update(kw)
        rc = raw(gpu, x, **args)[0]
        assert rc != 0 and what in last_error(gpu), last_error(gpu)
        with pytest.raises(gpu.BwtmError):
            gpu.capi.check(rc)

    refused("null argument", hit_offsets=False)
    refused("max_edits = 8", e=8)
    refused("pattern 1 holds the symbol 0 at offset 2", patterns=[ones(3), np.array([1, 2, 0, 3], dtype=np.uint8)])
    refused("pattern 2 holds the symbol 6 at offset 0", patterns=[ones(3), ones(0), np.array([6], dtype=np.uint8)])
    refused("offsets must not decrease (pattern 1)", text_offsets=(ones(8), np.array([0, 3, 2, 8], dtype=np.uint64)))
    refused("pattern 1 has 65536 symbols", patterns=[ones(2), ones(65536)])
    # two faults: the offsets are looked at before any text is read through them
    refused("offsets must not decrease (pattern 2)", text_offsets=(np.array([0, 2, 3, 4, 1, 1, 2, 3], dtype=np.uint8), np.array([0, 3, 5, 4], dtype=np.uint64)))
    assert gpu.capi.lib().bwtm_find_edit_batch(None, None, None, 0, 0, 0, None, None, None, None, None, 0) != 0 and "null argument" in last_error(gpu)
    # the longest pattern that is accepted, and the index still answers
    got = x.find_edit([ones(65535)], 0)
    assert got[0].tolist() == [0, 0]
    same(x.find_edit(mixed_patterns("iid"), 1), mixed_expected("iid", 1))
    # a window of an index
    from parts_inputs import host
    fa = oracle.FMI.from_text(text_of(list(genome_reads(21)[:400])))
    ha = host(gpu, fa)
    b0, b1, fp, before_counts = gpu.window_blocks(ha, 1000, 5000)
    Cs = (C.c_uint64 * 7)(*[int(v) for v in fa.C])
    out = gpu.capi.vp()
    data = fa.data                                                               # a copy of the native bytes, alive over the call
    gpu.capi.check(gpu.capi.lib().bwtm_index_upload_window(data.ctypes.data + 64 * b0, 64 * (b1 - b0), fp, before_counts, int(fa.bases), int(fa.sequences), Cs, 0, C.byref(out)))
    W = gpu.Index(out)
    with pytest.raises(gpu.BwtmError) as err:
        W.find_edit(good, 1)
    assert "window" in str(err.value)
    W.free()
    same(x.find_edit(mixed_patterns("iid"), 1), mixed_expected("iid", 1))


def test_the_same_call_twice_gives_identical_arrays(gpu, indexes):
    patterns = mixed_budget(mixed_patterns("iid"), 3)
    a = indexes["iid"].find_edit(patterns, 3)
    b = indexes["iid"].find_edit(patterns, 3)
    same(a, b)
    same(a, mixed_expected("iid", 3))


def test_device_memory_stays_within_the_documented_bound(gpu, indexes):
    x, coll = indexes["iid"], collection("iid")
    patterns = memory_patterns()
    P, H, T = batch_peaks(coll, patterns, 3)
    assert P > 20 * 256 and H > len(patterns)                                    # the frontier spans many workgroups
    want = expected(coll, patterns, 3)
    assert int(want[0][-1]) == H
    gpu.synchronize()
    gpu.trim()                                                                    # what the pool has cached so far is not this call's
    held = gpu.pool_stats()["held_bytes"]
    gpu.device_bytes_peak(reset=True)
    rc, ho, *arrays = raw(gpu, x, patterns, 3, 0, H, H)                           # one call: the capacity is known from the brute force
    peak = gpu.device_bytes_peak()
    assert rc == 0
    same((ho,) + tuple(arrays), want)
    stats = gpu.find_edit_stats()
    assert (stats["frontier_peak"], stats["batch_hits"]) == (P, H)
    assert held <= peak <= held + peak_formula(P, H, T, 3), (held, peak, peak_formula(P, H, T, 3))
    assert peak - held >= 32 * P + 24 * H                                         # the reset took: the call's own frontier and hits are in the figure


def test_locate_edit_gives_the_occurrences(gpu, indexes):
    x, coll = indexes["genome"], collection("genome")
    patterns = [p for p in mixed_patterns("genome") if 3 <= len(p) <= 40][:16]
    loc = x.locator(max_len=40)
    hit_offsets, sp, count, edits, lengths, occ_offsets, ids, offs = loc.locate_edit(patterns, 1)
    same((hit_offsets, sp, count, edits, lengths), expected(coll, patterns, 1))
    assert np.array_equal(np.diff(occ_offsets), count)
    some = 0
    for j, p in enumerate(patterns):
        got = set()
        for h in range(int(hit_offsets[j]), int(hit_offsets[j + 1])):
            for o in range(int(occ_offsets[h]), int(occ_offsets[h + 1])):
                got.add((int(ids[o]), int(offs[o]), int(edits[h]), int(lengths[h])))
        want = coll.edit_hits(p, 1, want_occurrences=True)[5]
        assert got == want and len(got) == int(count[int(hit_offsets[j]): int(hit_offsets[j + 1])].sum()), j
        some += len(got)
    assert some > len(patterns)
    loc.free()


def test_on_a_poisoned_pool(bwtm):
    """The mixed-length case in a fresh process whose pool hands out blocks filled with 0xA5A5A5A5: every total, slot, band and node that is
    read was written by the kernels."""
    env = dict(os.environ, BWTM_POOL_POISON="0xA5A5A5A5")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "edit_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), "exit status %s\n%s%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
    assert got and int(got.group(1)) > 0 and int(got.group(2)) >= 256 * int(got.group(1)), out.stdout[-3000:]
