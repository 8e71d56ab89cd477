"""Patterns with up to d substitutions on the GPU (bwtm_find_approx_batch, Index.find_approx, Locator.locate_approx).  Every case is exact:
hit_offsets, sp, count, mismatches and the order.  Expected values come from the reads the test itself made -- a brute force over every
window of the text (tests/approx_inputs.py, pinned to the oracle in tests/test_find_approx_host.py) -- never the library's own search."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from approx_inputs import Collection, batch_peaks, cut_patterns, expected, genome_reads, iid_reads, peak_formula, text_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RECORD = 128
MIXED_LENGTHS = (0, 1, 2, 3, 12, 31, 40, 41)


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    return bwtm


def uploaded(gpu, oracle, rows):
    f = oracle.FMI.from_text(text_of(list(rows)))
    assert f.sequences == len(rows)
    return gpu.Index.upload(f.data, f.sequences, f.bases)


@functools.lru_cache(maxsize=None)
def collection(name):
    return Collection(list({"iid": iid_reads, "genome": genome_reads}[name]()))


@pytest.fixture(scope="module")
def indexes(gpu, oracle):
    made = {name: uploaded(gpu, oracle, collection(name).rows) for name in ("iid", "genome")}
    yield made
    for x in made.values():
        x.free()


def mixed_patterns(name):
    """96 patterns of the lengths 0 .. 41, each cut from a read with one substitution, in mixed order: they finish at different levels."""
    patterns = cut_patterns(collection(name).rows, MIXED_LENGTHS, 12, 7 if name == "iid" else 8)
    order = np.random.default_rng(9).permutation(len(patterns))
    return [patterns[j] for j in order.tolist()]


@functools.lru_cache(maxsize=None)
def mixed_expected(name, d):
    return expected(collection(name), mixed_patterns(name), d)


def same(got, want):
    assert len(got) == 4
    for g, w, what in zip(got, want, ("hit_offsets", "sp", "count", "mismatches")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what


def pack(patterns):
    offsets = np.zeros(len(patterns) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(p) for p in patterns])
    text = np.concatenate([np.asarray(p, dtype=np.uint8) for p in patterns] + [np.zeros(0, dtype=np.uint8)])
    return np.ascontiguousarray(text), offsets


GUARD64, GUARD8 = 0xFEEDFACECAFEBEEF, 0xEE


def raw(gpu, x, patterns, d, max_hits, capacity, size, fill=(True, True, True), hit_offsets=True, text_offsets=None):
    """One C call with arrays of `size` entries filled with guard values; returns (rc, hit_offsets, sp, count, mismatches)."""
    p_u8, p_u64 = gpu.capi.p_u8, gpu.capi.p_u64
    text, offsets = pack(patterns) if text_offsets is None else text_offsets
    ho = np.full(offsets.size, GUARD64, dtype=np.uint64)
    sp, cnt, mm = np.full(size, GUARD64, dtype=np.uint64), np.full(size, GUARD64, dtype=np.uint64), np.full(size, GUARD8, dtype=np.uint8)
    rc = gpu.capi.lib().bwtm_find_approx_batch(x.h, text.ctypes.data_as(p_u8), offsets.ctypes.data_as(p_u64), offsets.size - 1, d, max_hits,
                                               ho.ctypes.data_as(p_u64) if hit_offsets else None,
                                               sp.ctypes.data_as(p_u64) if fill[0] else None, cnt.ctypes.data_as(p_u64) if fill[1] else None,
                                               mm.ctypes.data_as(p_u8) if fill[2] else None, capacity)
    return rc, ho, sp, cnt, mm


def last_error(gpu):
    return gpu.capi.lib().bwtm_last_error().decode()


@pytest.mark.parametrize("d", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["iid", "genome"])
def test_mixed_lengths_and_budgets(gpu, indexes, name, d):
    patterns = mixed_patterns(name)
    want = mixed_expected(name, d)
    got = indexes[name].find_approx(patterns, d)
    same(got, want)
    stats = gpu.find_approx_stats()
    assert 1 <= stats["levels"] <= 41 and stats["frontier_peak"] >= len(patterns) and stats["batch_hits"] == int(want[0][-1])
    per_pattern = np.diff(want[0])
    for j, p in enumerate(patterns):
        if len(p) == 41:
            assert per_pattern[j] == 0
        if len(p) == 0:
            h = int(want[0][j])
            assert per_pattern[j] == 1 and (int(got[1][h]), int(got[2][h]), int(got[3][h])) == (0, indexes[name].bases, 0)
    if d == 3:
        assert stats["frontier_peak"] > 20 * 256                                  # many workgroups, crossed raggedly
    if d >= 1:
        assert int(per_pattern.max()) > 1 and int(got[3].max()) == d


@pytest.mark.parametrize("name", ["iid", "genome"])
def test_budget_zero_is_find(gpu, indexes, name):
    x = indexes[name]
    patterns = [p for p in cut_patterns(collection(name).rows, (1, 2, 3, 12, 31, 40, 41), 8, 21, substitutions=0) + mixed_patterns(name) if len(p) > 0]
    fsp, fep = x.find(patterns)
    hit_offsets, sp, count, mm = x.find_approx(patterns, 0)
    found = 0
    for j in range(len(patterns)):
        a, b = int(hit_offsets[j]), int(hit_offsets[j + 1])
        if int(fsp[j]) <= int(fep[j]) and int(fep[j]) < x.bases:
            assert b - a == 1 and (int(sp[a]), int(sp[a] + count[a]) - 1, int(mm[a])) == (int(fsp[j]), int(fep[j]), 0), j
            found += 1
        else:
            assert b == a, j
    assert 40 <= found < len(patterns)
    same((hit_offsets, sp, count, mm), expected(collection(name), patterns, 0))


@pytest.mark.parametrize("m", [1, 2, 6])
def test_budget_that_covers_the_pattern(gpu, indexes, m):
    """d = 8 >= m: every distinct string of m symbols in the collection is a hit, its mismatches its distance."""
    coll = collection("iid")
    p = cut_patterns(coll.rows, (m,), 1, 30 + m)[0]
    hit_offsets, sp, count, mm = indexes["iid"].find_approx([p], 8)
    want = coll.hits(p, 8)
    w, valid, _ = coll.windows(m)
    distinct = np.unique(w[valid], axis=0)
    assert int(hit_offsets[1]) == distinct.shape[0] == want[0].size and int(count.sum()) == int(valid.sum())
    assert distinct.shape[0] > 4 ** m                                             # strings with N are among them
    same((hit_offsets, sp, count, mm), expected(coll, [p], 8))
    assert np.array_equal(mm, (want[3] != p[None, :]).sum(axis=1)) and int(mm.max()) == m


def test_n_is_a_symbol_and_repeats_get_equal_results(gpu, indexes):
    coll = collection("iid")
    with_n = [r for r in coll.rows if (r[10:22] == 5).any()][:10]
    assert len(with_n) == 10
    patterns = [r[10:22].copy() for r in with_n] + [r[5:17].copy() for r in coll.rows[:10]]
    for p in patterns[10:]:
        p[4] = 5                                                                  # an N the read does not have: found at the cost of one mismatch
    patterns = patterns + [patterns[3], patterns[12]] + [patterns[3], patterns[12]]
    for d in (0, 1, 2):
        got = indexes["iid"].find_approx(patterns, d)
        same(got, expected(coll, patterns, d))
        per = [tuple(a[int(got[0][j]): int(got[0][j + 1])].tolist() for a in got[1:]) for j in range(len(patterns))]
        assert per[3] == per[20] == per[22] and per[12] == per[21] == per[23]
        assert all(len(per[j][0]) >= 1 for j in range(10)) and (d == 0 or all(len(per[j][0]) >= 1 for j in range(10, 20)))


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
    coll = Collection(rows)
    patterns = [np.full(m, 4, dtype=np.uint8) for m in (1, 2, 3, 4, 6)] + [np.array([4, 4, 3, 4], dtype=np.uint8), np.array([1, 4, 4, 4, 4], dtype=np.uint8), rows[3][:9].copy()]
    for d in (0, 1, 2):
        got = x.find_approx(patterns, d)
        same(got, expected(coll, patterns, d))
        ends = got[1] + got[2]
        assert int(ends.max()) == n and int((ends == n).sum()) >= 5               # the all-4 strings: their ranges end at n
    x.free()


def test_batches_give_the_same_result(gpu, indexes):
    patterns = mixed_patterns("genome")
    want = mixed_expected("genome", 2)
    try:
        for batch in (7, 1):
            gpu.tune("approx_batch", batch)
            same(indexes["genome"].find_approx(patterns, 2), want)
            same(indexes["genome"].find_approx(patterns, 2, max_hits=2), expected(collection("genome"), patterns, 2, max_hits=2))
    finally:
        gpu.tune("approx_batch", 0)
    same(indexes["genome"].find_approx(patterns, 2), want)


def batched_patterns():
    """33 patterns for approx_batch = 7, five batches: seven mixed ones; the seven empty ones, which every position matches (a hit each, and
    nothing else: the batch has no text); seven mixed; seven 41-mers, longer than any read (no hit: the batch contributes nothing); five mixed."""
    mixed = [p for p in mixed_patterns("genome") if 0 < len(p) < 41]
    none = cut_patterns(collection("genome").rows, (41,), 7, 51)
    return mixed[:7] + [np.zeros(0, dtype=np.uint8)] * 7 + mixed[7:14] + none + mixed[14:19]


def test_the_two_rounds_of_a_call_of_many_batches(gpu, indexes):
    """approx_batch = 7, so that the call searches every batch twice: the sizing call, a capacity one short, the exact capacity; the
    statistics of the filling call are those of the sizing call; a batch of empty patterns and a batch without hits in the middle."""
    x, coll, patterns = indexes["genome"], collection("genome"), batched_patterns()
    want = expected(coll, patterns, 2)
    per = np.diff(want[0].astype(np.int64))
    total = int(want[0][-1])
    assert len(patterns) == 33 and per[7:14].tolist() == [1] * 7 and not per[21:28].any() and per[:7].sum() > 7 and per[28:].sum() > 5
    assert np.all(want[0][21:29] == want[0][21])                                  # flat across the fourth batch
    try:
        gpu.tune("approx_batch", 7)
        rc, ho, sp, cnt, mm = raw(gpu, x, patterns, 2, 0, 0, total + 3)
        sized = gpu.find_approx_stats()
        assert rc == 0 and np.array_equal(ho, want[0]) and np.all(sp == GUARD64) and np.all(cnt == GUARD64) and np.all(mm == GUARD8)
        rc, ho, sp, cnt, mm = raw(gpu, x, patterns, 2, 0, total - 1, total + 3)
        assert rc == 1 and "bwtm_find_approx_batch: capacity %d is too small (%d hits)" % (total - 1, total) in last_error(gpu)
        assert np.array_equal(ho, want[0]) and np.all(sp == GUARD64) and np.all(cnt == GUARD64) and np.all(mm == GUARD8)
        rc, ho, sp, cnt, mm = raw(gpu, x, patterns, 2, 0, total, total + 3)
        filled = gpu.find_approx_stats()
    finally:
        gpu.tune("approx_batch", 0)
    assert rc == 0
    same((ho, sp[:total], cnt[:total], mm[:total]), want)
    assert np.all(sp[total:] == GUARD64) and np.all(cnt[total:] == GUARD64) and np.all(mm[total:] == GUARD8)
    assert filled == sized and sized["expanded"] > len(patterns) and sized["frontier_peak"] >= 7      # the second round leaves no trace
    h = int(want[0][7])
    assert sp[h: h + 7].tolist() == [0] * 7 and cnt[h: h + 7].tolist() == [x.bases] * 7 and not mm[h: h + 7].any()


def test_max_hits_sizes_capacity_and_null_arrays(gpu, indexes):
    x, coll, patterns = indexes["iid"], collection("iid"), mixed_patterns("iid")
    full = mixed_expected("iid", 2)
    most = int(np.diff(full[0]).max())
    assert most > 2
    for max_hits in (1, 2, most + 5):
        want = expected(coll, patterns, 2, max_hits=max_hits)
        same(x.find_approx(patterns, 2, max_hits=max_hits), want)
        for j in range(len(patterns)):                                            # the prefix of the full list
            a, k = int(full[0][j]), int(want[0][j + 1] - want[0][j])
            assert k == min(int(full[0][j + 1]) - a, max_hits)
            assert all(np.array_equal(w[int(want[0][j]): int(want[0][j + 1])], f[a: a + k]) for w, f in zip(want[1:], full[1:]))
    total = int(full[0][-1])
    # sizes only: capacity 0, or no arrays
    for capacity, fill in ((0, (True, True, True)), (total, (False, False, False))):
        rc, ho, sp, cnt, mm = raw(gpu, x, patterns, 2, 0, capacity, total + 3, fill=fill)
        assert rc == 0 and np.array_equal(ho, full[0])
        assert np.all(sp == GUARD64) and np.all(cnt == GUARD64) and np.all(mm == GUARD8)
    # one short
    rc, ho, sp, cnt, mm = raw(gpu, x, patterns, 2, 0, total - 1, total + 3)
    assert rc != 0 and "capacity %d is too small (%d hits)" % (total - 1, total) in last_error(gpu)
    assert np.all(sp == GUARD64) and np.all(cnt == GUARD64) and np.all(mm == GUARD8)
    with pytest.raises(gpu.BwtmError):
        gpu.capi.check(rc)
    # exact and generous capacities; nothing behind hit_offsets[count] is touched
    for capacity in (total, total + 3):
        rc, ho, sp, cnt, mm = raw(gpu, x, patterns, 2, 0, capacity, total + 3)
        assert rc == 0
        same((ho, sp[:total], cnt[:total], mm[:total]), full)
        assert np.all(sp[total:] == GUARD64) and np.all(cnt[total:] == GUARD64) and np.all(mm[total:] == GUARD8)
    # any one of the arrays missing
    for missing in range(3):
        fill = tuple(j != missing for j in range(3))
        rc, ho, sp, cnt, mm = raw(gpu, x, patterns, 2, 0, total, total + 3, fill=fill)
        assert rc == 0 and np.array_equal(ho, full[0])
        for j, (got, want, guard) in enumerate(((sp, full[1], GUARD64), (cnt, full[2], GUARD64), (mm, full[3], GUARD8))):
            if j == missing:
                assert np.all(got == guard)
            else:
                assert np.array_equal(got[:total], want) and np.all(got[total:] == guard)
    # no patterns at all
    rc, ho, sp, cnt, mm = raw(gpu, x, [], 2, 0, 0, 3)
    assert rc == 0 and ho.tolist() == [0]


def test_argument_errors(gpu, oracle, indexes):
    x = indexes["iid"]
    ones = lambda m: np.ones(m, dtype=np.uint8)
    good = [ones(3), ones(4)]

    def refused(what, **kw):
        args = dict(patterns=good, d=1, max_hits=0, capacity=0, size=1)
        args.update(kw)
        rc = raw(gpu, x, **args)[0]
        assert rc != 0 and what in last_error(gpu), last_error(gpu)
        with pytest.raises(gpu.BwtmError):
            gpu.capi.check(rc)

    refused("null argument", hit_offsets=False)
    refused("max_mismatches = 9", d=9)
    refused("pattern 1 holds the symbol 0 at offset 2", patterns=[ones(3), np.array([1, 2, 0, 3], dtype=np.uint8)])
    refused("pattern 2 holds the symbol 6 at offset 0", patterns=[ones(3), ones(0), np.array([6], dtype=np.uint8)])
    refused("offsets must not decrease (pattern 1)", text_offsets=(ones(8), np.array([0, 3, 2, 8], dtype=np.uint64)))
    refused("pattern 1 has 65536 symbols", patterns=[ones(2), ones(65536)])
    # two faults: the offsets are looked at before any text is read through them
    refused("offsets must not decrease (pattern 2)", text_offsets=(np.array([0, 2, 3, 4, 1, 1, 2, 3], dtype=np.uint8), np.array([0, 3, 5, 4], dtype=np.uint64)))
    assert gpu.capi.lib().bwtm_find_approx_batch(None, None, None, 0, 0, 0, None, None, None, None, 0) != 0 and "null argument" in last_error(gpu)
    # the longest pattern that is accepted, and the index still answers
    hit_offsets, sp, count, mm = x.find_approx([ones(65535)], 0)
    assert hit_offsets.tolist() == [0, 0]
    same(x.find_approx(mixed_patterns("iid"), 1), mixed_expected("iid", 1))
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
    with pytest.raises(gpu.BwtmError) as e:
        W.find_approx(good, 1)
    assert "window" in str(e.value)
    W.free()


def test_the_same_call_twice_gives_identical_arrays(gpu, indexes):
    patterns = mixed_patterns("iid")
    a = indexes["iid"].find_approx(patterns, 3)
    b = indexes["iid"].find_approx(patterns, 3)
    same(a, b)
    same(a, mixed_expected("iid", 3))


def test_device_memory_stays_within_the_documented_bound(gpu, indexes):
    x, coll = indexes["iid"], collection("iid")
    patterns = cut_patterns(coll.rows, (12,), 40, 41) + cut_patterns(coll.rows, (5,), 10, 42)
    P, H, T = batch_peaks(coll, patterns, 2)
    assert P > 20 * 256 and H > len(patterns)                                    # the frontier spans many workgroups
    want = expected(coll, patterns, 2)
    assert int(want[0][-1]) == H
    gpu.synchronize()
    gpu.trim()                                                                    # what the pool has cached so far is not this call's
    held = gpu.pool_stats()["held_bytes"]
    gpu.device_bytes_peak(reset=True)
    rc, ho, sp, cnt, mm = raw(gpu, x, patterns, 2, 0, H, H)                       # one call: the capacity is known from the brute force
    peak = gpu.device_bytes_peak()
    assert rc == 0
    same((ho, sp, cnt, mm), want)
    stats = gpu.find_approx_stats()
    assert (stats["frontier_peak"], stats["batch_hits"]) == (P, H)
    assert held <= peak <= held + peak_formula(P, H, T), (held, peak, peak_formula(P, H, T))
    assert peak - held >= 24 * P + 24 * H                                         # the reset took: the call's own frontier and hits are in the figure


def test_locate_approx_gives_the_occurrences(gpu, indexes):
    x, coll = indexes["genome"], collection("genome")
    patterns = [p for p in mixed_patterns("genome") if 3 <= len(p) <= 40][:40]
    loc = x.locator(max_len=40)
    hit_offsets, sp, count, mm, occ_offsets, ids, offs = loc.locate_approx(patterns, 1)
    same((hit_offsets, sp, count, mm), expected(coll, patterns, 1))
    assert np.array_equal(np.diff(occ_offsets), count)
    for j, p in enumerate(patterns):
        got = set()
        for h in range(int(hit_offsets[j]), int(hit_offsets[j + 1])):
            for o in range(int(occ_offsets[h]), int(occ_offsets[h + 1])):
                got.add((int(ids[o]), int(offs[o]), int(mm[h])))
        want = coll.hits(p, 1, want_occurrences=True)[4]
        assert got == want and len(got) == int(count[int(hit_offsets[j]): int(hit_offsets[j + 1])].sum()), j
    loc.free()


def test_on_a_poisoned_pool(bwtm):
    """The mixed-length case in a fresh process whose pool hands out blocks filled with 0xA5A5A5A5: every total, slot and node that is read
    was written by the kernels."""
    env = dict(os.environ, BWTM_POOL_POISON="0xA5A5A5A5")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "approx_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), "exit status %s\n%s%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
    assert got and int(got.group(1)) > 0 and int(got.group(2)) >= 256 * int(got.group(1)), out.stdout[-3000:]
