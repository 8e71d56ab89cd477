"""Matching statistics and maximal exact matches on the GPU (bwtm_matching_stats_batch, bwtm_mem_batch, Index.matching_stats, Index.mems,
Locator.locate_mems).  Expected values are always computed from the reads the test itself made -- the substrings of the rows and the
three-condition definition of a MEM (tests/mem_inputs.py, checked against the oracle in tests/test_mem_host.py) -- never the library's
own search."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from locate_inputs import FILL
from mem_inputs import FILL32, Brute, expected_mems, expected_stats, mems_raw, pack, same, special_patterns, stats_raw, varied_patterns
from overlap_inputs import overlap_reads, rows_of
from test_gpu_sequences import text_of, uploaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    return bwtm


def collection(gpu, oracle, m, seed):
    reads, lengths = overlap_reads(m, seed)
    rows = rows_of(reads, lengths)
    return uploaded(gpu, oracle, reads, lengths), rows, Brute(rows)


@pytest.fixture(scope="module")
def three_hundred(gpu, oracle):
    x, rows, brute = collection(gpu, oracle, 300, 1)
    yield x, rows, brute
    x.free()


@pytest.fixture(scope="module")
def thousand(gpu, oracle):
    x, rows, brute = collection(gpu, oracle, 1000, 2)
    yield x, rows, brute
    x.free()


def check_all_reads(gpu, x, rows, brute):
    """Every read as a pattern: each non-empty read is one MEM (0, len), and its statistics grow by one per symbol."""
    got = mems_raw(gpu, x, rows, 1)
    assert same(got, expected_mems(brute, rows, 1))
    assert np.diff(got[0].astype(np.int64)).tolist() == [1 if len(r) > 0 else 0 for r in rows] and any(len(r) == 0 for r in rows)
    assert not got[1].any() and got[2].tolist() == [len(r) for r in rows if len(r) > 0]
    stats = stats_raw(gpu, x, rows)
    assert same(stats, expected_stats(brute, rows))
    assert stats[0].tolist() == [i + 1 for r in rows for i in range(len(r))]


def check_varied_reads(gpu, x, rows, brute, seed):
    """Every read with one substitution, with a symbol before and behind it, and two reads joined (longer than any sequence)."""
    patterns = varied_patterns(rows, seed)
    assert max(len(p) for p in patterns) > 40 and sum(len(p) for p in patterns) % 64 != 0
    for min_length in (1, 12):
        assert same(mems_raw(gpu, x, patterns, min_length), expected_mems(brute, patterns, min_length)), min_length
    stats = stats_raw(gpu, x, patterns)
    assert same(stats, expected_stats(brute, patterns))
    assert int(stats[0].max()) == 40                                       # capped by the endmarker, in a pattern of up to 80 symbols


def test_all_reads_as_patterns(gpu, thousand):
    x, rows, brute = thousand
    assert x.bases > 100 * 128                                             # many 128-position records
    check_all_reads(gpu, x, rows, brute)


def test_reads_with_a_substitution_an_extension_and_joined(gpu, three_hundred):
    x, rows, brute = three_hundred
    check_varied_reads(gpu, x, rows, brute, 21)


@pytest.mark.parametrize("min_length", [1, 12, 40, 41])
def test_thresholds_on_the_edge_cases(gpu, three_hundred, min_length):
    """Empty patterns at the front, in the middle and at the end, one-symbol patterns, the largest symbol alone, the largest suffix of the
    collection, an absent symbol, a 100-symbol pattern that ends in a whole read -- in one batch with reads and their variations."""
    x, rows, brute = three_hundred
    special = special_patterns(rows, 22)
    patterns = special[:9] + varied_patterns(rows, 23)[::5] + special[9:-2] + rows[::3] + special[-2:]
    total = sum(len(p) for p in patterns)
    assert total % 64 != 0 and total > 8 * 64 and len(patterns[0]) == 0 and len(patterns[-1]) == 0
    want = expected_mems(brute, patterns, min_length)
    got = mems_raw(gpu, x, patterns, min_length)
    assert same(got, want)
    if min_length == 41:
        assert got[1].size == 0 and not got[0].any()
    if min_length == 40:
        assert got[1].size >= 2 and np.all(got[2] == 40)
    if min_length == 1:
        stats = stats_raw(gpu, x, patterns)
        assert same(stats, expected_stats(brute, patterns))
        text, offsets, _, _ = pack(gpu, patterns)
        k = patterns.index((5,) * 9)
        a, b = int(offsets[k]), int(offsets[k + 1])
        assert not stats[0][a:b].any() and not stats[1][a:b].any() and not stats[2][a:b].any() and got[0][k] == got[0][k + 1]
        k = patterns.index(special[8])                                      # the largest suffix: its range ends at the last position
        e = int(offsets[k + 1]) - 1
        assert int(stats[0][e]) == len(special[8]) and int(stats[1][e]) + int(stats[2][e]) == x.bases
        k = next(j for j, p in enumerate(patterns) if len(p) == 100)
        h = int(got[0][k + 1]) - 1
        assert (int(got[1][h]), int(got[2][h])) == (60, 40)                 # the whole read at the long pattern's end
        # the binding's own wrappers
        assert same(x.mems(patterns), want) and same(x.matching_stats(patterns), stats)
        assert same(x.mems(patterns, min_length=12), expected_mems(brute, patterns, 12))
        st = gpu.mem_stats()
        assert st["tasks"] == len(patterns) and st["batches"] == 1 and st["mems"] == int(want[0][-1]) > int(expected_mems(brute, patterns, 12)[0][-1])


def test_batches_give_the_same_bytes(gpu, three_hundred):
    x, rows, brute = three_hundred
    patterns = special_patterns(rows, 24) + varied_patterns(rows, 25)[::4] + rows[::2]
    want, want_stats = expected_mems(brute, patterns, 5), expected_stats(brute, patterns)
    whole, whole_stats = mems_raw(gpu, x, patterns, 5), stats_raw(gpu, x, patterns)
    small = {}
    try:
        for batch in (7, 64):
            gpu.tune("mem_batch", batch)
            small[batch] = (mems_raw(gpu, x, patterns, 5), stats_raw(gpu, x, patterns), gpu.mem_stats())
            x.mems(patterns, 5)
            after_mems = gpu.mem_stats()
            assert after_mems["batches"] == -(-len(patterns) // batch) and after_mems["tasks"] == len(patterns)                  # every batch once
    finally:
        gpu.tune("mem_batch", 0)
    assert same(whole, want) and same(whole_stats, want_stats)
    for batch in (7, 64):
        assert same(small[batch][0], want) and same(small[batch][1], want_stats), batch
        assert small[batch][2]["batches"] == -(-len(patterns) // batch)
    x.matching_stats(patterns)
    assert gpu.mem_stats()["batches"] == 1                                # the default is back


def test_capacity_and_null_outputs(gpu, three_hundred):
    x, rows, brute = three_hundred
    lib, p_u64, p_u32 = gpu.capi.lib(), gpu.capi.p_u64, gpu.capi.p_u32
    patterns = varied_patterns(rows, 26)[::6] + rows[:40]
    want = expected_mems(brute, patterns, 3)
    total = int(want[0][-1])
    assert total > 100
    text, offsets, tp, op = pack(gpu, patterns)
    # exact capacity: the guard slots behind hit_offsets[count] keep their fill
    assert same(mems_raw(gpu, x, patterns, 3, spare=0), want)
    # one slot short: BWTM_EINVAL, hit_offsets complete, nothing else written
    hit_offsets = np.zeros(len(patterns) + 1, dtype=np.uint64)
    begin = np.full(total, FILL32, dtype=np.uint32); length = np.full(total, FILL32, dtype=np.uint32)
    sp = np.full(total, FILL, dtype=np.uint64); count = np.full(total, FILL, dtype=np.uint64)
    rc = lib.bwtm_mem_batch(x.h, tp, op, len(patterns), 3, hit_offsets.ctypes.data_as(p_u64), begin.ctypes.data_as(p_u32), length.ctypes.data_as(p_u32),
                            sp.ctypes.data_as(p_u64), count.ctypes.data_as(p_u64), total - 1)
    assert rc == 1 and b"capacity" in lib.bwtm_last_error()
    assert np.array_equal(hit_offsets, want[0]) and np.all(begin == FILL32) and np.all(length == FILL32) and np.all(sp == FILL) and np.all(count == FILL)
    # each single NULL output
    for skip in range(4):
        outs = [np.full(total, FILL32, dtype=np.uint32), np.full(total, FILL32, dtype=np.uint32), np.full(total, FILL, dtype=np.uint64), np.full(total, FILL, dtype=np.uint64)]
        ptrs = [o.ctypes.data_as(p_u32 if o.dtype == np.uint32 else p_u64) for o in outs]
        ptrs[skip] = None
        gpu.capi.check(lib.bwtm_mem_batch(x.h, tp, op, len(patterns), 3, hit_offsets.ctypes.data_as(p_u64), ptrs[0], ptrs[1], ptrs[2], ptrs[3], total))
        assert all(np.array_equal(outs[j], want[1 + j]) for j in range(4) if j != skip), skip
    want_stats = expected_stats(brute, patterns)
    n = int(offsets[-1])
    for skip in range(3):
        outs = [np.full(n, FILL32, dtype=np.uint32), np.full(n, FILL, dtype=np.uint64), np.full(n, FILL, dtype=np.uint64)]
        ptrs = [o.ctypes.data_as(p_u32 if o.dtype == np.uint32 else p_u64) for o in outs]
        ptrs[skip] = None
        gpu.capi.check(lib.bwtm_matching_stats_batch(x.h, tp, op, len(patterns), ptrs[0], ptrs[1], ptrs[2]))
        assert all(np.array_equal(outs[j], want_stats[j]) for j in range(3) if j != skip), skip
    # offsets that do not start at 0: the entries lie at offsets[k] + i - offsets[0]
    shifted = offsets[5:].copy()
    lengths = np.full(int(shifted[-1] - shifted[0]), FILL32, dtype=np.uint32)
    gpu.capi.check(lib.bwtm_matching_stats_batch(x.h, tp, shifted.ctypes.data_as(p_u64), shifted.size - 1, lengths.ctypes.data_as(p_u32), None, None))
    assert np.array_equal(lengths, want_stats[0][int(shifted[0]):])
    # count == 0
    one = np.full(1, 99, dtype=np.uint64)
    gpu.capi.check(lib.bwtm_mem_batch(x.h, None, None, 0, 1, one.ctypes.data_as(p_u64), None, None, None, None, 0))
    assert one.tolist() == [0]
    assert x.mems([])[0].tolist() == [0] and x.mems([(), ()])[0].tolist() == [0, 0, 0] and x.matching_stats([()])[0].size == 0


def test_the_two_rounds_of_a_call_of_many_batches(gpu, three_hundred):
    """mem_batch = 7, so that the call searches every batch twice: the sizing call, a capacity one short, the exact capacity; the
    statistics of the filling call are those of the sizing call; a batch of seven empty patterns in the middle contributes nothing."""
    x, rows, brute = three_hundred
    lib, p_u64, p_u32 = gpu.capi.lib(), gpu.capi.p_u64, gpu.capi.p_u32
    reads = [r for r in rows if len(r) > 0]
    patterns = varied_patterns(rows, 32)[:14] + [()] * 7 + reads[:12]
    want = expected_mems(brute, patterns, 3)
    per = np.diff(want[0].astype(np.int64))
    total = int(want[0][-1])
    assert len(patterns) == 33 and not per[14:21].any() and per[:14].sum() > 14 and per[21:].sum() > 5
    assert np.all(want[0][14:22] == want[0][14])                                  # flat across the third batch
    text, offsets, tp, op = pack(gpu, patterns)

    def call(capacity):
        hit_offsets = np.full(len(patterns) + 1, FILL, dtype=np.uint64)
        outs = [np.full(total + 3, FILL32, dtype=np.uint32), np.full(total + 3, FILL32, dtype=np.uint32), np.full(total + 3, FILL, dtype=np.uint64), np.full(total + 3, FILL, dtype=np.uint64)]
        rc = lib.bwtm_mem_batch(x.h, tp, op, len(patterns), 3, hit_offsets.ctypes.data_as(p_u64), outs[0].ctypes.data_as(p_u32), outs[1].ctypes.data_as(p_u32),
                                outs[2].ctypes.data_as(p_u64), outs[3].ctypes.data_as(p_u64), capacity)
        return rc, hit_offsets, outs

    untouched = lambda outs: all(np.all(o == (FILL32 if o.dtype == np.uint32 else FILL)) for o in outs)
    try:
        gpu.tune("mem_batch", 7)
        rc, ho, outs = call(0)
        sized = gpu.mem_stats()
        assert rc == 0 and np.array_equal(ho, want[0]) and untouched(outs)
        rc, ho, outs = call(total - 1)
        assert rc == 1 and "bwtm_mem_batch: capacity %d is too small (%d MEMs)" % (total - 1, total) in lib.bwtm_last_error().decode()
        assert np.array_equal(ho, want[0]) and untouched(outs)
        rc, ho, outs = call(total)
        filled = gpu.mem_stats()
    finally:
        gpu.tune("mem_batch", 0)
    assert rc == 0 and same((ho,) + tuple(o[:total] for o in outs), want) and untouched([o[total:] for o in outs])
    assert filled == sized and sized["batches"] == 5 and sized["tasks"] == len(patterns) - 7 and sized["steps"] > 0 and sized["mems"] >= total    # a batch without text runs no task; the second round leaves no trace


def test_every_einval_names_its_offender(gpu, oracle, three_hundred):
    x, rows, brute = three_hundred
    lib, p_u64, p_u32, p_u8 = gpu.capi.lib(), gpu.capi.p_u64, gpu.capi.p_u32, gpu.capi.p_u8

    def mem_rc(text, offsets, min_length=1, index=x.h, hit=True):
        text = np.ascontiguousarray(text, dtype=np.uint8); offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        hit_offsets = np.zeros(offsets.size, dtype=np.uint64)
        rc = lib.bwtm_mem_batch(index, text.ctypes.data_as(p_u8), offsets.ctypes.data_as(p_u64), offsets.size - 1, min_length, hit_offsets.ctypes.data_as(p_u64) if hit else None,
                                None, None, None, None, 0)
        return rc, lib.bwtm_last_error().decode()

    def ms_rc(text, offsets, index=x.h, out=True):
        text = np.ascontiguousarray(text, dtype=np.uint8); offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lengths = np.zeros(max(int(offsets[-1]), 1), dtype=np.uint32)
        rc = lib.bwtm_matching_stats_batch(index, text.ctypes.data_as(p_u8), offsets.ctypes.data_as(p_u64), offsets.size - 1, lengths.ctypes.data_as(p_u32) if out else None, None, None)
        return rc, lib.bwtm_last_error().decode()

    for call, name in ((mem_rc, "bwtm_mem_batch"), (ms_rc, "bwtm_matching_stats_batch")):
        rc, msg = call([1, 2, 3, 4, 1, 0, 2, 3], [0, 3, 8])
        assert rc == 1 and name in msg and "pattern 1 holds the symbol 0 at offset 2" in msg, msg
        rc, msg = call([1, 2, 6, 4, 1, 1, 2, 3], [0, 3, 8])
        assert rc == 1 and name in msg and "pattern 0 holds the symbol 6 at offset 2" in msg, msg
        rc, msg = call([1, 2, 3, 4, 1, 1, 2, 3], [0, 5, 3, 8])
        assert rc == 1 and name in msg and "offsets must not decrease (pattern 1)" in msg, msg
        rc, msg = call([0, 2, 3, 4, 1, 1, 2, 3], [0, 3, 5, 4])                   # two faults: the offsets are looked at before any text is read through them
        assert rc == 1 and name in msg and "offsets must not decrease (pattern 2)" in msg, msg
        rc, msg = call(np.ones(65536 + 3, dtype=np.uint8), [0, 3, 65536 + 3])
        assert rc == 1 and name in msg and "pattern 1 has 65536 symbols" in msg, msg
        rc, msg = call([1, 2, 3], [0, 3], index=None)
        assert rc == 1 and name in msg and "null argument" in msg, msg
    rc, msg = mem_rc([1, 2, 3], [0, 3], hit=False)
    assert rc == 1 and "bwtm_mem_batch: null argument" in msg, msg
    rc, msg = ms_rc([1, 2, 3], [0, 3], out=False)
    assert rc == 1 and "bwtm_matching_stats_batch: null argument" in msg, msg
    rc, msg = mem_rc([1, 2, 3], [0, 3], min_length=0)
    assert rc == 1 and "min_length must be at least 1" in msg, msg
    with pytest.raises(gpu.BwtmError) as e:
        x.mems([(1, 2, 3)], min_length=0)
    assert "min_length" in str(e.value)
    # a window of an index only serves the partitioned merge
    from parts_inputs import host
    reads, lengths = overlap_reads(1000, 2)
    f = oracle.FMI.from_text(text_of(reads, lengths))
    b0, b1, fp, before_counts = gpu.window_blocks(host(gpu, f), 1000, 5000)
    Cs = (C.c_uint64 * 7)(*[int(v) for v in f.C])
    out = gpu.capi.vp()
    data = f.data                                                        # a copy of the native bytes, alive over the call
    gpu.capi.check(lib.bwtm_index_upload_window(data.ctypes.data + 64 * b0, 64 * (b1 - b0), fp, before_counts, int(f.bases), int(f.sequences), Cs, 0, C.byref(out)))
    w = gpu.Index(out)
    for call, name in ((mem_rc, "bwtm_mem_batch"), (ms_rc, "bwtm_matching_stats_batch")):
        rc, msg = call([1, 2, 3], [0, 3], index=w.h)
        assert rc == 1 and name in msg and "a window of an index" in msg, msg
    w.free()
    # a 65 535-symbol pattern is accepted, and the index still answers
    longest = np.tile(np.array([1, 2], dtype=np.uint8), 32768)[:65535]
    lengths = x.matching_stats([longest])[0]
    assert lengths.size == 65535 and int(lengths.max()) <= 40 and int(lengths[:40].min()) >= 1
    assert same(mems_raw(gpu, x, rows[:50], 1), expected_mems(brute, rows[:50], 1))


def test_consistent_with_find(gpu, thousand):
    """A secondary check against the library's own exact search: for every entry with l > 0, Index.find of the matched substring returns
    the same range and Index.find of the one-longer substring an empty one."""
    x, rows, brute = thousand
    patterns = varied_patterns(rows, 27)[::9] + special_patterns(rows, 28)
    lengths, sp, count = x.matching_stats(patterns)
    matched, longer, at = [], [], []
    t = 0
    for p in patterns:
        for i in range(len(p)):
            l = int(lengths[t])
            if l > 0:
                matched.append(np.array(p[i + 1 - l:i + 1], dtype=np.uint8)); at.append(t)
                if l < i + 1:
                    longer.append(np.array(p[i - l:i + 1], dtype=np.uint8))
            t += 1
    assert len(matched) > 3000 and len(longer) > 300
    fsp, fep = x.find(matched)
    at = np.array(at)
    assert np.array_equal(fsp, sp[at]) and np.array_equal(fep, sp[at] + count[at] - np.uint64(1))
    lsp, lep = x.find(longer)
    assert np.all(lsp > lep)
    st = gpu.mem_stats()
    assert st["tasks"] == lengths.size and st["steps"] >= int(lengths.astype(np.int64).sum()) and st["mems"] == 0


def test_stats_count_tasks_and_steps(gpu, three_hundred):
    x, rows, brute = three_hundred
    """A search takes one step per symbol it consumes: l(e) of them when it stops at the pattern's begin, one more when it stops at an
    empty range.  The statistics search every end; the MEM search goes from the last end downwards and stops behind the first search
    that reaches the pattern's begin.  Expected from the brute force's lengths."""
    patterns = varied_patterns(rows, 29)[::3] + special_patterns(rows, 31)
    x.matching_stats(patterns)
    st = gpu.mem_stats()
    total = sum(len(p) for p in patterns)
    want = sum(l + (1 if l < e else 0) for p in patterns for e, l in enumerate(brute.lengths(p), start=1))
    assert st["tasks"] == total and st["batches"] == 1 and st["mems"] == 0
    assert st["steps"] == want >= sum(l for p in patterns for l in brute.lengths(p))
    want_mems = 0
    for p in patterns:
        lengths = brute.lengths(p)
        for e in range(len(p), 0, -1):
            want_mems += lengths[e - 1] + (1 if lengths[e - 1] < e else 0)
            if lengths[e - 1] == e:
                break
    x.mems(patterns, 1)
    st = gpu.mem_stats()
    assert st["tasks"] == len(patterns) and st["steps"] == want_mems < want and st["mems"] == int(expected_mems(brute, patterns, 1)[0][-1])


def test_locate_mems(gpu, three_hundred):
    x, rows, brute = three_hundred
    loc = x.locator(max_len=40)
    patterns = varied_patterns(rows, 30)[::11]
    hit_offsets, begin, length, sp, count, occ_offsets, ids, offs = loc.locate_mems(patterns, 8)
    assert same((hit_offsets, begin, length, sp, count), expected_mems(brute, patterns, 8)) and begin.size > 30
    assert np.array_equal(np.diff(occ_offsets.astype(np.int64)), count.astype(np.int64))
    for k, p in enumerate(patterns):
        for h in range(int(hit_offsets[k]), int(hit_offsets[k + 1])):
            w = tuple(p[int(begin[h]): int(begin[h]) + int(length[h])])
            occ = sorted((int(ids[j]), int(offs[j])) for j in range(int(occ_offsets[h]), int(occ_offsets[h + 1])))
            assert occ == sorted((t, o) for t, r in enumerate(rows) for o in range(len(r) - len(w) + 1) if r[o:o + len(w)] == w), (k, h)
    capped = loc.locate_mems(patterns, 8, max_hits=1)
    assert np.array_equal(np.diff(capped[5].astype(np.int64)), np.minimum(count.astype(np.int64), 1))
    loc.free()


def test_on_a_poisoned_pool(bwtm):
    """The all-reads case and the varied-reads case in a fresh process whose pool hands out blocks filled with 0xA5A5A5A5: every length,
    flag, slot, count and output that is read was written by the kernels."""
    env = dict(os.environ, BWTM_POOL_POISON="0xA5A5A5A5")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mem_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), "exit status %s\n%s%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
    assert got and int(got.group(1)) > 0 and int(got.group(2)) >= 256 * int(got.group(1)), out.stdout[-3000:]
