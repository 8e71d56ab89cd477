"""K-mer error correction of reads on the GPU (bwtm_corrector_*, bwtm_correct_batch, bwtm_correct_sequences; Kmers.corrector).  Every
result is compared exactly -- text, status and edits -- with the brute force of tests/correct_inputs.py, which restates the rule of
include/bwtm.h over a Counter of windows and never uses the library (tests/test_correct_host.py checks it on its own)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from correct_inputs import (CLEAN, CORRECTED, FAILED, HAND_K, HAND_T, SHORT, as_bytes, correct_all, hand_made, long_reads, solid_count, table_of)
from kmer_inputs import genome_reads, text_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GUARD = 4096


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    yield bwtm
    bwtm.tune("correct_batch", 0)


def uploaded(gpu, oracle, rows):
    f = oracle.FMI.from_text(text_of(list(rows)))
    assert f.sequences == len(rows)
    return gpu.Index.upload(f.data, f.sequences, f.bases)


@pytest.fixture(scope="module")
def genome(gpu, oracle):
    rows = list(genome_reads())
    x = uploaded(gpu, oracle, rows)
    yield x, rows
    x.free()


@pytest.fixture(scope="module")
def longs(gpu, oracle):
    rows = long_reads()[0]
    x = uploaded(gpu, oracle, rows)
    yield x, rows
    x.free()


@functools.lru_cache(maxsize=None)
def genome_table():
    return table_of(list(genome_reads()), 12)


@functools.lru_cache(maxsize=None)
def genome_want(t, rounds):
    return correct_all(list(genome_reads()), 12, t, rounds, table=genome_table())


@functools.lru_cache(maxsize=None)
def long_want(k, skip=5):
    rows = long_reads()[0]
    if skip == 4:
        rows = [sorted_alphabet(r) for r in rows]
    table = table_of(rows, k, skip)
    return correct_all(rows, k, 3, 10, skip, table), solid_count(table, 3)


def sorted_alphabet(row):
    """$ A C G N T: T is comp 5 and N comp 4."""
    return np.array([0, 1, 2, 3, 5, 4], dtype=np.uint8)[row]


def split(offsets, text):
    return [bytes(bytearray(text[int(offsets[j]): int(offsets[j + 1])].tolist())) for j in range(offsets.size - 1)]


def same(got, want, picks=None):
    """(offsets, text, status, edits) of correct_sequences against (texts, status, edits) of the brute force, for the reads `picks`."""
    offsets, text, status, edits = got
    texts, wstatus, wedits = want
    picks = list(range(len(texts))) if picks is None else list(picks)
    assert offsets.size == len(picks) + 1 and offsets[0] == 0
    assert np.array_equal(status, wstatus[picks]), np.flatnonzero(status != wstatus[picks])[:10]
    assert np.array_equal(edits, wedits[picks]), np.flatnonzero(edits != wedits[picks])[:10]
    if text is not None:
        assert split(offsets, text) == [texts[j] for j in picks]
    else:
        assert np.array_equal(np.diff(offsets), [len(texts[j]) for j in picks])


@pytest.mark.parametrize("t", [1, 2, 3, 50, 10 ** 6])
def test_genome_reads_and_thresholds(gpu, genome, t):
    x, rows = genome
    km = x.kmers(12)
    cor = km.corrector(t)
    km.free()
    assert cor.k == 12 and cor.solid == solid_count(genome_table(), t)
    want = genome_want(t, 10)
    got = cor.correct_sequences(x)
    same(got, want)
    if t == 10 ** 6:
        assert cor.solid == 0 and got[2].tolist() == [FAILED] * len(rows) and not got[3].any()
    if t == 3:
        assert np.bincount(got[2], minlength=4).tolist() == [1339, 654, 7, 0]
    stats = gpu.correct_stats()
    assert stats["batches"] == 1 and stats["max_edits"] == int(want[2].max()) and stats["lookups"] >= len(rows) * (40 - 12 + 1)
    cor.free()


@pytest.mark.parametrize("rounds", [0, 1, 10])
def test_rounds(gpu, genome, rounds):
    x, rows = genome
    cor = x.kmers(12).corrector(3)
    want = genome_want(3, rounds)
    same(cor.correct_sequences(x, max_rounds=rounds), want)
    if rounds == 0:
        assert CORRECTED not in want[1] and FAILED in want[1]
    if rounds == 1:
        assert int(want[2].max()) == 1
    cor.free()


@pytest.mark.parametrize("k", [1, 2, 21, 31, 32])
def test_long_reads(gpu, longs, k):
    x, rows = longs
    km = x.kmers(k)
    cor = km.corrector(3)
    want, solid = long_want(k)
    assert cor.solid == solid and cor.k == k
    got = cor.correct_sequences(x, max_len=300)
    same(got, want)
    if k >= 21:
        assert all(c > 0 for c in np.bincount(got[2], minlength=4).tolist())
    if k == 21:
        assert int(got[3].max()) >= 5 and max(len(r) for r in rows) - k + 1 > 256
    # the batch form on the same reads: the same bytes
    texts, status, edits = cor.correct(rows)
    assert [as_bytes(t) for t in texts] == want[0] and np.array_equal(status, want[1]) and np.array_equal(edits, want[2])
    cor.free(); km.free()


def test_hand_made_reads(gpu, oracle):
    collection, cases = hand_made()
    x = uploaded(gpu, oracle, collection)
    km = x.kmers(HAND_K)
    cor = km.corrector(HAND_T)
    assert cor.solid == solid_count(table_of(collection, HAND_K), HAND_T)
    for rounds in sorted({c[2] for c in cases}):
        mine = [c for c in cases if c[2] == rounds]
        texts, status, edits = cor.correct([c[1] for c in mine], max_rounds=rounds)
        for (name, read, _, wstatus, wtext, wedits), text, st, ed in zip(mine, texts, status, edits):
            assert (as_bytes(text), int(st), int(ed)) == (wtext, wstatus, wedits), name
    assert {c[3] for c in cases} == {CLEAN, CORRECTED, FAILED, SHORT} and any(len(c[1]) == 0 for c in cases)
    for h in (cor, km, x):
        h.free()


def test_ids_and_ranges(gpu, genome):
    x, rows = genome
    cor = x.kmers(12).corrector(3)
    want = genome_want(3, 10)
    rng = np.random.default_rng(3)
    ids = rng.integers(0, len(rows), size=333)
    ids[10:13] = ids[9]
    same(cor.correct_sequences(x, ids=ids), want, ids.tolist())
    for first, count in ((0, 1), (1999, 1), (17, 257), (1000, None), (5, 0)):
        picks = range(first, len(rows) if count is None else first + count)
        same(cor.correct_sequences(x, first=first, count=count), want, picks)
    # the status call: the same status and edits, the offsets of Index.sequences, no text
    got = cor.correct_sequences(x, first=100, count=700, text=False)
    assert got[1] is None
    same(got, want, range(100, 800))
    assert np.array_equal(got[0], x.sequences(first=100, count=700)[0])
    cor.free()


def test_many_batches_give_the_same_bytes(gpu, genome):
    x, rows = genome
    cor = x.kmers(12).corrector(3)
    want = genome_want(3, 10)
    one = cor.correct_sequences(x, first=0, count=300)
    one_stats = gpu.correct_stats()
    gpu.tune("correct_batch", 7)
    try:
        many = cor.correct_sequences(x, first=0, count=300)
        stats = gpu.correct_stats()
        assert stats["batches"] == (300 + 6) // 7 and one_stats["batches"] == 1
        assert {k: v for k, v in stats.items() if k != "batches"} == {k: v for k, v in one_stats.items() if k != "batches"}
        texts, status, edits = cor.correct(rows[:100])
        assert gpu.correct_stats()["batches"] == (100 + 6) // 7
        status_only = cor.correct_sequences(x, first=0, count=300, text=False)
    finally:
        gpu.tune("correct_batch", 0)
    same(many, want, range(300))
    assert all(np.array_equal(a, b) for a, b in zip(one, many))
    same(status_only, want, range(300))
    assert [as_bytes(t) for t in texts] == want[0][:100] and np.array_equal(status, want[1][:100]) and np.array_equal(edits, want[2][:100])
    # two runs: equal bytes
    again = cor.correct_sequences(x, first=0, count=300)
    assert all(np.array_equal(a, b) for a, b in zip(one, again))
    cor.free()


def test_sorted_alphabet(gpu, oracle):
    rows = [sorted_alphabet(r) for r in long_reads()[0]]
    x = uploaded(gpu, oracle, rows)
    cor = x.kmers(21, skip=4).corrector(3, skip=4)
    want, solid = long_want(21, 4)
    assert cor.solid == solid == long_want(21)[1]
    got = cor.correct_sequences(x, max_len=300)
    same(got, want)
    default = long_want(21)[0]
    assert np.array_equal(want[1], default[1]) and np.array_equal(want[2], default[2])
    assert [as_bytes(sorted_alphabet(np.frombuffer(t, dtype=np.uint8))) for t in default[0]] == want[0]
    cor.free(); x.free()


def bound_of_a_call(nreads, nbytes):
    """include/bwtm.h: 17/8 T + 27 (B + 1) + 2^16."""
    return 17 * nbytes // 8 + 27 * (nreads + 1) + (1 << 16)


def test_handle_and_device_memory_stay_within_the_documented_bounds(gpu, longs):
    x, rows = longs
    km = x.kmers(21)
    gpu.synchronize(); gpu.trim()
    cor = km.corrector(3)
    km.free()
    S = cor.solid
    D = min(42, 24, max(1, int(np.ceil(np.log2(S)))))
    exact = 8 * S + 8 * (2 ** D + 1)
    assert S > 1000 and exact <= cor.nbytes <= exact * 17 // 16 + 512
    gpu.synchronize(); gpu.trim()
    held = gpu.pool_stats()["held_bytes"]
    gpu.device_bytes_peak(reset=True)
    got = cor.correct_sequences(x, max_len=300)
    peak = gpu.device_bytes_peak()
    T = int(got[0][-1])
    assert held <= peak <= held + bound_of_a_call(len(rows), T), (held, peak, T)
    assert peak - held >= 2 * T                                                    # the reset took: the text and its working copy are in the figure
    same(got, long_want(21)[0])
    cor.free()


def test_outputs_stay_inside_their_buffers(gpu, genome):
    x, rows = genome
    lib, capi = gpu.capi.lib(), gpu.capi
    cor = x.kmers(12).corrector(3)
    want = genome_want(3, 10)
    n, T = 500, 500 * 40
    bufs = {name: np.full(nbytes + 2 * GUARD, 0xA5, dtype=np.uint8) for name, nbytes in (("offsets", 8 * (n + 1)), ("text", T + 100), ("status", n), ("edits", 4 * n))}

    def ptr(name, ctype):
        return C.cast(C.c_void_p(bufs[name].ctypes.data + GUARD), C.POINTER(ctype))

    capi.check(lib.bwtm_correct_sequences(cor.h, x.h, None, 200, n, 0, 10, ptr("offsets", C.c_uint64), ptr("text", C.c_uint8), T + 100 + GUARD, ptr("status", C.c_uint8),
                                          ptr("edits", C.c_uint32)))
    for name, written in (("offsets", 8 * (n + 1)), ("text", T), ("status", n), ("edits", 4 * n)):
        assert np.all(bufs[name][:GUARD] == 0xA5) and np.all(bufs[name][GUARD + written:] == 0xA5), name
    inner = {name: b[GUARD: b.size - GUARD] for name, b in bufs.items()}
    same((inner["offsets"].view(np.uint64), inner["text"][:T], inner["status"], inner["edits"].view(np.uint32)), want, range(200, 200 + n))
    # a capacity that is too small: refused before anything is written, the offsets included
    for name in bufs:
        bufs[name][:] = 0xA5
    rc = lib.bwtm_correct_sequences(cor.h, x.h, None, 200, n, 0, 10, ptr("offsets", C.c_uint64), ptr("text", C.c_uint8), T - 1, ptr("status", C.c_uint8), ptr("edits", C.c_uint32))
    assert rc != 0 and "capacity %d is too small" % (T - 1) in lib.bwtm_last_error().decode()
    assert all(np.all(b == 0xA5) for b in bufs.values())
    # the batch form: out_text has the input's layout, any output may be NULL
    reads = rows[:50]
    text = np.concatenate(reads); offsets = (np.arange(51) * 40).astype(np.uint64)
    out = np.full(text.size + 2 * GUARD, 0xA5, dtype=np.uint8)
    capi.check(lib.bwtm_correct_batch(cor.h, text.ctypes.data_as(capi.p_u8), offsets.ctypes.data_as(capi.p_u64), 50, 10,
                                      C.cast(C.c_void_p(out.ctypes.data + GUARD), capi.p_u8), None, None))
    assert np.all(out[:GUARD] == 0xA5) and np.all(out[GUARD + text.size:] == 0xA5)
    assert split(offsets, out[GUARD: GUARD + text.size]) == want[0][:50]
    capi.check(lib.bwtm_correct_sequences(cor.h, x.h, None, 0, 50, 0, 10, None, None, 0, None, None))      # every output NULL
    cor.free()


def test_argument_errors_name_the_offender(gpu, oracle, genome):
    x, rows = genome
    lib, capi = gpu.capi.lib(), gpu.capi
    km = x.kmers(12)
    for skip in (0, 6):
        with pytest.raises(gpu.BwtmError) as e:
            km.corrector(3, skip=skip)
        assert "skip = %d" % skip in str(e.value)
    out = capi.vp()
    assert lib.bwtm_corrector_create(None, 5, 3, C.byref(out)) != 0 and "null argument" in lib.bwtm_last_error().decode()
    assert lib.bwtm_corrector_create(km.h, 5, 3, None) != 0 and "null argument" in lib.bwtm_last_error().decode()
    cor = km.corrector(0)                                                         # a threshold of 0 is taken as 1
    assert cor.solid == km.distinct
    cor.free()
    cor = km.corrector(3)
    km.free()
    for call in (lambda: cor.correct([rows[0]], max_rounds=65536), lambda: cor.correct_sequences(x, max_rounds=65536, text=False)):
        with pytest.raises(gpu.BwtmError) as e:
            call()
        assert "max_rounds = 65536" in str(e.value)
    assert cor.correct([rows[0]], max_rounds=65535)[1].tolist() == [int(genome_want(3, 10)[1][0])]
    text = np.concatenate(rows[:3]); st = np.zeros(3, dtype=np.uint8)
    offsets = np.array([0, 40, 30, 120], dtype=np.uint64)
    args = (text.ctypes.data_as(capi.p_u8), offsets.ctypes.data_as(capi.p_u64), 3, 10, None, st.ctypes.data_as(capi.p_u8), None)
    assert lib.bwtm_correct_batch(cor.h, *args) != 0 and "offsets must not decrease (pattern 1)" in lib.bwtm_last_error().decode()
    spoiled = text.copy(); spoiled[0] = 0                                         # two faults: the offsets are looked at before any text is read through them
    later = np.array([0, 40, 90, 80], dtype=np.uint64)
    assert lib.bwtm_correct_batch(cor.h, spoiled.ctypes.data_as(capi.p_u8), later.ctypes.data_as(capi.p_u64), *args[2:]) != 0
    assert "offsets must not decrease (pattern 2)" in lib.bwtm_last_error().decode()
    assert lib.bwtm_correct_batch(None, *args) != 0 and "null argument" in lib.bwtm_last_error().decode()
    assert lib.bwtm_correct_batch(cor.h, args[0], None, *args[2:]) != 0 and "null argument" in lib.bwtm_last_error().decode()
    offsets[2] = 80
    assert lib.bwtm_correct_batch(cor.h, None, *args[1:]) != 0 and "null pattern text" in lib.bwtm_last_error().decode()
    for bad in (0, 6):
        spoiled = [rows[0], rows[1].copy()]
        spoiled[1][7] = bad
        with pytest.raises(gpu.BwtmError) as e:
            cor.correct(spoiled)
        assert "pattern 1 holds the symbol %d at offset 7" % bad in str(e.value)
    with pytest.raises(gpu.BwtmError) as e:
        cor.correct_sequences(x, ids=np.array([5, 2000, 7], dtype=np.uint64))
    assert "sequence 2000 out of range" in str(e.value)
    with pytest.raises(gpu.BwtmError) as e:
        cor.correct_sequences(x, first=1990, count=11)
    assert "out of range" in str(e.value)
    with pytest.raises(gpu.BwtmError) as e:
        cor.correct_sequences(x, first=3, count=5, max_len=39, text=False)
    assert "sequence 3 is longer than max_len = 39" in str(e.value)
    assert lib.bwtm_correct_sequences(cor.h, None, None, 0, 1, 0, 10, None, None, 0, None, None) != 0 and "null argument" in lib.bwtm_last_error().decode()
    assert lib.bwtm_correct_sequences(None, x.h, None, 0, 1, 0, 10, None, None, 0, None, None) != 0 and "null argument" in lib.bwtm_last_error().decode()
    assert lib.bwtm_correct_stats(None) != 0 and "null argument" in lib.bwtm_last_error().decode()
    # a window of an index
    from parts_inputs import host
    f = oracle.FMI.from_text(text_of(rows[:400]))
    b0, b1, fp, before_counts = gpu.window_blocks(host(gpu, f), 1000, 5000)
    Cs = (C.c_uint64 * 7)(*[int(v) for v in f.C])
    out = capi.vp()
    data = f.data                                        # a copy of the native bytes, alive over the call
    capi.check(lib.bwtm_index_upload_window(data.ctypes.data + 64 * b0, 64 * (b1 - b0), fp, before_counts, int(f.bases), int(f.sequences), Cs, 0, C.byref(out)))
    W = gpu.Index(out)
    with pytest.raises(gpu.BwtmError) as e:
        cor.correct_sequences(W, first=0, count=1, text=False)
    assert "window" in str(e.value)
    W.free()
    # a corrector and an index of different contexts
    other = gpu.Context(0)
    other.make_current()
    try:
        y = uploaded(gpu, oracle, rows[:50])
    finally:
        gpu.make_default_current()
    with pytest.raises(gpu.BwtmError) as e:
        cor.correct_sequences(y, text=False)
    assert "different contexts" in str(e.value)
    y.free()
    other.destroy()
    same(cor.correct_sequences(x, first=0, count=20), genome_want(3, 10), range(20))     # the corrector still answers
    cor.free()
    with pytest.raises(gpu.BwtmError):
        cor.correct([rows[0]])


def test_on_a_merged_index(gpu, oracle):
    ra, rb = list(genome_reads(21)[:400]), list(genome_reads(22)[:270])
    A, B = uploaded(gpu, oracle, ra), uploaded(gpu, oracle, rb)
    M = gpu.merge(A, B)
    U = uploaded(gpu, oracle, ra + rb)
    assert M.sequences == U.sequences == 670
    got = []
    for x in (M, U):
        km = x.kmers(10, min_count=2)
        cor = km.corrector(2)
        km.free()
        got.append((cor.solid,) + cor.correct_sequences(x))
        cor.free()
    assert got[0][0] == got[1][0] and all(np.array_equal(u, v) for u, v in zip(got[0][1:], got[1][1:]))
    same(got[0][1:], correct_all(ra + rb, 10, 2, 10))
    for h in (M, U, A, B):
        h.free()


@pytest.mark.parametrize("word", ["0x00000000", "0xA5A5A5A5"])
def test_on_a_poisoned_pool(bwtm, word):
    """The long reads and the hand-made ones in a fresh process whose pool hands out blocks filled with `word`: every flag, slot, directory
    entry, offset, status and edit count that is read was written by the kernels."""
    env = dict(os.environ, BWTM_POOL_POISON=word)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "correct_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), "exit status %s\n%s%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
    assert got and int(got.group(1)) > 0 and int(got.group(2)) >= 256 * int(got.group(1)), out.stdout[-3000:]
