"""Sequences by id on the GPU (bwtm_sequences_extract, Index.sequences): what comes out of an index is the reads that went in.
Expected values are always the input reads themselves (hand-made, the oracle's generator or the tensor generator), never the
library's own inverse: sequence k of an index built from reads 0, 1, ... is read k, and merge(a, b) holds a's reads, then b's."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

LENGTH_CYCLE = (0, 1, 7, 8, 9, 15, 16, 17, 33, 40)         # around the 8-byte words of the text: empty, one byte, one word -1 / +0 / +1, ...
WIDTH = 40
SPARE = 64


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    return bwtm


def ragged_reads(oracle, n, seed):
    """n rows of WIDTH comp values with lengths cycling through LENGTH_CYCLE (zero behind each read's end); rows 20..29 repeat rows
    10..19 (exact duplicates, the same lengths) and row 38 (33 symbols) is a substring of row 39 (40 symbols)."""
    reads = oracle.generate_reads(seed, n, WIDTH).reshape(n, WIDTH + 1)[:, :WIDTH].copy()
    lengths = np.array([LENGTH_CYCLE[k % len(LENGTH_CYCLE)] for k in range(n)], dtype=np.uint32)
    reads[20:30] = reads[10:20]
    reads[38, :33] = reads[39, 5:38]
    for k in range(n):
        reads[k, lengths[k]:] = 0
    return reads, lengths


def text_of(reads, lengths):
    """Rows -> the oracle's text: every read followed by an endmarker."""
    parts = []
    for k, row in enumerate(reads):
        parts.append(row[: int(lengths[k])]); parts.append(np.zeros(1, dtype=np.uint8))
    return np.concatenate(parts)


def uploaded(gpu, oracle, reads, lengths):
    f = oracle.FMI.from_text(text_of(reads, lengths))
    assert f.sequences == reads.shape[0]
    return gpu.Index.upload(f.data, f.sequences, f.bases)


def expected(reads, lengths, ids):
    """(offsets, text) of the reads with the given ids, straight from the input rows."""
    lens = np.asarray(lengths, dtype=np.uint64)[ids]
    offsets = np.zeros(len(ids) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    text = np.concatenate([reads[j, : int(lengths[j])] for j in ids] + [np.zeros(0, dtype=np.uint8)])
    return offsets, text


def extract_raw(gpu, index, ids=None, first=0, count=None, max_len=0):
    """The two calls Index.sequences makes, through the same prototypes, with the caller's text prefilled with 0xEE and SPARE bytes
    longer than needed: the bytes behind offsets[count] must still hold 0xEE afterwards."""
    lib = gpu.capi.lib()
    ip = None
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        ip, count = ids.ctypes.data_as(gpu.capi.p_u64), ids.size
    offsets = np.full(count + 1, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    gpu.capi.check(lib.bwtm_sequences_extract(index.h, ip, first, count, max_len, offsets.ctypes.data_as(gpu.capi.p_u64), None, 0))
    sized = offsets.copy()
    total = int(offsets[-1])
    text = np.full(total + SPARE, 0xEE, dtype=np.uint8)
    gpu.capi.check(lib.bwtm_sequences_extract(index.h, ip, first, count, max_len, offsets.ctypes.data_as(gpu.capi.p_u64), text.ctypes.data_as(gpu.capi.p_u8), text.size))
    assert np.array_equal(offsets, sized), "the sizing call and the extracting call disagree about the offsets"
    assert np.all(text[total:] == 0xEE), "bytes behind offsets[count] were written"
    return offsets, text[:total]


def check_ids(gpu, index, reads, lengths, ids=None, first=0, count=None):
    want = expected(reads, lengths, list(ids) if ids is not None else list(range(first, first + count)))
    got = extract_raw(gpu, index, ids, first, count)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    got = index.sequences(ids=ids, first=first, count=count)             # the binding's own wrapper
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_ragged_lengths_around_store_boundaries(gpu, oracle):
    """300 reads whose lengths put every slot boundary at every offset inside an 8-byte word; all ids in one call; every sequence and offset."""
    n = 300
    reads, lengths = ragged_reads(oracle, n, 7101)
    assert np.array_equal(reads[25], reads[15]) and lengths[38] == 33 and lengths[39] == 40
    x = uploaded(gpu, oracle, reads, lengths)
    offsets, text = extract_raw(gpu, x, first=0, count=n)
    want_off, want_text = expected(reads, lengths, list(range(n)))
    assert np.array_equal(offsets, want_off)
    for k in range(n):
        assert np.array_equal(text[int(offsets[k]): int(offsets[k + 1])], reads[k, : int(lengths[k])]), k
    assert np.array_equal(text, want_text)
    assert {int(o) % 8 for o in offsets} == set(range(8))               # the slots do start at every offset of a word
    assert int(x.sequences) == n and x.sequences + 1 == n + 1            # the count is still the plain number it was
    x.free()


@pytest.fixture(scope="module")
def thousand(gpu, oracle):
    reads, lengths = ragged_reads(oracle, 1000, 7102)
    x = uploaded(gpu, oracle, reads, lengths)
    yield x, reads, lengths
    x.free()


@pytest.mark.parametrize("count", [1, 3, 4, 5, 63, 64, 65, 257])
def test_counts_that_leave_partial_quads_waves_and_blocks(gpu, thousand, count):
    x, reads, lengths = thousand
    check_ids(gpu, x, reads, lengths, first=1000 - count - 3, count=count)          # a range that ends close to the last sequence
    check_ids(gpu, x, reads, lengths, first=0, count=count)
    rng = np.random.default_rng(count)
    ids = rng.integers(0, 1000, size=count)
    if count >= 3:
        ids[-1] = ids[0]                                                             # unsorted, with repeats
        ids[count // 2] = 999
    check_ids(gpu, x, reads, lengths, ids=ids)


def test_batches_give_the_same_result(gpu, oracle):
    """extract_batch = 64: sixteen batches, the last one partial; offsets and text equal those of the default batch size and the reads."""
    reads, lengths = ragged_reads(oracle, 1000, 7103)
    x = uploaded(gpu, oracle, reads, lengths)
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 1000, size=777)
    whole = extract_raw(gpu, x, first=0, count=1000)
    listed = extract_raw(gpu, x, ids=ids)
    gpu.tune("extract_batch", 64)
    try:
        small = extract_raw(gpu, x, first=0, count=1000)
        small_listed = extract_raw(gpu, x, ids=ids)
    finally:
        gpu.tune("extract_batch", 0)
    for got, base, want in ((small, whole, expected(reads, lengths, list(range(1000)))), (small_listed, listed, expected(reads, lengths, list(ids)))):
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    x.free()


def test_every_form_of_an_index(gpu, oracle):
    """An uploaded native stream, the result of a merge (a's reads, then b's), a builder's result (records only) -- and a window, refused."""
    from parts_inputs import host
    ra, la = ragged_reads(oracle, 400, 7104)
    rb, lb = ragged_reads(oracle, 270, 7105)
    fa = oracle.FMI.from_text(text_of(ra, la))
    A = gpu.Index.upload(fa.data, fa.sequences, fa.bases); B = uploaded(gpu, oracle, rb, lb)
    check_ids(gpu, A, ra, la, first=0, count=400)
    M = gpu.merge(A, B)
    both, both_len = np.concatenate([ra, rb]), np.concatenate([la, lb])
    assert M.sequences == 670
    check_ids(gpu, M, both, both_len, first=0, count=670)
    off, text = M.sequences(first=395, count=10)                          # across the seam: ids below a.sequences are a's, the rest b's
    for k in range(10):
        j = 395 + k
        want = ra[j, : int(la[j])] if j < 400 else rb[j - 400, : int(lb[j - 400])]
        assert np.array_equal(text[int(off[k]): int(off[k + 1])], want), j
    bld = gpu.Builder(128)
    bld.add(both, both_len)
    X = bld.finish()
    assert X.nbytes == 0                                                  # not encoded: records and super table only
    check_ids(gpu, X, both, both_len, first=0, count=670)
    check_ids(gpu, X, both, both_len, ids=np.array([669, 0, 401, 401, 38, 39]))
    # a window of an index answers no queries of its own
    ha = host(gpu, fa)
    b0, b1, fp, before = gpu.window_blocks(ha, 1000, 5000)
    Cs = (C.c_uint64 * 7)(*[int(v) for v in fa.C])
    out = gpu.capi.vp()
    data = fa.data                                        # a copy of the native bytes, alive over the call
    gpu.capi.check(gpu.capi.lib().bwtm_index_upload_window(data.ctypes.data + 64 * b0, 64 * (b1 - b0), fp, before, int(fa.bases), int(fa.sequences), Cs, 0, C.byref(out)))
    W = gpu.Index(out)
    with pytest.raises(gpu.BwtmError):
        W.sequences(first=0, count=4)
    for h in (W, X, M, A, B):
        h.free()


def test_record_and_super_row_boundaries(gpu):
    """One index of more than 2^25 positions (340 000 iid reads of 100 bp): walks cross records and read the super table's second row."""
    import torch
    from bwt_merge_amd import synth
    n, L, seed = 340_000, 100, 7106
    assert n * (L + 1) > (1 << 25)
    sym = synth.leaf_bwt(synth.generate_reads(seed, 0, n, L, device=torch.device("cuda", 0))).contiguous()
    torch.cuda.synchronize()
    x = gpu.Index.from_symbols_device(sym.data_ptr(), sym.numel())
    del sym
    assert x.sequences == n and x.bases == n * (L + 1)
    ids = np.concatenate([np.random.default_rng(12).integers(0, n, size=4096), np.arange(4096)])
    want = synth.generate_reads(seed, ids, None, L).numpy()
    offsets, text = x.sequences(ids=ids, max_len=L)
    assert np.array_equal(offsets, np.arange(ids.size + 1, dtype=np.uint64) * np.uint64(L))
    assert np.array_equal(text.reshape(ids.size, L), want)
    x.free()


def test_errors_without_hangs(gpu, oracle):
    n, L = 500, 100
    reads = oracle.generate_reads(7107, n, L).reshape(n, L + 1)[:, :L].copy()
    lengths = np.full(n, L, dtype=np.uint32)
    x = uploaded(gpu, oracle, reads, lengths)
    lib, p_u64, p_u8 = gpu.capi.lib(), gpu.capi.p_u64, gpu.capi.p_u8
    with pytest.raises(gpu.BwtmError) as e:                               # every read is too long: the first offending id is the first one asked for
        x.sequences(first=10, count=300, max_len=50)
    assert re.search(r"sequence 10 is longer than max_len = 50", str(e.value)), str(e.value)
    with pytest.raises(gpu.BwtmError) as e:
        x.sequences(ids=np.array([7, 499, 3, 3]), max_len=99)
    assert re.search(r"sequence 7 is longer", str(e.value)), str(e.value)
    with pytest.raises(gpu.BwtmError) as e:                               # an id equal to `sequences`
        x.sequences(ids=np.array([1, n, 2]))
    assert "sequence %d out of range" % n in str(e.value)
    with pytest.raises(gpu.BwtmError):
        x.sequences(first=n - 1, count=2)
    with pytest.raises(gpu.BwtmError):
        x.sequences(first=0, count=4, max_len=(1 << 24) + 1)
    offsets = np.zeros(5, dtype=np.uint64)
    text = np.full(4 * L, 0xEE, dtype=np.uint8)
    rc = lib.bwtm_sequences_extract(x.h, None, 0, 4, 0, offsets.ctypes.data_as(p_u64), text.ctypes.data_as(p_u8), 4 * L - 1)       # one byte short
    assert rc == 1 and b"capacity" in lib.bwtm_last_error()
    offsets = np.full(1, 99, dtype=np.uint64)
    gpu.capi.check(lib.bwtm_sequences_extract(x.h, None, 0, 0, 0, offsets.ctypes.data_as(p_u64), None, 0))
    assert offsets.tolist() == [0]
    off, text = x.sequences(first=0, count=0)
    assert off.tolist() == [0] and text.size == 0
    check_ids(gpu, x, reads, lengths, first=0, count=n)                   # the index still answers
    off, text = x.sequences(first=0, count=3, max_len=L)                  # exactly max_len symbols is allowed
    assert np.array_equal(text.reshape(3, L), reads[:3])
    x.free()


def test_on_a_poisoned_pool(bwtm):
    """The ragged and the batching case in a fresh process whose pool hands out blocks filled with 0xA5A5A5A5: every byte of a batch's
    lengths and text that the host reads was written by the kernels."""
    env = dict(os.environ, BWTM_POOL_POISON="0xA5A5A5A5")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sequences_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), "exit status %s\n%s%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
    assert got and int(got.group(1)) > 0 and int(got.group(2)) >= 256 * int(got.group(1)), out.stdout[-3000:]
