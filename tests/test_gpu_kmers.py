"""The k-mers of an index with their counts on the GPU (bwtm_kmers_*, Index.kmers).  Expected values are always computed from the reads the
test itself made -- a sliding window over the rows and np.unique on the codes (tests/kmer_inputs.py, checked against the oracle in
tests/test_kmers_host.py) -- never the library's own search."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from kmer_inputs import RECORD, SUPER, brute, brute_levels, decode, folded_histogram, genome_reads, iid_reads, peak_formula, text_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    return bwtm


def uploaded(gpu, oracle, rows):
    f = oracle.FMI.from_text(text_of(list(rows)))
    assert f.sequences == len(rows)
    return gpu.Index.upload(f.data, f.sequences, f.bases)


@pytest.fixture(scope="module")
def iid(gpu, oracle):
    rows = iid_reads()
    x = uploaded(gpu, oracle, rows)
    yield x, rows
    x.free()


@pytest.fixture(scope="module")
def genome(gpu, oracle):
    rows = genome_reads()
    x = uploaded(gpu, oracle, rows)
    yield x, rows
    x.free()


@functools.lru_cache(maxsize=None)
def iid_levels(k):
    return brute_levels(list(iid_reads()), k, 5)


@functools.lru_cache(maxsize=None)
def genome_expected(min_count):
    rows = list(genome_reads())
    return brute(rows, 12, 5, min_count), brute_levels(rows, 12, 5, min_count)


def same_kmers(km, want):
    """The whole result against (codes, counts, sp): exact, strictly ascending, the totals consistent."""
    codes, counts, sp = km.download()
    assert km.distinct == want[0].size == codes.size
    assert np.array_equal(codes, want[0]) and np.array_equal(counts, want[1]) and np.array_equal(sp, want[2])
    assert np.all(codes[1:] > codes[:-1]) and np.all(sp[1:] >= sp[:-1] + counts[:-1])
    assert km.total == int(want[1].sum())
    return codes, counts, sp


def check_collection(gpu, x, rows, k, skip=5, min_count=1):
    km = x.kmers(k, skip=skip, min_count=min_count)
    got = same_kmers(km, brute(list(rows), k, skip, min_count))
    assert np.array_equal(km.levels(), brute_levels(list(rows), k, skip, min_count))
    km.free()
    return got


@pytest.mark.parametrize("k", [1, 2, 4, 5, 12, 31, 32])
def test_iid_collection(gpu, iid, k):
    x, rows = iid
    km = x.kmers(k)
    codes, counts, sp = same_kmers(km, brute(list(rows), k, 5))
    levels = km.levels()
    assert np.array_equal(levels, iid_levels(32)[:k])
    assert levels[:5].tolist() == [4, 16, 64, 256, 1024][:k]                     # full workgroups first
    if k >= 12:
        assert levels[11] % 256 != 0 and 40000 < int(levels[11]) < 4 ** 12       # ragged ones later
    if k == 32:
        assert int(codes.max() >> np.uint64(62)) == 3 and len({int(c >> np.uint64(62)) for c in codes}) == 4      # the first symbol sits in bits 62..63
    assert np.array_equal(gpu.decode_kmers(codes, k, 5), decode(codes, k, 5))
    assert km.nbytes >= 24 * km.distinct
    km.free()


def test_k_beyond_32_is_refused(gpu, iid):
    x, rows = iid
    with pytest.raises(gpu.BwtmError) as e:
        x.kmers(40)
    assert "k = 40" in str(e.value)


@pytest.mark.parametrize("min_count", [0, 1, 2, 3, 50, 10 ** 6])
def test_genome_collection_and_thresholds(gpu, genome, min_count):
    x, rows = genome
    want, want_levels = genome_expected(min_count)
    km = x.kmers(12, min_count=min_count)
    codes, counts, sp = same_kmers(km, want)
    assert np.array_equal(km.levels(), want_levels)
    if min_count == 10 ** 6:
        assert km.distinct == 0 and km.total == 0 and not km.levels().any()
        assert all(a.size == 0 for a in km.download(0, 0))
    if min_count == 3:
        assert genome_expected(1)[0][0].size - km.distinct >= 1000 and km.distinct >= 2500
    for bins in (2, 16, 4096):
        assert np.array_equal(km.histogram(bins), folded_histogram(want[1], bins)), bins
    if min_count <= 1:
        assert int(counts.max()) >= 16                                           # bins = 16 folds an overflow in
    km.free()


def test_skip_symbol(gpu, oracle, iid):
    x, rows = iid
    # the sorted alphabet: $ A C G N T, so T is comp 5 and N comp 4
    sorted_rows = rows.copy()
    sorted_rows[rows == 4] = 5; sorted_rows[rows == 5] = 4
    y = uploaded(gpu, oracle, sorted_rows)
    a = check_collection(gpu, x, rows, 12)
    b = check_collection(gpu, y, sorted_rows, 12, skip=4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    letters_default, letters_sorted = np.frombuffer(b"$ACGTN", dtype=np.uint8), np.frombuffer(b"$ACGNT", dtype=np.uint8)
    assert np.array_equal(letters_default[gpu.decode_kmers(a[0], 12, 5)], letters_sorted[gpu.decode_kmers(b[0], 12, 4)])
    y.free()
    # without N every window counts, whatever the skip; a read of N alone, and Ns that leave no window of k, contribute nothing
    plain = genome_reads(13)[:300]
    z = uploaded(gpu, oracle, plain)
    codes, counts, sp = check_collection(gpu, z, plain, 9, skip=5)
    assert int(counts.sum()) == 300 * (40 - 9 + 1)
    z.free()
    with_n = [r for r in plain] + [np.full(17, 5, dtype=np.uint8), np.array([1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2, 3, 4], dtype=np.uint8)]
    w = uploaded(gpu, oracle, with_n)
    got = check_collection(gpu, w, with_n, 9, skip=5)
    assert np.array_equal(got[0], codes) and np.array_equal(got[1], counts)
    w.free()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_ranges_that_end_at_n_on_a_record_edge(gpu, oracle, delta):
    """n = 32 records exactly (128 reads of 31 symbols and their endmarkers), one less and one more: the last k-mer's range ends at n - 1."""
    rng = np.random.default_rng(40 + delta)
    rows = [rng.integers(1, 5, size=31).astype(np.uint8) for _ in range(128)]
    rows[5] = rng.integers(1, 5, size=31 + delta).astype(np.uint8)
    rows[77][-4:] = 4                                                            # TTTT$ : the last suffixes of the collection
    x = uploaded(gpu, oracle, rows)
    n = x.bases
    assert n == 32 * RECORD + delta
    for k in (1, 3, 4):
        codes, counts, sp = check_collection(gpu, x, rows, k)
        assert int(codes[-1]) == 4 ** k - 1 and int(sp[-1] + counts[-1]) == n
    x.free()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_ranges_that_end_at_n_on_a_super_edge(gpu, delta):
    """n = one super row exactly (2^20 reads of 31 symbols 1..4), one less and one more.  The counts of all 6-mers by np.bincount over the
    rows; the last one's range ends at n - 1."""
    import torch
    from bwt_merge_amd import synth
    m, k = SUPER // 32, 6
    rng = np.random.default_rng(50)
    rows = np.zeros((m, 32), dtype=np.uint8)
    rows[:, :31] = rng.integers(1, 5, size=(m, 31))
    lengths = np.full(m, 31, dtype=np.int64)
    lengths[9] += delta
    rows[9, 31] = 3
    rows[9, lengths[9]:] = 0
    dev = torch.device("cuda", 0)
    sym = synth.leaf_bwt(torch.as_tensor(rows, device=dev), torch.as_tensor(lengths, device=dev)).contiguous()
    torch.cuda.synchronize()
    x = gpu.Index.from_symbols_device(sym.data_ptr(), sym.numel())
    del sym
    n = x.bases
    assert n == SUPER + delta and n % RECORD == delta % RECORD
    windows = np.lib.stride_tricks.sliding_window_view(rows, k, axis=1)
    valid = windows.min(axis=2) > 0
    codes = np.zeros(windows.shape[:2], dtype=np.int64)
    for j in range(k):
        codes |= (windows[:, :, j].astype(np.int64) - 1) << (2 * (k - 1 - j))
    want = np.bincount(codes[valid], minlength=4 ** k)
    assert want.min() > 0
    km = x.kmers(k)
    got_codes, counts, sp = km.download()
    assert np.array_equal(got_codes, np.arange(4 ** k, dtype=np.uint64)) and np.array_equal(counts, want.astype(np.uint64))
    assert int(sp[-1] + counts[-1]) == n and np.all(sp[1:] >= sp[:-1] + counts[:-1]) and int(sp[0]) >= m
    assert km.total == int(valid.sum())
    km.free()
    x.free()


def test_every_form_of_an_index(gpu, oracle):
    from parts_inputs import host
    ra, rb = genome_reads(21)[:400], genome_reads(22)[:270]
    fa = oracle.FMI.from_text(text_of(list(ra)))
    A = gpu.Index.upload(fa.data, fa.sequences, fa.bases); B = uploaded(gpu, oracle, rb)
    both = np.concatenate([ra, rb])
    check_collection(gpu, A, ra, 10)
    M = gpu.merge(A, B)
    assert M.sequences == 670
    before = check_collection(gpu, M, both, 10, min_count=2)
    M.encode()
    after = check_collection(gpu, M, both, 10, min_count=2)
    assert all(np.array_equal(u, v) for u, v in zip(before, after))
    bld = gpu.Builder(128)
    bld.add(both)
    X = bld.finish()
    assert X.nbytes == 0                                                          # not encoded: records and super table only
    check_collection(gpu, X, both, 10)
    ha = host(gpu, fa)
    b0, b1, fp, before_counts = gpu.window_blocks(ha, 1000, 5000)
    Cs = (C.c_uint64 * 7)(*[int(v) for v in fa.C])
    out = gpu.capi.vp()
    data = fa.data                                        # a copy of the native bytes, alive over the call
    gpu.capi.check(gpu.capi.lib().bwtm_index_upload_window(data.ctypes.data + 64 * b0, 64 * (b1 - b0), fp, before_counts, int(fa.bases), int(fa.sequences), Cs, 0, C.byref(out)))
    W = gpu.Index(out)
    with pytest.raises(gpu.BwtmError) as e:
        W.kmers(10)
    assert "window" in str(e.value)
    for h in (W, X, M, A, B):
        h.free()


def test_consistency_with_find_and_locate(gpu, genome):
    x, rows = genome
    km = x.kmers(12)
    codes, counts, sp = km.download()
    picks = np.sort(np.random.default_rng(6).choice(codes.size, size=500, replace=False))
    patterns = gpu.decode_kmers(codes[picks], 12, 5)
    fsp, fep = x.find(list(patterns))
    assert np.array_equal(fsp, sp[picks]) and np.array_equal(fep, sp[picks] + counts[picks] - np.uint64(1))
    loc = x.locator(max_len=40)
    ten = picks[::50]
    hit_offsets, ids, offs = loc.locate_ranges(sp[ten], sp[ten] + counts[ten] - np.uint64(1))
    assert np.array_equal(np.diff(hit_offsets), counts[ten])
    for j, pick in enumerate(ten.tolist()):
        for h in range(int(hit_offsets[j]), int(hit_offsets[j + 1])):
            assert np.array_equal(rows[int(ids[h]), int(offs[h]): int(offs[h]) + 12], patterns[picks.tolist().index(pick)])
    loc.free()
    km.free()


def test_degenerate_inputs_and_argument_errors(gpu, oracle, iid):
    x, rows = iid
    lib, p_u64 = gpu.capi.lib(), gpu.capi.p_u64
    short = [r[:7] for r in rows[:50]]
    y = uploaded(gpu, oracle, short)
    km = y.kmers(8)
    assert km.distinct == 0 and km.total == 0 and km.levels().tolist()[7] == 0 and km.levels().tolist()[6] > 0 and km.nbytes == 0
    assert not km.histogram(4).any()
    km.free()
    check_collection(gpu, y, short, 7)
    y.free()
    one = [rows[3]]
    y = uploaded(gpu, oracle, one)
    for k in (1, 12, 32):
        check_collection(gpu, y, one, k)
    y.free()
    ragged = [rows[0], rows[1][:0], rows[2][:13], rows[3][:0], rows[4][:12], rows[5][:0]]
    y = uploaded(gpu, oracle, ragged)
    check_collection(gpu, y, ragged, 12)
    y.free()
    # slices
    km = x.kmers(12)
    codes, counts, sp = km.download()
    d = km.distinct
    for first, count in ((0, 0), (0, 1), (1, 1), (d - 1, 1), (d, 0), (1, d - 1), (1000, 257)):
        got = km.download(first, count)
        assert np.array_equal(got[0], codes[first: first + count]) and np.array_equal(got[1], counts[first: first + count]) and np.array_equal(got[2], sp[first: first + count])
    only = np.zeros(5, dtype=np.uint64)
    gpu.capi.check(lib.bwtm_kmers_download(km.h, 7, 5, None, only.ctypes.data_as(p_u64), None))       # any of the three may be NULL
    assert np.array_equal(only, counts[7:12])
    for first, count in ((d, 1), (0, d + 1), (d + 1, 0), (1, (1 << 64) - 1), ((1 << 64) - 1, 2)):
        with pytest.raises(gpu.BwtmError) as e:
            km.download(first, count)
        assert "lie beyond" in str(e.value)
    for bins in (0, 1):
        with pytest.raises(gpu.BwtmError) as e:
            km.histogram(bins)
        assert "bins" in str(e.value)
    km.free()
    with pytest.raises(gpu.BwtmError):
        km.download()
    for k, skip, what in ((0, 5, "k = 0"), (33, 5, "k = 33"), (12, 0, "skip = 0"), (12, 6, "skip = 6")):
        with pytest.raises(gpu.BwtmError) as e:
            x.kmers(k, skip=skip)
        assert what in str(e.value)
    assert np.array_equal(x.kmers(12).download()[0], codes)                      # the index still answers


def test_device_memory_stays_within_the_documented_bound(gpu, iid):
    x, rows = iid
    gpu.synchronize()
    gpu.trim()                                                                    # what the pool has cached so far is not this call's
    held = gpu.pool_stats()["held_bytes"]                                         # the indexes that are alive (this one and other fixtures'), nothing else
    gpu.device_bytes_peak(reset=True)
    km = x.kmers(12)
    peak = gpu.device_bytes_peak()
    levels = km.levels()
    assert int(levels.max()) > 40000
    assert held <= peak <= held + peak_formula(levels), (held, peak, peak_formula(levels))
    assert peak - held >= 24 * int(levels.max())                                  # the reset took: the call's own frontiers are in the figure
    assert 24 * km.distinct <= km.nbytes <= 24 * km.distinct * 17 // 16 + 65536
    km.free()


def test_on_a_poisoned_pool(bwtm):
    """The iid collection at k = 12 in a fresh process whose pool hands out blocks filled with 0xA5A5A5A5: every total, base, node and bin
    that is read was written by the kernels."""
    env = dict(os.environ, BWTM_POOL_POISON="0xA5A5A5A5")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kmers_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), "exit status %s\n%s%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
    assert got and int(got.group(1)) > 0 and int(got.group(2)) >= 256 * int(got.group(1)), out.stdout[-3000:]
