"""From BWT positions to (sequence id, offset) on the GPU (bwtm_locator_*, bwtm_locate_batch, bwtm_locate_ranges, Index.locator).
Expected values are always computed from the reads the test itself made -- the sorted suffixes of the rows and a naive substring
table (tests/locate_inputs.py) -- never the library's own find or extraction."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from locate_inputs import FILL, all_suffixes, locate_raw, naive_hits, pairs, ranges_raw, substring_table, suffix_order
from test_gpu_sequences import ragged_reads, text_of, uploaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    return bwtm


def cut_patterns(reads, lengths, count, seed, longest=6):
    """`count` patterns of 1 .. longest symbols cut from reads at random places."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        j = int(rng.integers(0, reads.shape[0]))
        if lengths[j] == 0:
            continue
        k = int(rng.integers(1, min(longest, int(lengths[j])) + 1))
        o = int(rng.integers(0, int(lengths[j]) - k + 1))
        out.append(reads[j, o: o + k].copy())
    return out


def absent_pattern(table, rng):
    while True:
        p = tuple(int(v) for v in rng.integers(1, 6, size=6))
        if p not in table:
            return np.array(p, dtype=np.uint8)


def check_patterns(gpu, loc, table, lengths, patterns, max_hits=0):
    """locate_patterns against the naive table: the same hit sets; returns (hit_offsets, ids, offsets)."""
    hit_offsets, ids, offs = loc.locate_patterns(patterns, max_hits)
    assert hit_offsets.size == len(patterns) + 1 and int(hit_offsets[-1]) == ids.size == offs.size
    for k, pat in enumerate(patterns):
        got = pairs(ids[int(hit_offsets[k]): int(hit_offsets[k + 1])], offs[int(hit_offsets[k]): int(hit_offsets[k + 1])])
        want = naive_hits(table, lengths, pat)
        if max_hits == 0:
            assert sorted(got) == want, (k, list(pat))
        else:
            assert len(got) == min(len(want), max_hits) and len(set(got)) == len(got) and set(got) <= set(want), (k, list(pat))
    return hit_offsets, ids, offs


def test_every_position_locates_to_its_own_suffix(gpu, oracle):
    """The 300 ragged reads (empty reads, ten exact duplicates, one read that is a substring of another): all 4 680 positions, as positions
    and as the single range [0, n - 1]: the same answers, exactly the set {(j, o) : 0 <= o <= len_j}, each position its own suffix."""
    n = 300
    reads, lengths = ragged_reads(oracle, n, 7101)
    x = uploaded(gpu, oracle, reads, lengths)
    bases = x.bases
    assert bases == 4680
    loc = x.locator()
    assert loc.nbytes == 8 * n
    ids, offs = locate_raw(gpu, loc, np.arange(bases))
    hit_offsets, rids, roffs = ranges_raw(gpu, loc, [0], [bases - 1])
    assert hit_offsets.tolist() == [0, bases]
    assert np.array_equal(ids, rids) and np.array_equal(offs, roffs)
    got = pairs(ids, offs)
    assert len(set(got)) == bases and set(got) == all_suffixes(lengths)
    assert np.array_equal(ids[:n], np.arange(n)) and np.array_equal(offs[:n], lengths)       # position p < m: the endmarker suffix of sequence p
    want_ids, want_offs = suffix_order(reads, lengths)
    assert np.array_equal(ids, want_ids) and np.array_equal(offs, want_offs)
    ids2, offs2 = loc.locate(np.arange(bases))                                              # the binding's own wrapper
    assert np.array_equal(ids2, ids) and np.array_equal(offs2, offs)
    loc.free()
    x.free()


@pytest.fixture(scope="module")
def thousand(gpu, oracle):
    reads, lengths = ragged_reads(oracle, 1000, 7102)
    x = uploaded(gpu, oracle, reads, lengths)
    loc = x.locator()
    yield x, loc, reads, lengths, substring_table(reads, lengths, 7), suffix_order(reads, lengths)
    loc.free()
    x.free()


def test_patterns_against_a_naive_search(gpu, thousand):
    """200 patterns of 1 .. 6 symbols cut from reads, an absent one, the empty one and one that ends in the endmarker."""
    x, loc, reads, lengths, table, order = thousand
    patterns = cut_patterns(reads, lengths, 200, 41)
    patterns.append(absent_pattern(table, np.random.default_rng(42)))
    patterns.append(np.zeros(0, dtype=np.uint8))
    j = next(k for k in range(1000) if lengths[k] >= 3)
    patterns.append(np.concatenate([reads[j, int(lengths[j]) - 3: int(lengths[j])], np.zeros(1, dtype=np.uint8)]))     # reads that END in these three symbols
    hit_offsets, ids, offs = check_patterns(gpu, loc, table, lengths, patterns)
    assert hit_offsets[201] == hit_offsets[200]                                              # the absent pattern
    assert hit_offsets[202] - hit_offsets[201] == x.bases                                    # the empty pattern: every suffix
    assert hit_offsets[203] > hit_offsets[202]
    sp, ep = x.find(patterns)
    raw = ranges_raw(gpu, loc, sp, ep)
    assert np.array_equal(raw[0], hit_offsets) and np.array_equal(raw[1], ids) and np.array_equal(raw[2], offs)
    for k in range(len(patterns)):                                                           # inside a range: ascending BWT position
        if sp[k] <= ep[k]:
            a, b = locate_raw(gpu, loc, np.arange(int(sp[k]), int(ep[k]) + 1))
            assert np.array_equal(a, ids[int(hit_offsets[k]): int(hit_offsets[k + 1])]) and np.array_equal(b, offs[int(hit_offsets[k]): int(hit_offsets[k + 1])]), k


@pytest.mark.parametrize("count", [1, 3, 4, 5, 63, 64, 65, 257])
def test_counts_that_leave_partial_quads_waves_and_blocks(gpu, thousand, count):
    x, loc, reads, lengths, table, (want_ids, want_offs) = thousand
    positions = np.random.default_rng(count).integers(0, x.bases, size=count).astype(np.uint64)
    if count >= 3:
        positions[-1] = positions[0]                                                         # unsorted, with repeats
        positions[count // 2] = x.bases - 1
    ids, offs = locate_raw(gpu, loc, positions)
    assert np.array_equal(ids, want_ids[positions]) and np.array_equal(offs, want_offs[positions])
    for first in (0, x.bases - count, 1000 - count // 2):                                     # the last one straddles the endmarker suffixes' end
        hit_offsets, ids, offs = ranges_raw(gpu, loc, [first], [first + count - 1])
        assert hit_offsets.tolist() == [0, count]
        assert np.array_equal(ids, want_ids[first: first + count]) and np.array_equal(offs, want_offs[first: first + count])


def test_batches_give_the_same_result(gpu, oracle):
    """locate_batch = 64 for the build and for both locate calls: a range that spans many batches, many ranges inside one batch, empty
    ranges between them; equal to the default batch's results and to the sorted suffixes."""
    reads, lengths = ragged_reads(oracle, 1000, 7103)
    x = uploaded(gpu, oracle, reads, lengths)
    bases = x.bases
    want_ids, want_offs = suffix_order(reads, lengths)
    rng = np.random.default_rng(5)
    positions = rng.integers(0, bases, size=777).astype(np.uint64)
    sp = [0, 5, 900, 7, 1000, 1003, 1010, 1011, 2000, 1, bases - 70, 3000]
    ep = [bases - 1, 4, 1099, 7, 1002, 1009, 1010, 1010, 2100, 0, bases - 1, 3062]
    loc = x.locator()
    whole = locate_raw(gpu, loc, positions)
    ranged = ranges_raw(gpu, loc, sp, ep)
    loc.free()
    gpu.tune("locate_batch", 64)
    try:
        loc = x.locator()
        small = locate_raw(gpu, loc, positions)
        small_ranged = ranges_raw(gpu, loc, sp, ep)
        loc.free()
    finally:
        gpu.tune("locate_batch", 0)
    assert np.array_equal(small[0], whole[0]) and np.array_equal(small[1], whole[1])
    assert np.array_equal(small[0], want_ids[positions]) and np.array_equal(small[1], want_offs[positions])
    for got in (ranged, small_ranged):
        kept = [max(0, e - s + 1) for s, e in zip(sp, ep)]
        assert got[0].tolist() == [0] + list(np.cumsum(kept))
        for r in range(len(sp)):
            a, b = int(got[0][r]), int(got[0][r + 1])
            assert np.array_equal(got[1][a:b], want_ids[sp[r]: sp[r] + kept[r]]) and np.array_equal(got[2][a:b], want_offs[sp[r]: sp[r] + kept[r]]), r
    x.free()


@pytest.mark.parametrize("max_hits", [1, 2, 1 << 20])
def test_max_hits_keeps_a_prefix_of_every_range(gpu, thousand, max_hits):
    x, loc, reads, lengths, table, order = thousand
    patterns = cut_patterns(reads, lengths, 60, 43, longest=3) + [np.zeros(0, dtype=np.uint8), absent_pattern(table, np.random.default_rng(44))]
    full = check_patterns(gpu, loc, table, lengths, patterns)
    cut = check_patterns(gpu, loc, table, lengths, patterns, max_hits)
    assert max(np.diff(full[0]).tolist()) > 2                                                # the small limits do cut
    for k in range(len(patterns)):
        a, b = int(cut[0][k]), int(cut[0][k + 1])
        fa, fb = int(full[0][k]), int(full[0][k + 1])
        assert b - a == min(fb - fa, max_hits)
        assert np.array_equal(cut[1][a:b], full[1][fa: fa + b - a]) and np.array_equal(cut[2][a:b], full[2][fa: fa + b - a]), k
    if max_hits == 1 << 20:
        assert np.array_equal(cut[0], full[0])


def test_every_form_of_an_index(gpu, oracle):
    """An uploaded native stream, the result of a merge (ids >= a.sequences are b's reads; a pattern planted in both sides comes back from
    both), a builder's result (records only) -- and a window, refused."""
    from parts_inputs import host
    ra, la = ragged_reads(oracle, 400, 7104)
    rb, lb = ragged_reads(oracle, 270, 7105)
    plant = np.array([1, 4, 2, 2, 3, 1, 4, 4, 3, 2, 1, 3], dtype=np.uint8)
    assert la[49] == 40 and lb[59] == 40
    ra[49, 3:15] = plant
    rb[59, 11:23] = plant
    fa = oracle.FMI.from_text(text_of(ra, la))
    A = gpu.Index.upload(fa.data, fa.sequences, fa.bases); B = uploaded(gpu, oracle, rb, lb)
    both, both_len = np.concatenate([ra, rb]), np.concatenate([la, lb])
    patterns = cut_patterns(both, both_len, 80, 45) + [plant, np.zeros(0, dtype=np.uint8)]

    def whole_check(index, reads, lengths):
        loc = index.locator()
        table = substring_table(reads, lengths, 12)
        out = check_patterns(gpu, loc, table, lengths, patterns)       # a pattern cut from the other side may be absent here: no hits
        ids, offs = loc.locate(np.arange(index.bases))
        want = suffix_order(reads, lengths)
        assert np.array_equal(ids, want[0]) and np.array_equal(offs, want[1])
        loc.free()
        return out

    whole_check(A, ra, la)
    M = gpu.merge(A, B)
    assert M.sequences == 670
    whole_check(M, both, both_len)
    loc = M.locator()
    hit_offsets, ids, offs = loc.locate_patterns([plant])
    assert sorted(pairs(ids, offs)) == [(49, 3), (400 + 59, 11)]
    loc.free()
    bld = gpu.Builder(128)
    bld.add(both, both_len)
    X = bld.finish()
    assert X.nbytes == 0                                                  # not encoded: records and super table only
    whole_check(X, both, both_len)
    # a window of an index answers no queries of its own
    ha = host(gpu, fa)
    b0, b1, fp, before = gpu.window_blocks(ha, 1000, 5000)
    Cs = (C.c_uint64 * 7)(*[int(v) for v in fa.C])
    out = gpu.capi.vp()
    data = fa.data                                        # a copy of the native bytes, alive over the call
    gpu.capi.check(gpu.capi.lib().bwtm_index_upload_window(data.ctypes.data + 64 * b0, 64 * (b1 - b0), fp, before, int(fa.bases), int(fa.sequences), Cs, 0, C.byref(out)))
    W = gpu.Index(out)
    with pytest.raises(gpu.BwtmError) as e:
        W.locator()
    assert "window" in str(e.value)
    for h in (W, X, M, A, B):
        h.free()


def test_record_and_super_row_boundaries(gpu):
    """One index of more than 2^25 positions (340 000 iid reads of 100 bp): the walks cross records and read the super table's second row.
    4 096 24-mers cut at random (id, offset): each is found where it was cut, and every hit spells its pattern in the regenerated read."""
    import torch
    from bwt_merge_amd import synth
    n, L, seed, K = 340_000, 100, 7106, 24
    assert n * (L + 1) > (1 << 25)
    sym = synth.leaf_bwt(synth.generate_reads(seed, 0, n, L, device=torch.device("cuda", 0))).contiguous()
    torch.cuda.synchronize()
    x = gpu.Index.from_symbols_device(sym.data_ptr(), sym.numel())
    del sym
    assert x.sequences == n and x.bases == n * (L + 1)
    loc = x.locator(max_len=L)
    assert loc.nbytes == 8 * n
    rng = np.random.default_rng(13)
    cut_ids = rng.integers(0, n, size=4096)
    cut_offs = rng.integers(0, L - K + 1, size=4096)
    rows = synth.generate_reads(seed, cut_ids, None, L).numpy()
    patterns = [rows[k, int(cut_offs[k]): int(cut_offs[k]) + K] for k in range(4096)]
    hit_offsets, ids, offs = loc.locate_patterns(patterns)
    assert np.all(np.diff(hit_offsets.astype(np.int64)) >= 1)
    which = np.repeat(np.arange(4096), np.diff(hit_offsets.astype(np.int64)))
    hit_rows = synth.generate_reads(seed, ids.astype(np.int64), None, L).numpy()
    assert np.all(offs <= L - K)
    spelled = hit_rows[np.arange(ids.size)[:, None], offs.astype(np.int64)[:, None] + np.arange(K)[None, :]]
    assert np.array_equal(spelled, np.stack(patterns)[which])
    got = set(zip(which.tolist(), ids.tolist(), offs.tolist()))
    assert all((k, int(cut_ids[k]), int(cut_offs[k])) in got for k in range(4096))
    ends = np.array([n - 1, 0, n // 2], dtype=np.uint64)                                      # endmarker suffixes: (p, L)
    a, b = loc.locate(ends)
    assert np.array_equal(a, ends) and b.tolist() == [L, L, L]
    loc.free()
    x.free()


def test_errors_without_hangs(gpu, oracle):
    n, L = 500, 100
    reads = oracle.generate_reads(7107, n, L).reshape(n, L + 1)[:, :L].copy()
    lengths = np.full(n, L, dtype=np.uint32)
    x = uploaded(gpu, oracle, reads, lengths)
    bases = x.bases
    lib, p_u64 = gpu.capi.lib(), gpu.capi.p_u64
    with pytest.raises(gpu.BwtmError) as e:                               # every read is too long: the first offending sequence is the first one
        x.locator(max_len=50)
    assert re.search(r"sequence 0 is longer than max_len = 50", str(e.value)), str(e.value)
    with pytest.raises(gpu.BwtmError) as e:
        x.locator(max_len=(1 << 24) + 1)
    assert "2^24" in str(e.value)
    loc = x.locator(max_len=L)                                            # exactly max_len symbols is allowed
    want_ids, want_offs = suffix_order(reads, lengths)
    with pytest.raises(gpu.BwtmError) as e:
        loc.locate(np.array([3, bases, 4]))
    assert "position %d out of range" % bases in str(e.value)
    with pytest.raises(gpu.BwtmError) as e:
        loc.locate_ranges([0, 10], [5, bases])
    assert "position %d" % bases in str(e.value)
    hit_offsets, ids, offs = loc.locate_ranges([0, 10, 7], [5, bases - 1, 3])      # ep = bases - 1 is the last position; sp > ep is empty, whatever ep is
    assert hit_offsets.tolist() == [0, 6, bases - 4, bases - 4]
    sp, ep = np.array([100, 200], dtype=np.uint64), np.array([149, 249], dtype=np.uint64)
    hit_offsets = np.zeros(3, dtype=np.uint64)
    ids = np.full(100, FILL, dtype=np.uint64); offs = np.full(100, FILL, dtype=np.uint64)
    rc = lib.bwtm_locate_ranges(loc.h, sp.ctypes.data_as(p_u64), ep.ctypes.data_as(p_u64), 2, 0, hit_offsets.ctypes.data_as(p_u64), ids.ctypes.data_as(p_u64),
                                offs.ctypes.data_as(p_u64), 99)          # one slot short
    assert rc == 1 and b"capacity" in lib.bwtm_last_error()
    assert hit_offsets.tolist() == [0, 50, 100] and np.all(ids == FILL) and np.all(offs == FILL)
    gpu.capi.check(lib.bwtm_locate_batch(loc.h, None, 0, None, None))   # count == 0
    a, b = loc.locate(np.zeros(0, dtype=np.uint64))
    assert a.size == 0 and b.size == 0
    hit_offsets = np.full(1, 99, dtype=np.uint64)
    gpu.capi.check(lib.bwtm_locate_ranges(loc.h, None, None, 0, 0, hit_offsets.ctypes.data_as(p_u64), None, None, 0))
    assert hit_offsets.tolist() == [0]
    hit_offsets, ids, offs = loc.locate_ranges([], [])
    assert hit_offsets.tolist() == [0] and ids.size == 0
    ids, offs = loc.locate(np.arange(bases))                              # the locator still answers
    assert np.array_equal(ids, want_ids) and np.array_equal(offs, want_offs)
    loc.free()
    loc.free()
    with pytest.raises(gpu.BwtmError):
        loc.locate(np.array([0]))
    off, text = x.sequences(first=0, count=3)                             # the index still answers
    assert np.array_equal(text.reshape(3, L), reads[:3])
    sp, ep = x.find([reads[7, 10:40]])
    assert sp[0] <= ep[0]
    x.free()


def test_on_a_poisoned_pool(bwtm):
    """The bijection and the batching case in a fresh process whose pool hands out blocks filled with 0xA5A5A5A5: every entry of the table and
    of a batch's outputs that is read was written by the kernels (a table that was never filled does not pass its check)."""
    env = dict(os.environ, BWTM_POOL_POISON="0xA5A5A5A5")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "locate_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), "exit status %s\n%s%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
    assert got and int(got.group(1)) > 0 and int(got.group(2)) >= 256 * int(got.group(1)), out.stdout[-3000:]
