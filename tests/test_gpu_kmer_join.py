"""The k-mers of two indexes side by side on the GPU (bwtm_kmer_join_*, Index.kmer_join).  Expected values are always computed from the reads
the test itself made -- sliding windows over the rows of both collections and np.searchsorted (tests/kmer_join_inputs.py, checked against the
oracle in tests/test_kmer_join_host.py) -- never the library's own search; the merge identity is checked against bwtm_kmers_create on the
merged index, whose own tests do the same.
The pair of genome collections tops out near 2 * 10^4 nodes per level (3 000 positions and the error k-mers of 2 000 reads), so the cases
over k run on a second pair as well, the iid collection of the k-mer tests against one of another seed: its level 12 is the ragged frontier
of more than 40 000 nodes."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from kmer_inputs import RECORD, brute, decode, genome_reads, iid_reads, text_of
from kmer_join_inputs import brute_pair, brute_pair_levels, classes, pair_reads, peak_formula

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
EINVAL = 1                                                                       # BWTM_EINVAL (include/bwtm.h)


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    return bwtm


def uploaded(gpu, oracle, rows):
    f = oracle.FMI.from_text(text_of(list(rows)))
    assert f.sequences == len(rows)
    return gpu.Index.upload(f.data, f.sequences, f.bases)


def rows_of(which):
    return pair_reads() if which == "genome" else (iid_reads(), iid_reads(17))


@pytest.fixture(scope="module")
def pairs(gpu, oracle):
    made = {}
    for which in ("genome", "iid"):
        ra, rb = rows_of(which)
        made[which] = (uploaded(gpu, oracle, ra), uploaded(gpu, oracle, rb), ra, rb)
    yield made
    for a, b, _, _ in made.values():
        a.free(); b.free()


@pytest.fixture(scope="module")
def genome(pairs):
    return pairs["genome"]


@functools.lru_cache(maxsize=None)
def expected(which, k):
    """The union of a pair at k."""
    ra, rb = rows_of(which)
    return brute_pair(ra, rb, k, 5)


@functools.lru_cache(maxsize=None)
def union_levels(which):
    """Without upper bounds level t does not depend on k."""
    ra, rb = rows_of(which)
    return brute_pair_levels(ra, rb, 32, 5)


def same_join(kj, want):
    """The whole result against (codes, count_a, count_b, sp_a, sp_b): exact, ascending, the summary consistent."""
    got = kj.download()
    assert kj.distinct == want[0].size == got[0].size
    for g, w, name in zip(got, want, ("codes", "count_a", "count_b", "sp_a", "sp_b")):
        assert np.array_equal(g, w), name
    codes, ca, cb, spa, spb = got
    assert np.all(codes[1:] > codes[:-1]) and np.all(spa[1:] >= spa[:-1] + ca[:-1]) and np.all(spb[1:] >= spb[:-1] + cb[:-1])
    assert list(kj.summary().values()) == classes(want)
    assert kj.nbytes >= 40 * kj.distinct and (kj.distinct > 0 or kj.nbytes == 0)
    return got


def check_pair(gpu, A, B, rows_a, rows_b, k, skip=5, **bounds):
    kj = A.kmer_join(B, k, skip=skip, **bounds)
    got = same_join(kj, brute_pair(rows_a, rows_b, k, skip, **bounds))
    assert np.array_equal(kj.levels(), brute_pair_levels(rows_a, rows_b, k, skip, **bounds))
    kj.free()
    return got


@pytest.mark.parametrize("k", [1, 2, 5, 12, 31, 32])
@pytest.mark.parametrize("which", ["genome", "iid"])
def test_k_and_frontier_shape(gpu, pairs, which, k):
    A, B, ra, rb = pairs[which]
    kj = A.kmer_join(B, k)
    codes, ca, cb, spa, spb = same_join(kj, expected(which, k))
    levels = kj.levels()
    assert np.array_equal(levels, union_levels(which)[:k])
    assert levels[:5].tolist() == [4, 16, 64, 256, 1024][:k]                     # full workgroups first
    if k >= 12 and which == "iid":
        assert levels[11] % 256 != 0 and 40000 < int(levels[11]) < 4 ** 12       # ragged ones later
    if k >= 12 and which == "genome":                                           # the three classes, each well filled
        assert int((ca == 0).sum()) >= 500 and int((cb == 0).sum()) >= 500 and int(((ca > 0) & (cb > 0)).sum()) >= 500
    if k == 32:
        assert int(codes.max() >> np.uint64(62)) == 3 and len({int(c >> np.uint64(62)) for c in codes}) == 4      # the first symbol sits in bits 62..63
    kj.free()


FILTERS = {
    "shared": dict(min_a=1, min_b=1),
    "private_a": dict(max_b=0),
    "private_b": dict(max_a=0),
    "min_sum_2": dict(min_sum=2),
    "min_sum_3": dict(min_sum=3),
    "min_sum_50": dict(min_sum=50),
    "min_sum_1e6": dict(min_sum=10 ** 6),
    "fresh_in_b": dict(max_a=0, min_b=2),
    "exactly_3_in_a": dict(min_a=3, max_a=3),
    "solid_in_a_weak_in_b": dict(min_a=5, min_b=1, max_b=2, min_sum=7),
}


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_filters(gpu, genome, name):
    A, B, ra, rb = genome
    bounds = FILTERS[name]
    kj = A.kmer_join(B, 12, **bounds)
    want = brute_pair(ra, rb, 12, 5, **bounds)
    codes, ca, cb, spa, spb = same_join(kj, want)
    levels = kj.levels()
    assert np.array_equal(levels, brute_pair_levels(ra, rb, 12, 5, **bounds))
    lower = {key: v for key, v in bounds.items() if key.startswith("min")}
    if len(lower) != len(bounds):                                                # upper bounds act at the last level only
        free = A.kmer_join(B, 12, **lower)
        assert np.array_equal(levels[:11], free.levels()[:11]) and int(levels[11]) < int(free.levels()[11])
        assert int(levels[10]) > 0
        free.free()
    if name == "min_sum_1e6":
        assert kj.distinct == 0 and kj.nbytes == 0 and not levels.any() and not any(kj.summary().values())
        assert all(a.size == 0 for a in kj.download(0, 0)) and all(a.size == 0 for a in kj.download())
    else:
        assert kj.distinct > 0
    if name == "shared":
        assert np.all(ca >= 1) and np.all(cb >= 1)
    if name == "fresh_in_b":
        assert not ca.any() and int(cb.min()) >= 2
    if name == "exactly_3_in_a":
        assert np.all(ca == 3)
    if name == "min_sum_50":
        assert int((ca + cb).min()) >= 50 and int(levels[0]) == 4
    kj.free()


@pytest.mark.parametrize("k", [10, 12])
def test_the_merge_identity(gpu, genome, k):
    """merge(a, b).kmers(k) without merging: the count is the sum of the counts and sp the sum of the insertion points."""
    A, B, ra, rb = genome
    kj = A.kmer_join(B, k)
    codes, ca, cb, spa, spb = kj.download()
    M = gpu.merge(A, B)
    assert M.sequences == 4000
    for encoded in (False, True):
        if encoded:
            M.encode()
        km = M.kmers(k)
        mcodes, mcounts, msp = km.download()
        assert np.array_equal(mcodes, codes) and np.array_equal(mcounts, ca + cb) and np.array_equal(msp, spa + spb)
        assert np.array_equal(km.levels(), kj.levels())
        km.free()
    want = brute(list(ra) + list(rb), k, 5)
    assert np.array_equal(codes, want[0]) and np.array_equal(ca + cb, want[1]) and np.array_equal(spa + spb, want[2])
    M.free(); kj.free()


def test_the_same_handle_on_both_sides(gpu, genome):
    A, B, ra, rb = genome
    kj = A.kmer_join(A, 12)
    codes, ca, cb, spa, spb = kj.download()
    km = A.kmers(12)
    kcodes, kcounts, ksp = km.download()
    assert np.array_equal(codes, kcodes) and np.array_equal(ca, kcounts) and np.array_equal(cb, kcounts) and np.array_equal(spa, ksp) and np.array_equal(spb, ksp)
    assert np.array_equal(kj.levels(), km.levels())
    s = kj.summary()
    assert s["only_a"] == s["only_b"] == 0 and s["both"] == km.distinct and s["both_occurrences_a"] == s["both_occurrences_b"] == km.total
    km.free(); kj.free()


def test_a_side_without_kmers_and_tiny_sides(gpu, oracle, genome):
    A, B, ra, rb = genome
    short = [r[:7] for r in rb[:50]]
    S = uploaded(gpu, oracle, short)
    part = ra[:300]
    P = uploaded(gpu, oracle, part)
    for X, Y, rx, ry, dead in ((P, S, part, short, 2), (S, P, short, part, 1)):
        got = check_pair(gpu, X, Y, rx, ry, 8)
        only = brute(list(part), 8, 5)
        assert not got[dead].any() and np.array_equal(got[0], only[0]) and np.array_equal(got[3 - dead], only[1])
        assert len(set(got[2 + dead].tolist())) > 20                              # the insertion points of the side that holds none of them
        check_pair(gpu, X, Y, rx, ry, 7)                                          # at k = 7 the short reads count
    kj = S.kmer_join(S, 8)
    assert kj.distinct == 0 and kj.nbytes == 0 and kj.levels().tolist()[7] == 0 and kj.levels().tolist()[6] > 0
    kj.free()
    one = [rb[3]]
    T = uploaded(gpu, oracle, one)
    for k in (1, 12, 32):
        check_pair(gpu, T, P, one, part, k)
        check_pair(gpu, P, T, part, one, k)
        check_pair(gpu, T, T, one, one, k)
    check_pair(gpu, T, P, one, part, 12, min_a=1)
    per_symbol = np.bincount(one[0], minlength=5)[1:5]
    assert per_symbol.min() <= 10 < per_symbol.max()                              # k = 1 is made on the host: the upper bounds act there too
    assert 0 < check_pair(gpu, T, P, one, part, 1, max_a=10)[0].size < 4
    assert 0 < check_pair(gpu, P, T, part, one, 1, min_b=11, max_b=40)[0].size < 4
    ragged = [rb[0], rb[1][:0], rb[2][:13], rb[3][:0], rb[4][:12], rb[5][:0]]
    R = uploaded(gpu, oracle, ragged)
    check_pair(gpu, R, T, ragged, one, 12)
    for h in (R, T, P, S):
        h.free()


def test_built_and_merged_handles(gpu, oracle):
    ra, rb = genome_reads(21)[:400], genome_reads(22)[:270]
    rc = pair_reads()[1][:350]
    A, B = uploaded(gpu, oracle, ra), uploaded(gpu, oracle, rb)
    both = np.concatenate([ra, rb])
    M = gpu.merge(A, B)                                                           # the merged collection
    bld = gpu.Builder(128)
    bld.add(rc)
    X = bld.finish()
    assert X.nbytes == 0                                                          # not encoded: records and super table only
    before = check_pair(gpu, M, X, both, rc, 10)
    swapped = check_pair(gpu, X, M, rc, both, 10, min_a=1, max_b=0)
    assert swapped[0].size > 0
    M.encode()
    after = check_pair(gpu, M, X, both, rc, 10)
    assert all(np.array_equal(u, v) for u, v in zip(before, after))
    check_pair(gpu, X, A, rc, ra, 10, min_a=1, min_b=1)
    M2 = gpu.merge(B, A)
    check_pair(gpu, M, M2, both, np.concatenate([rb, ra]), 10)
    for h in (M2, X, M, A, B):
        h.free()


@pytest.mark.parametrize("deltas", [(-1, 0), (0, 1), (1, -1), (0, 0)])
def test_ranges_that_end_at_n_on_a_record_edge(gpu, oracle, deltas):
    """n = 32 records exactly (128 reads of 31 symbols and their endmarkers), one less and one more, on either side: the last k-mer's range
    ends at n - 1 in each index."""
    sides = []
    for side, delta in enumerate(deltas):
        rng = np.random.default_rng(60 + 3 * side + delta)
        rows = [rng.integers(1, 5, size=31).astype(np.uint8) for _ in range(128)]
        rows[5] = rng.integers(1, 5, size=31 + delta).astype(np.uint8)
        rows[77][-4:] = 4                                                        # TTTT$ : the last suffixes of the collection
        x = uploaded(gpu, oracle, rows)
        assert x.bases == 32 * RECORD + delta
        sides.append((x, rows))
    (A, ra), (B, rb) = sides
    for k in (1, 3, 4):
        codes, ca, cb, spa, spb = check_pair(gpu, A, B, ra, rb, k)
        assert int(codes[-1]) == 4 ** k - 1 and int(spa[-1] + ca[-1]) == A.bases and int(spb[-1] + cb[-1]) == B.bases
    check_pair(gpu, A, B, ra, rb, 7)                                              # most 7-mers are in one side only: insertion points up to n
    A.free(); B.free()


def test_alphabets(gpu, oracle, pairs):
    A, B, ra, rb = pairs["iid"]                                                  # 1 % N
    # the sorted alphabet: $ A C G N T, so T is comp 5 and N comp 4
    sa, sb = ra.copy(), rb.copy()
    for s, r in ((sa, ra), (sb, rb)):
        s[r == 4] = 5; s[r == 5] = 4
    SA, SB = uploaded(gpu, oracle, sa), uploaded(gpu, oracle, sb)
    got = check_pair(gpu, SA, SB, sa, sb, 12, skip=4)
    want = expected("iid", 12)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    letters_default, letters_sorted = np.frombuffer(b"$ACGTN", dtype=np.uint8), np.frombuffer(b"$ACGNT", dtype=np.uint8)
    assert np.array_equal(letters_default[gpu.decode_kmers(want[0], 12, 5)], letters_sorted[gpu.decode_kmers(got[0], 12, 4)])
    SA.free(); SB.free()
    # reads of N alone hold no k-mer, on either side or on both
    ns = [np.full(17, 5, dtype=np.uint8), np.full(3, 5, dtype=np.uint8)]
    plain = pair_reads()[0][:300]
    N, P = uploaded(gpu, oracle, ns), uploaded(gpu, oracle, plain)
    got = check_pair(gpu, N, P, ns, plain, 9)
    assert not got[1].any() and int(got[2].sum()) == 300 * (40 - 9 + 1) and np.all(got[3] == 2)        # behind the two endmarkers, before every N
    check_pair(gpu, P, N, plain, ns, 9)
    kj = N.kmer_join(N, 1)
    assert kj.distinct == 0 and kj.levels().tolist() == [0]
    kj.free()
    N.free(); P.free()


def test_download_slices_and_null_outputs(gpu, genome):
    A, B, ra, rb = genome
    lib, p_u64 = gpu.capi.lib(), gpu.capi.p_u64
    kj = A.kmer_join(B, 12)
    whole = kj.download()
    d = kj.distinct
    for first, count in ((0, 0), (0, 1), (1, 1), (d - 1, 1), (d, 0), (1, d - 1), (1000, 257)):
        got = kj.download(first, count)
        assert all(np.array_equal(g, w[first: first + count]) for g, w in zip(got, whole)), (first, count)
    for which in range(5):                                                       # any of the five may be NULL
        only = np.zeros(5, dtype=np.uint64)
        args = [None] * 5
        args[which] = only.ctypes.data_as(p_u64)
        gpu.capi.check(lib.bwtm_kmer_join_download(kj.h, 7, 5, *args))
        assert np.array_equal(only, whole[which][7:12]), which
    gpu.capi.check(lib.bwtm_kmer_join_download(kj.h, 7, 5, None, None, None, None, None))
    for first, count in ((d, 1), (0, d + 1), (d + 1, 0), (1, (1 << 64) - 1), ((1 << 64) - 1, 2)):
        with pytest.raises(gpu.BwtmError) as e:
            kj.download(first, count)
        assert "lie beyond" in str(e.value)
    kj.free()
    with pytest.raises(gpu.BwtmError):
        kj.download()


def test_argument_errors(gpu, oracle, genome):
    from parts_inputs import host
    A, B, ra, rb = genome
    lib, vp = gpu.capi.lib(), gpu.capi.vp
    none = (1 << 64) - 1

    def create(a, b, k=12, skip=5, min_a=0, max_a=none, min_b=0, max_b=none, min_sum=1, out=True):
        res = vp()
        rc = lib.bwtm_kmer_join_create(a, b, k, skip, min_a, max_a, min_b, max_b, min_sum, C.byref(res) if out else None)
        if rc == 0:
            lib.bwtm_kmer_join_free(res)
        return rc, lib.bwtm_last_error().decode()

    for args, kw in (((None, B.h), {}), ((A.h, None), {}), ((A.h, B.h), dict(out=False))):
        rc, msg = create(*args, **kw)
        assert rc == EINVAL and "null argument" in msg
    fa = oracle.FMI.from_text(text_of(list(ra[:300])))
    ha = host(gpu, fa)
    b0, b1, fp, before_counts = gpu.window_blocks(ha, 1000, 5000)
    Cs = (C.c_uint64 * 7)(*[int(v) for v in fa.C])
    out = vp()
    data = fa.data                                        # a copy of the native bytes, alive over the call
    gpu.capi.check(lib.bwtm_index_upload_window(data.ctypes.data + 64 * b0, 64 * (b1 - b0), fp, before_counts, int(fa.bases), int(fa.sequences), Cs, 0, C.byref(out)))
    W = gpu.Index(out)
    for x, y, side in ((W, B, "a is a window"), (A, W, "b is a window"), (W, W, "a is a window")):
        with pytest.raises(gpu.BwtmError) as e:
            x.kmer_join(y, 10)
        assert side in str(e.value)
    W.free()
    ctx = gpu.Context(0); ctx.make_current()
    X = uploaded(gpu, oracle, ra[:100])
    gpu.make_default_current()
    for x, y in ((A, X), (X, A)):
        with pytest.raises(gpu.BwtmError) as e:
            x.kmer_join(y, 10)
        assert "different contexts" in str(e.value)
    X.free(); ctx.destroy()
    for kw, what in ((dict(k=0), "k = 0"), (dict(k=33), "k = 33"), (dict(skip=0), "skip = 0"), (dict(skip=6), "skip = 6"), (dict(min_a=3, max_a=2), "min_a = 3"),
                     (dict(min_b=1, max_b=0), "min_b = 1"), (dict(k=40, skip=9, min_a=3, max_a=2), "k = 40"), (dict(skip=9, min_a=3, max_a=2, min_b=2, max_b=1), "skip = 9"),
                     (dict(min_a=3, max_a=2, min_b=2, max_b=1), "min_a = 3")):
        rc, msg = create(A.h, B.h, **kw)
        assert rc == EINVAL and what in msg, (kw, msg)
    kj = A.kmer_join(B, 12, min_sum=0)                                           # a min_sum of 0 is taken as 1
    same_join(kj, expected("genome", 12))                                        # the indexes still answer
    null = np.zeros(7, dtype=np.uint64)
    assert lib.bwtm_kmer_join_summary(kj.h, None) == EINVAL and lib.bwtm_kmer_join_levels(None, null.ctypes.data_as(gpu.capi.p_u64)) == EINVAL
    assert lib.bwtm_kmer_join_distinct(None) == 0 and lib.bwtm_kmer_join_bytes(None) == 0
    lib.bwtm_kmer_join_free(None)
    kj.free()


def test_device_memory_stays_within_the_documented_bound(gpu, pairs):
    A, B, ra, rb = pairs["iid"]
    gpu.synchronize()
    gpu.trim()                                                                    # what the pool has cached so far is not this call's
    held = gpu.pool_stats()["held_bytes"]                                         # the indexes that are alive (these and other fixtures'), nothing else
    gpu.device_bytes_peak(reset=True)
    kj = A.kmer_join(B, 12)
    peak = gpu.device_bytes_peak()
    levels = kj.levels()
    assert int(levels.max()) > 40000
    assert held <= peak <= held + peak_formula(levels), (held, peak, peak_formula(levels))
    assert peak - held >= 40 * int(levels.max())                                  # the reset took: the call's own frontiers are in the figure
    assert 40 * kj.distinct <= kj.nbytes <= 40 * kj.distinct * 17 // 16 + 65536
    kj.free()


def test_on_a_poisoned_pool(bwtm):
    """The union and a filtered join of the genome pair at k = 12, twice, in a fresh process whose pool hands out blocks filled with
    0xA5A5A5A5: every total, base, node and sum that is read was written by the kernels."""
    env = dict(os.environ, BWTM_POOL_POISON="0xA5A5A5A5")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kmer_join_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), "exit status %s\n%s%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
    assert got and int(got.group(1)) > 0 and int(got.group(2)) >= 256 * int(got.group(1)), out.stdout[-3000:]
