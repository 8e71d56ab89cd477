"""The k-mer join, the parts that need no GPU: the expected values of the GPU tests (tests/kmer_join_inputs.py) are checked here against the
oracle -- the backward search of a k-mer on the oracle's FMI of either collection gives its count there and the first position of its range,
and for a k-mer that collection does not hold an empty range -- and the pair of collections is as hard as the GPU tests need it.
FMI.find stops at the first empty range, so for an absent k-mer the sp it returns is the insertion point of the SUFFIX it had reached, not
of the k-mer.  The insertion point of the whole k-mer is therefore taken from the oracle's own step, FMI.LF(i, c) = C[c] + rank(i, c), applied
to both ends of the range for every symbol without stopping; where find does not stop early the two agree, which is checked as well."""
import os
import subprocess

import numpy as np

from kmer_inputs import decode, text_of
from kmer_join_inputs import brute_pair, classes, pair_reads

K = 12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_range(f, pattern):
    s, e = f.find(np.ascontiguousarray(pattern, dtype=np.uint8))
    return int(s), int(e)


def oracle_walk(f, pattern):
    """(sp, count) by the oracle's LF on both ends of the half-open range, all symbols: sp is the insertion point when count == 0."""
    C = f.C
    c = int(pattern[-1])
    s, e = int(C[c]), int(C[c + 1])
    for c in reversed(pattern[:-1].tolist()):
        s, e = f.LF(s, int(c)), f.LF(e, int(c))
    return s, e - s


def test_brute_pair_against_the_oracle(oracle):
    rows_a, rows_b = pair_reads()
    assert rows_a.shape == rows_b.shape == (2000, 40) and min(rows_a.min(), rows_b.min()) == 1 and max(rows_a.max(), rows_b.max()) == 4
    fa, fb = (oracle.FMI.from_text(text_of(list(rows))) for rows in (rows_a, rows_b))
    codes, ca, cb, spa, spb = brute_pair(rows_a, rows_b, K, 5)
    assert np.all(codes[1:] > codes[:-1]) and np.all(spa[1:] >= spa[:-1] + ca[:-1]) and np.all(spb[1:] >= spb[:-1] + cb[:-1])
    for rows, counts in ((rows_a, ca), (rows_b, cb)):
        assert int(counts.sum()) == rows.shape[0] * (rows.shape[1] - K + 1)
    assert np.all(ca + cb >= 1)
    rng = np.random.default_rng(3)
    for members in ((ca > 0) & (cb == 0), (ca == 0) & (cb > 0), (ca > 0) & (cb > 0)):
        picks = rng.choice(np.flatnonzero(members), size=200, replace=False)
        for j, pattern in zip(picks.tolist(), decode(codes[picks], K, 5)):
            for f, counts, sp in ((fa, ca, spa), (fb, cb, spb)):
                s, e = oracle_range(f, pattern)
                assert (e + 1 - s) % (1 << 64) == int(counts[j]), (j, s, e)      # an absent k-mer: ep == sp - 1 in the oracle's unsigned arithmetic
                assert int(counts[j]) == 0 or s == int(sp[j]), (j, s, e)
                assert oracle_walk(f, pattern) == (int(sp[j]), int(counts[j])), (j, oracle_walk(f, pattern))


def test_the_pair_is_as_hard_as_the_gpu_tests_need(oracle):
    rows_a, rows_b = pair_reads()
    want = brute_pair(rows_a, rows_b, K, 5)
    only_a, only_b, both = classes(want)[:3]
    assert min(only_a, only_b, both) >= 500, (only_a, only_b, both)
    fresh = brute_pair(rows_a, rows_b, K, 5, max_a=0, min_b=2)
    assert fresh[0].size >= 50 and not fresh[1].any() and int(fresh[2].min()) >= 2
    assert fresh[0].size < only_b                                                # the threshold drops the error k-mers of b
    shared = brute_pair(rows_a, rows_b, K, 5, min_a=1, min_b=1)
    assert shared[0].size == both
    assert sum(classes(want)[:3]) == want[0].size and classes(want)[3] + classes(want)[5] == int(want[1].sum())


def test_bwt_kmer_compare_builds_and_the_calls_are_bound(bwtm):
    host = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")
    bwtm.build()
    subprocess.check_call(["make", "-C", host, "-s"])
    out = subprocess.run([os.path.join(host, "bwt_kmer_compare")], capture_output=True, text=True)
    assert out.returncode == 0 and "Usage: bwt_kmer_compare [options] input1 input2 output" in out.stderr
    for option in ("-g N", "-i format", "-k N", "-a N", "-A N", "-b N", "-B N", "-s N", "-S"):
        assert option in out.stderr, option
    bound = {name: args for name, _, args in bwtm.capi.SYMBOLS}
    for name, nargs in (("bwtm_kmer_join_create", 10), ("bwtm_kmer_join_free", 1), ("bwtm_kmer_join_distinct", 1), ("bwtm_kmer_join_bytes", 1),
                        ("bwtm_kmer_join_levels", 2), ("bwtm_kmer_join_download", 8), ("bwtm_kmer_join_summary", 2)):
        assert name in bound and len(bound[name]) == nargs and hasattr(bwtm.capi.lib(), name), name
    assert all(callable(getattr(bwtm.KmerJoin, f)) for f in ("levels", "download", "summary", "free")) and callable(bwtm.Index.kmer_join)
    header = open(os.path.join(ROOT, "include", "bwtm.h")).read()
    for name in bound:
        if name.startswith("bwtm_kmer_join_"):
            assert name + "(" in header, name
