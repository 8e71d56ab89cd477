"""Locate, the parts that need no GPU: the tool exists and says how it is used, the binding knows the calls and the knob -- and the
expected values of the GPU tests (tests/locate_inputs.py) are checked here against the oracle: the sorted suffixes of the reads spell
the oracle's BWT, and the identity the locator's table rests on holds on it."""
import os
import subprocess

import numpy as np

from locate_inputs import all_suffixes, naive_hits, substring_table, suffix_order
from test_gpu_sequences import ragged_reads, text_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")


def test_bwt_locate_builds_and_the_calls_are_bound(bwtm):
    bwtm.build()
    subprocess.check_call(["make", "-C", HOST, "-s"])
    exe = os.path.join(HOST, "bwt_locate")
    assert os.path.exists(exe) and os.path.exists(os.path.join(HOST, "host_load_test"))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "Usage: bwt_locate [options] input patterns output" in out.stderr
    for option in ("-g N", "-i format", "-m N", "-x N"):
        assert option in out.stderr, option
    bound = {name: args for name, _, args in bwtm.capi.SYMBOLS}
    for name, nargs in (("bwtm_locator_create", 3), ("bwtm_locator_free", 1), ("bwtm_locator_bytes", 1), ("bwtm_locate_batch", 5), ("bwtm_locate_ranges", 9)):
        assert name in bound and len(bound[name]) == nargs, name
        assert hasattr(bwtm.capi.lib(), name)
    assert bwtm.tune("locate_batch", 64) is None and bwtm.tune("locate_batch", 0) is None     # the knob exists (an unknown key raises)
    assert callable(getattr(bwtm.Index, "locator")) and all(hasattr(bwtm.Locator, f) for f in ("locate", "locate_ranges", "locate_patterns", "nbytes", "free"))


def test_expected_values_agree_with_the_oracle(oracle):
    """On the 300 ragged reads: the suffixes in sorted order have the oracle's BWT symbols before them; the walk from any position to the first
    endmarker symbol, the rank of 0 there and the table built from the walks from positions 0 .. m - 1 give exactly that (id, offset)."""
    m = 300
    reads, lengths = ragged_reads(oracle, m, 7101)
    f = oracle.FMI.from_text(text_of(reads, lengths))
    bwt = np.asarray(f.symbols)
    n = bwt.size
    assert n == 4680 and f.sequences == m
    ids, offs = suffix_order(reads, lengths)
    assert set(zip(ids.tolist(), offs.tolist())) == all_suffixes(lengths) and ids.size == n
    before = np.array([reads[int(j), int(o) - 1] if o > 0 else 0 for j, o in zip(ids, offs)], dtype=np.uint8)
    assert np.array_equal(before, bwt)
    C = np.zeros(7, dtype=np.int64)
    C[1:] = np.cumsum(np.bincount(bwt, minlength=6))[:6]
    rank = np.zeros((6, n + 1), dtype=np.int64)
    for c in range(6):
        rank[c, 1:] = np.cumsum(bwt == c)

    def walk(p):
        d = 0
        while bwt[p] != 0:
            c = int(bwt[p]); p = int(C[c] + rank[c, p]); d += 1
        return int(rank[0, p]), d

    table = np.full(m, -1, dtype=np.int64)
    for j in range(m):
        k, d = walk(j)
        assert d == lengths[j]
        table[k] = j
    assert sorted(table.tolist()) == list(range(m))
    got = [walk(p) for p in range(n)]
    assert [int(table[k]) for k, d in got] == ids.tolist() and [d for k, d in got] == offs.tolist()
    # the substring table against a direct scan
    tab = substring_table(reads, lengths, 4)
    pattern = reads[39, 7:10]
    want = sorted((j, o) for j in range(m) for o in range(int(lengths[j]) - 2) if np.array_equal(reads[j, o: o + 3], pattern))
    assert naive_hits(tab, lengths, pattern) == want and (39, 7) in want and (38, 2) in want
    assert naive_hits(tab, lengths, []) == sorted(all_suffixes(lengths))
