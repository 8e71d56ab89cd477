"""Overlaps, the parts that need no GPU: the tool exists and says how it is used, the binding knows the calls and the knob -- and the
expected values of the GPU tests (tests/overlap_inputs.py) are checked here against the oracle: a backward search on the oracle's BWT
whose rank(., 0) pairs are looked up in the locator's table reproduces the all-pairs string comparison, order included."""
import os
import subprocess

import numpy as np

from overlap_inputs import all_pairs_hits, overlap_reads, prefix_table, rows_of, table_hits
from test_gpu_sequences import text_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")


def test_bwt_overlap_builds_and_the_calls_are_bound(bwtm):
    bwtm.build()
    subprocess.check_call(["make", "-C", HOST, "-s"])
    exe = os.path.join(HOST, "bwt_overlap")
    assert os.path.exists(exe)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "Usage: bwt_overlap [options] input output" in out.stderr
    for option in ("-g N", "-i format", "-t N", "-x N", "-f N", "-n N", "-m N", "-s "):
        assert option in out.stderr, option
    bound = {name: args for name, _, args in bwtm.capi.SYMBOLS}
    for name in ("bwtm_overlap_batch", "bwtm_overlap_sequences"):
        assert name in bound and len(bound[name]) == 10, name
        assert hasattr(bwtm.capi.lib(), name)
    assert bwtm.tune("overlap_batch", 64) is None and bwtm.tune("overlap_batch", 0) is None   # the knob exists (an unknown key raises)
    assert all(callable(getattr(bwtm.Locator, f)) for f in ("overlaps", "overlap_patterns"))


def test_expected_values_agree_with_the_oracle(oracle):
    """On the 300 reads of the overlap input: the backward search of every read on the oracle's BWT with cumulative rank arrays, the
    interval [rank(sp, 0), rank(ep + 1, 0)) after every symbol and the table built from the walks from positions 0 .. m - 1 give exactly
    the hits of the all-pairs comparison, longest first and in ascending BWT position within a length -- and the input is as hard as the
    GPU tests need it: many hits, a query with many lengths, a large interval, a read that overlaps itself."""
    m, tau = 300, 5
    reads, lengths = overlap_reads(m, 1)
    rows = rows_of(reads, lengths)
    f = oracle.FMI.from_text(text_of(reads, lengths))
    bwt = np.asarray(f.symbols)
    n = bwt.size
    assert f.sequences == m and n == int(lengths.sum()) + m
    C = np.zeros(7, dtype=np.int64)
    C[1:] = np.cumsum(np.bincount(bwt, minlength=6))[:6]
    rank = np.zeros((6, n + 1), dtype=np.int64)
    for c in range(6):
        rank[c, 1:] = np.cumsum(bwt == c)
    table = np.full(m, -1, dtype=np.int64)
    for j in range(m):
        p = j
        while bwt[p] != 0:
            c = int(bwt[p]); p = int(C[c] + rank[c, p])
        table[int(rank[0, p])] = j
    assert sorted(table.tolist()) == list(range(m))

    def search(query):
        """Hits in the order found: lengths ascending, BWT position ascending within one."""
        found, sp, e1 = [], 0, n
        for l in range(1, len(query) + 1):
            c = query[len(query) - l]
            sp, e1 = int(C[c] + rank[c, sp]), int(C[c] + rank[c, e1])
            if sp >= e1:
                break
            if l >= tau:
                found.append((l, [int(table[z]) for z in range(int(rank[0, sp]), int(rank[0, e1]))]))
        return found

    hashed = prefix_table(rows)
    total = nontrivial = periodic = 0
    most_hits = most_lengths = largest = 0
    for q in range(m):
        want = all_pairs_hits(rows, rows[q], tau)
        assert table_hits(hashed, rows[q], tau) == want, q                  # the hashed form the larger GPU cases use
        found = search(rows[q])
        got = [(t, l) for l, targets in reversed(found) for t in targets]
        assert got == want, q
        total += len(want); nontrivial += sum(1 for t, l in want if t != q)
        periodic += sum(1 for t, l in want if t == q and l < len(rows[q]))
        most_hits = max(most_hits, len(want)); most_lengths = max(most_lengths, len([1 for l, targets in found if targets]))
        largest = max([largest] + [len(targets) for l, targets in found])
        if len(rows[q]) >= tau:
            assert want[0][1] == len(rows[q]) and (q, len(rows[q])) in want    # the read itself, over its whole length
        else:
            assert want == []
    print("hits %d, not the query itself %d, self-overlaps below the full length %d, most hits %d, most lengths %d, largest interval %d"
          % (total, nontrivial, periodic, most_hits, most_lengths, largest))
    assert total > 2000 and most_lengths >= 20 and largest >= 10 and periodic >= 1
