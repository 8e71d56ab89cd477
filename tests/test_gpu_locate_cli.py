"""bwt_ingest -> bwt_merge -> bwt_locate: the hits file is a naive substring search over the normalised reads, line for line."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_sequences_cli import ragged_text_reads, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")
pytestmark = pytest.mark.gpu


def occurrences(normal, pattern):
    """Sorted (read, offset) of every occurrence, overlapping ones included."""
    hits = []
    for j, read in enumerate(normal):
        o = read.find(pattern)
        while o >= 0:
            hits.append((j, o))
            o = read.find(pattern, o + 1)
    return hits


def test_cli_ingest_merge_locate(bwtm, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    reads, normal = ragged_text_reads()
    for name, part in (("a", reads[:400]), ("b", reads[400:])):
        (tmp_path / (name + ".txt")).write_text("\n".join(part) + "\n")
        run([os.path.join(HOST, "bwt_ingest"), "-l", "150", str(tmp_path / (name + ".txt")), str(tmp_path / (name + ".bwt"))])
    run([os.path.join(HOST, "bwt_merge"), str(tmp_path / "a.bwt"), str(tmp_path / "b.bwt"), str(tmp_path / "ab.bwt")])
    rng = np.random.default_rng(22)
    patterns = []
    while len(patterns) < 120:                                            # cut from both sides of the merge, 1 .. 12 symbols
        j = int(rng.integers(0, len(normal)))
        if len(normal[j]) == 0:
            continue
        k = int(rng.integers(1, min(12, len(normal[j])) + 1))
        o = int(rng.integers(0, len(normal[j]) - k + 1))
        patterns.append(normal[j][o: o + k])
    patterns.append(normal[5])                                            # a whole read that is there twice (reads 5 and 6)
    patterns.append(normal[17])                                           # the read with the foreign character, as the tools stored it
    absent = "ACGTACGTTTGGCCAANNAC"
    assert not occurrences(normal, absent)
    patterns.append(absent)
    # empty lines between the patterns are skipped and do not count
    (tmp_path / "patterns.txt").write_text("\n".join(patterns[:50]) + "\n\n" + "\n".join(patterns[50:]) + "\n")
    want = [occurrences(normal, p) for p in patterns]
    assert (5, 0) in want[120] and (6, 0) in want[120] and (17, 0) in want[121]
    locate = os.path.join(HOST, "bwt_locate")
    out = run([locate, str(tmp_path / "ab.bwt"), str(tmp_path / "patterns.txt"), str(tmp_path / "hits.tsv")])
    lines = ["%d\t%d\t%d" % (k, j, o) for k in range(len(patterns)) for j, o in want[k]]
    assert (tmp_path / "hits.tsv").read_text().split("\n") == lines + [""]
    assert "Located %d patterns: %d found, %d hits" % (len(patterns), sum(1 for w in want if w), len(lines)) in out.stdout
    run([locate, "-i", "native", "-m", "139", "-x", "1", str(tmp_path / "ab.bwt"), str(tmp_path / "patterns.txt"), str(tmp_path / "one.tsv")])
    one = [tuple(int(v) for v in line.split("\t")) for line in (tmp_path / "one.tsv").read_text().split("\n") if line]
    assert [k for k, j, o in one] == [k for k in range(len(patterns)) if want[k]]                    # one line per matching pattern
    assert all((j, o) in want[k] for k, j, o in one)
    # a bound that a read exceeds is an error, not a partial file of hits
    out = subprocess.run([locate, "-m", "20", str(tmp_path / "ab.bwt"), str(tmp_path / "patterns.txt"), str(tmp_path / "short.tsv")], capture_output=True, text=True)
    assert out.returncode != 0 and "longer than max_len" in out.stderr
