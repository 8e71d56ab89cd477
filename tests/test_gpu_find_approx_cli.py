"""bwt_ingest -> bwt_locate -d on a small file the test writes: with -d 1 the lines, as a set, are the brute force's occurrences with their
mismatch column (tests/approx_inputs.py); without -d the tool writes the bytes of -d 0 with the last column removed."""
import os
import subprocess

import numpy as np
import pytest

from approx_inputs import Collection, cut_patterns, genome_reads
from test_gpu_sequences_cli import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")
pytestmark = pytest.mark.gpu


def test_cli_locate_with_mismatches(bwtm, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    rows = genome_reads(14)[:300]
    rows[7, 20] = 5                                                              # one N: the alphabet of the file has it
    letters = "$ACGTN"
    (tmp_path / "reads.txt").write_text("\n".join("".join(letters[v] for v in row) for row in rows) + "\n")
    coll = Collection(list(rows))
    patterns = cut_patterns(coll.rows, (3, 12, 31, 40), 6, 15) + cut_patterns(coll.rows, (12, 40), 3, 16, substitutions=0) + [rows[7, 15:27].copy()]
    (tmp_path / "patterns.txt").write_text("\n".join("".join(letters[v] for v in p) for p in patterns) + "\n")
    bwt = str(tmp_path / "reads.bwt")
    run([os.path.join(HOST, "bwt_ingest"), "-l", "128", str(tmp_path / "reads.txt"), bwt])
    locate = os.path.join(HOST, "bwt_locate")
    args = ["-m", "128", bwt, str(tmp_path / "patterns.txt")]
    out = run([locate, "-d", "1"] + args + [str(tmp_path / "d1.tsv")])
    assert "up to 1 substitutions" in out.stdout and "(pattern, sequence, offset, mismatches)" in out.stdout
    got = (tmp_path / "d1.tsv").read_text().split("\n")
    assert got[-1] == ""
    want = set()
    for k, p in enumerate(patterns):
        want |= {"%d\t%d\t%d\t%d" % ((k,) + occ) for occ in coll.hits(p, 1, want_occurrences=True)[4]}
    assert len(got) - 1 == len(want) and set(got[:-1]) == want
    assert {line.split("\t")[3] for line in got[:-1]} == {"0", "1"}
    # the exact search: three columns, as it always wrote them
    plain = run([locate] + args + [str(tmp_path / "plain.tsv")])
    assert "(pattern, sequence, offset)" in plain.stdout and "substitutions" not in plain.stdout
    run([locate, "-d", "0"] + args + [str(tmp_path / "d0.tsv")])
    d0 = (tmp_path / "d0.tsv").read_bytes()
    assert d0.count(b"\n") >= 9 and all(line.endswith(b"\t0") for line in d0.split(b"\n")[:-1])
    assert (tmp_path / "plain.tsv").read_bytes() == b"".join(line[:-2] + b"\n" for line in d0.split(b"\n")[:-1])
    exact = {"%d\t%d\t%d" % ((k,) + occ[:2]) for k, p in enumerate(patterns) for occ in coll.hits(p, 0, want_occurrences=True)[4]}
    assert set((tmp_path / "plain.tsv").read_text().split("\n")[:-1]) == exact
    bad = subprocess.run([locate, "-d", "9"] + args + [str(tmp_path / "bad.tsv")], capture_output=True, text=True)
    assert bad.returncode != 0 and "0 to 8" in bad.stderr
