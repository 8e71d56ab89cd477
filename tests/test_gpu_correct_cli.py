"""bwt_ingest -> bwt_correct on the genome collection of the k-mer tests: the lines, the reads -x drops, the sub-ranges and the summary on
stderr are the brute force's (tests/correct_inputs.py), and the output goes through bwt_ingest and bwt_extract unchanged."""
import os
import subprocess

import numpy as np
import pytest

from correct_inputs import FAILED, correct_all
from kmer_inputs import genome_reads
from test_gpu_sequences_cli import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")
pytestmark = pytest.mark.gpu
K, T, R = 12, 3, 10


def lines_of(texts):
    return ["".join("$ACGTN"[v] for v in t) for t in texts]


def summary(status, edits, solid):
    counts = np.bincount(status, minlength=4).tolist()
    return "clean=%d corrected=%d failed=%d short=%d edits=%d solid=%d" % (counts[0], counts[1], counts[2], counts[3], int(edits.sum()), solid)


def test_cli_ingest_correct_ingest_extract(bwtm, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    from correct_inputs import solid_count, table_of
    rows = genome_reads()
    rows[7, 20] = 5                                                              # one N: the alphabet of the file has it
    rows = list(rows)
    (tmp_path / "reads.txt").write_text("\n".join(lines_of(rows)) + "\n")
    bwt = str(tmp_path / "reads.bwt")
    run([os.path.join(HOST, "bwt_ingest"), "-l", "128", str(tmp_path / "reads.txt"), bwt])
    table = table_of(rows, K)
    texts, status, edits = correct_all(rows, K, T, R, table=table)
    solid = solid_count(table, T)
    want = lines_of(texts)
    assert FAILED in status and want != lines_of(rows)
    tool = os.path.join(HOST, "bwt_correct")
    opts = ["-k", str(K), "-t", str(T), "-r", str(R)]
    out = run([tool] + opts + [bwt, str(tmp_path / "all.txt")])
    assert (tmp_path / "all.txt").read_text().split("\n") == want + [""]
    assert out.stderr.rstrip("\n").split("\n")[-1] == summary(status, edits, solid)
    # -x drops exactly the FAILED reads; the summary still counts them
    out = run([tool] + opts + ["-x", "-i", "native", bwt, str(tmp_path / "kept.txt")])
    assert (tmp_path / "kept.txt").read_text().split("\n") == [w for w, s in zip(want, status.tolist()) if s != FAILED] + [""]
    assert out.stderr.rstrip("\n").split("\n")[-1] == summary(status, edits, solid)
    # sub-ranges: the table is that of the whole index
    for first, count in ((0, 1), (1990, None), (301, 555)):
        sel = slice(first, None if count is None else first + count)
        out = run([tool] + opts + ["-f", str(first)] + ([] if count is None else ["-n", str(count)]) + [bwt, str(tmp_path / "part.txt")])
        assert (tmp_path / "part.txt").read_text().split("\n") == want[sel] + [""]
        assert out.stderr.rstrip("\n").split("\n")[-1] == summary(status[sel], edits[sel], solid)
    # the defaults are k = 21, t = 3, r = 10
    out = run([tool, bwt, str(tmp_path / "defaults.txt")])
    table21 = table_of(rows, 21)
    d_texts, d_status, d_edits = correct_all(rows, 21, 3, 10, table=table21)
    assert (tmp_path / "defaults.txt").read_text().split("\n") == lines_of(d_texts) + [""]
    assert out.stderr.rstrip("\n").split("\n")[-1] == summary(d_status, d_edits, solid_count(table21, 3))
    # the output is bwt_ingest's input: the corrected index gives the same lines back
    run([os.path.join(HOST, "bwt_ingest"), "-l", "128", str(tmp_path / "all.txt"), str(tmp_path / "corrected.bwt")])
    run([os.path.join(HOST, "bwt_extract"), str(tmp_path / "corrected.bwt"), str(tmp_path / "back.txt")])
    assert (tmp_path / "back.txt").read_text().split("\n") == want + [""]
    for bad, what in ((["-k", "33"], "1 to 32"), (["-r", "65536"], "65535")):
        out = subprocess.run([tool] + bad + [bwt, str(tmp_path / "bad.txt")], capture_output=True, text=True)
        assert out.returncode != 0 and what in out.stderr
