"""bwt_ingest -> bwt_locate -e on a small file the test writes: with -e 1 the lines, as a set, are the brute force's occurrences with their
edits and length columns (tests/edit_inputs.py); without -e the tool writes the bytes of -e 0 with the last two columns removed."""
import os
import subprocess

import pytest

from approx_inputs import cut_patterns
from edit_inputs import EditCollection, edited_patterns, genome_reads
from test_gpu_sequences_cli import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")
pytestmark = pytest.mark.gpu


def test_cli_locate_with_edits(bwtm, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    rows = genome_reads(14)[:300]
    rows[7, 20] = 5                                                              # one N: the alphabet of the file has it
    letters = "$ACGTN"
    (tmp_path / "reads.txt").write_text("\n".join("".join(letters[v] for v in row) for row in rows) + "\n")
    coll = EditCollection(list(rows))
    patterns = edited_patterns(coll.rows, (3, 12, 31, 40), 5, 15) + cut_patterns(coll.rows, (12, 40), 3, 16, substitutions=0) + [rows[7, 15:27].copy()]
    (tmp_path / "patterns.txt").write_text("\n".join("".join(letters[v] for v in p) for p in patterns) + "\n")
    bwt = str(tmp_path / "reads.bwt")
    run([os.path.join(HOST, "bwt_ingest"), "-l", "128", str(tmp_path / "reads.txt"), bwt])
    locate = os.path.join(HOST, "bwt_locate")
    args = ["-m", "128", bwt, str(tmp_path / "patterns.txt")]
    out = run([locate, "-e", "1"] + args + [str(tmp_path / "e1.tsv")])
    assert "up to 1 edits" in out.stdout and "(pattern, sequence, offset, edits, length)" in out.stdout
    got = (tmp_path / "e1.tsv").read_text().split("\n")
    assert got[-1] == ""
    want = set()
    for k, p in enumerate(patterns):
        want |= {"%d\t%d\t%d\t%d\t%d" % ((k,) + occ) for occ in coll.edit_hits(p, 1, want_occurrences=True)[5]}
    assert len(got) - 1 == len(want) and set(got[:-1]) == want
    assert {line.split("\t")[3] for line in got[:-1]} == {"0", "1"}
    relative = {int(line.split("\t")[4]) - len(patterns[int(line.split("\t")[0])]) for line in got[:-1]}
    assert relative == {-1, 0, 1}                                                # a symbol less, the same, a symbol more
    # the exact search: three columns, as it always wrote them
    plain = run([locate] + args + [str(tmp_path / "plain.tsv")])
    assert "(pattern, sequence, offset)" in plain.stdout and "Search:" not in plain.stdout
    run([locate, "-e", "0"] + args + [str(tmp_path / "e0.tsv")])
    e0 = (tmp_path / "e0.tsv").read_bytes().split(b"\n")[:-1]
    assert len(e0) >= 9
    stripped = []
    for k_line in e0:
        cols = k_line.split(b"\t")
        assert len(cols) == 5 and cols[3] == b"0" and int(cols[4]) == len(patterns[int(cols[0])])
        stripped.append(b"\t".join(cols[:3]) + b"\n")
    assert (tmp_path / "plain.tsv").read_bytes() == b"".join(stripped)
    bad = subprocess.run([locate, "-e", "8"] + args + [str(tmp_path / "bad.tsv")], capture_output=True, text=True)
    assert bad.returncode != 0 and "0 to 7" in bad.stderr
    both = subprocess.run([locate, "-d", "1", "-e", "1"] + args + [str(tmp_path / "both.tsv")], capture_output=True, text=True)
    assert both.returncode != 0 and "cannot be used together" in both.stderr
