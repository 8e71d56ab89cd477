"""bwt_ingest -> bwt_locate -M on a small file the test writes: every line's piece of the pattern is the located sequence's text at that
offset, the lines, as a set, are the brute force's MEMs with their occurrences (tests/mem_inputs.py), and -M does not go with -d."""
import os
import subprocess

import pytest

from mem_inputs import Brute, varied_patterns
from overlap_inputs import overlap_reads, rows_of
from test_gpu_sequences_cli import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")
pytestmark = pytest.mark.gpu


def test_cli_locate_maximal_exact_matches(bwtm, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    rows = [list(r) for r in rows_of(*overlap_reads(300, 1)) if len(r) > 0]
    with_n = next(j for j, r in enumerate(rows) if len(r) >= 12)
    rows[with_n][3] = 5                                                          # one N: the alphabet of the file has it
    rows = [tuple(r) for r in rows]
    letters = "$ACGTN"
    (tmp_path / "reads.txt").write_text("\n".join("".join(letters[v] for v in row) for row in rows) + "\n")
    patterns = varied_patterns(rows, 41)[::13] + [rows[with_n], rows[with_n][:4], (5, 5, 5, 5, 5, 5)]
    (tmp_path / "patterns.txt").write_text("\n".join("".join(letters[v] for v in p) for p in patterns) + "\n")
    bwt = str(tmp_path / "reads.bwt")
    run([os.path.join(HOST, "bwt_ingest"), "-l", "128", str(tmp_path / "reads.txt"), bwt])
    locate = os.path.join(HOST, "bwt_locate")
    args = ["-m", "128", bwt, str(tmp_path / "patterns.txt")]
    out = run([locate, "-M", "5"] + args + [str(tmp_path / "mems.tsv")])
    assert "maximal exact matches of at least 5 symbols" in out.stdout and "(pattern, sequence, offset, begin, length)" in out.stdout
    got = (tmp_path / "mems.tsv").read_text().split("\n")
    assert got[-1] == ""
    for line in got[:-1]:
        k, t, o, b, l = (int(v) for v in line.split("\t"))
        assert l >= 5 and patterns[k][b:b + l] == rows[t][o:o + l], line
    brute = Brute(rows)
    want = set()
    for k, p in enumerate(patterns):
        for b, l, _, _ in brute.mems(p, 5):
            w = tuple(p[b:b + l])
            want |= {"%d\t%d\t%d\t%d\t%d" % (k, t, o, b, l) for t, r in enumerate(rows) for o in range(len(r) - l + 1) if r[o:o + l] == w}
    assert len(got) - 1 == len(want) > 50 and set(got[:-1]) == want
    assert not any(line.startswith("%d\t" % (len(patterns) - 1)) or line.startswith("%d\t" % (len(patterns) - 2)) for line in got[:-1])   # too short, absent
    # -x caps the occurrences of every match
    run([locate, "-M", "5", "-x", "1"] + args + [str(tmp_path / "one.tsv")])
    one = (tmp_path / "one.tsv").read_text().split("\n")[:-1]
    assert set(one) <= want and len(one) == len({tuple(line.split("\t")[i] for i in (0, 3, 4)) for line in got[:-1]})
    for flags in (["-M", "5", "-d", "1"], ["-d", "1", "-M", "5"], ["-M", "5", "-e", "1"], ["-M", "0"]):
        bad = subprocess.run([locate] + flags + args + [str(tmp_path / "bad.tsv")], capture_output=True, text=True)
        assert bad.returncode != 0 and "-M" in bad.stderr, flags
