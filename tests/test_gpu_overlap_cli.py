"""bwt_ingest -> bwt_overlap on the 300 reads of the overlap input: the TSV is the all-pairs string comparison of the reads, line for line."""
import os
import subprocess

import pytest

from overlap_inputs import overlap_reads, prefix_table, rows_of, table_hits
from test_gpu_sequences_cli import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")
pytestmark = pytest.mark.gpu
TAU = 5


def lines_of(path):
    return [tuple(int(v) for v in line.split("\t")) for line in path.read_text().split("\n") if line]


def test_cli_ingest_overlap(bwtm, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    reads, lengths = overlap_reads(300, 1)
    rows = rows_of(reads, lengths)
    (tmp_path / "reads.txt").write_text("\n".join("".join(" ACGT"[v] for v in row) for row in rows) + "\n")     # comp values 1..4
    bwt = str(tmp_path / "reads.bwt")
    run([os.path.join(HOST, "bwt_ingest"), "-l", "128",str(tmp_path / "reads.txt"), bwt])
    table = prefix_table(rows)
    want = [(q, t, l) for q in range(300) for t, l in table_hits(table, rows[q], TAU)]
    overlap = os.path.join(HOST, "bwt_overlap")
    out = run([overlap, "-t", str(TAU), bwt, str(tmp_path / "all.tsv")])
    assert (tmp_path / "all.tsv").read_text().split("\n") == ["%d\t%d\t%d" % h for h in want] + [""]
    assert "Searched 300 sequences: %d with overlaps, %d hits" % (len({q for q, t, l in want}), len(want)) in out.stdout
    run([overlap, "-i", "native", "-m", "40", "-t", str(TAU), "-s", bwt, str(tmp_path / "others.tsv")])
    assert lines_of(tmp_path / "others.tsv") == [(q, t, l) for q, t, l in want if not (t == q and l == len(rows[q]))]
    run([overlap, "-t", str(TAU), "-x", "2", bwt, str(tmp_path / "two.tsv")])
    two = [(q, t, l) for q in range(300) for t, l in table_hits(table, rows[q], TAU)[:2]]
    assert lines_of(tmp_path / "two.tsv") == two and len(two) < len(want)
    run([overlap, "-t", str(TAU), "-x", "2", "-s", bwt, str(tmp_path / "two_s.tsv")])                            # -s applies after -x
    assert lines_of(tmp_path / "two_s.tsv") == [(q, t, l) for q, t, l in two if not (t == q and l == len(rows[q]))]
    run([overlap, "-t", str(TAU), "-f", "100", "-n", "57", bwt, str(tmp_path / "page.tsv")])
    assert lines_of(tmp_path / "page.tsv") == [h for h in want if 100 <= h[0] < 157]
    run([overlap, "-t", str(TAU), "-f", "290", "-n", "1000", bwt, str(tmp_path / "tail.tsv")])                  # -n beyond the end: what is there
    assert lines_of(tmp_path / "tail.tsv") == [h for h in want if h[0] >= 290]
    # a bound that a read exceeds is an error, not a partial file of hits
    out = subprocess.run([overlap, "-m", "20", bwt, str(tmp_path / "short.tsv")], capture_output=True, text=True)
    assert out.returncode != 0 and "longer than max_len" in out.stderr
