"""bwt_ingest -> bwt_unitigs: the GFA the tool writes is parsed here and compared with the brute force of tests/unitig_inputs.py --
segments, KC, links, the circular tag -- and so is the summary on stderr; bad options exit non-zero with a message."""
import os
import subprocess

import pytest

from kmer_inputs import genome_reads
from test_gpu_sequences_cli import run
from unitig_inputs import CIRCULAR, NONE, Graph, case, comps_of, table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")
pytestmark = pytest.mark.gpu


def lines_of(rows):
    return ["".join("$ACGTN"[v] for v in r) for r in rows]


def parse(path):
    """(segments {id: (text, KC, circular)}, links [(from, to, overlap)]) of a GFA 1 file whose records are all on the plus strand."""
    lines = open(path).read().split("\n")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == ""
    segments, links, seen_link = {}, [], False
    for line in lines[1:-1]:
        f = line.split("\t")
        if f[0] == "S":
            assert not seen_link and int(f[1]) == len(segments) and f[3].startswith("KC:i:") and f[4:] in ([], ["TP:Z:circular"])
            segments[int(f[1])] = (f[2], int(f[3][5:]), f[4:] == ["TP:Z:circular"])
        else:
            assert f[0] == "L" and len(f) == 6 and f[2] == "+" and f[4] == "+" and f[5].endswith("M")
            seen_link = True
            links.append((int(f[1]), int(f[3]), int(f[5][:-1])))
    return segments, links


def compare(path, stderr, g):
    segments, links = parse(path)
    assert len(segments) == g.U
    for u, (text, _, occ, flags, _) in enumerate(g.unitigs):
        assert segments[u] == ("".join("$ACGTN"[v] for v in text), occ, bool(flags & CIRCULAR)), u
    want = [(u, v, g.k - 1) for u, unitig in enumerate(g.unitigs) for v in unitig[4] if v != NONE]
    assert links == want
    assert open(path).read().split("\n")[:-1] == g.gfa()
    circular = sum(1 for unitig in g.unitigs if unitig[3] & CIRCULAR)
    assert stderr.rstrip("\n").split("\n")[-1] == "nodes=%d unitigs=%d circular=%d links=%d longest=%d" % (g.S, g.U, circular, len(want), g.longest)


def test_cli_ingest_unitigs(bwtm, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    tool = os.path.join(HOST, "bwt_unitigs")
    rows = genome_reads()
    rows[7, 20] = 5                                                              # one N: the alphabet of the file has it
    rows = list(rows)
    (tmp_path / "reads.txt").write_text("\n".join(lines_of(rows)) + "\n")
    bwt = str(tmp_path / "reads.bwt")
    run([os.path.join(HOST, "bwt_ingest"), "-l", "128", str(tmp_path / "reads.txt"), bwt])
    for k, t in ((12, 3), (12, 1)):
        out = run([tool, "-k", str(k), "-t", str(t), "-i", "native", bwt, str(tmp_path / "graph.gfa")])
        compare(str(tmp_path / "graph.gfa"), out.stderr, Graph(table_of(rows, k), k, t))
    out = run([tool, bwt, str(tmp_path / "defaults.gfa")])                        # the defaults are k = 21, t = 3
    compare(str(tmp_path / "defaults.gfa"), out.stderr, Graph(table_of(rows, 21), 21, 3))
    # circular segments, and a unitig that links to itself
    cyc = case("long_cycle")[0] + [comps_of("TTGCA" + "ACGT" * 6), comps_of("N")]
    (tmp_path / "cycles.txt").write_text("\n".join(lines_of(cyc)) + "\n")
    run([os.path.join(HOST, "bwt_ingest"), "-l", "128", str(tmp_path / "cycles.txt"), str(tmp_path / "cycles.bwt")])
    out = run([tool, "-k", "12", "-t", "1", str(tmp_path / "cycles.bwt"), str(tmp_path / "cycles.gfa")])
    g = Graph(table_of(cyc, 12), 12, 1)
    assert g.circular_nodes == 3000 and any(u in unitig[4] for u, unitig in enumerate(g.unitigs))
    compare(str(tmp_path / "cycles.gfa"), out.stderr, g)
    for bad, what in ((["-k", "33"], "1 to 32"), (["-k", "0"], "1 to 32"), (["-i", "nonsense"], "Invalid input format")):
        out = subprocess.run([tool] + bad + [bwt, str(tmp_path / "bad.gfa")], capture_output=True, text=True)
        assert out.returncode != 0 and what in out.stderr
    out = subprocess.run([tool, bwt], capture_output=True, text=True)
    assert out.returncode != 0 and "must be specified" in out.stderr
    out = subprocess.run([tool, str(tmp_path / "missing.bwt"), str(tmp_path / "bad.gfa")], capture_output=True, text=True)
    assert out.returncode != 0
