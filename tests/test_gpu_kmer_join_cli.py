"""bwt_ingest -> bwt_kmer_compare on the genome pair of the k-mer join tests: the list and the summary are what sliding windows over the
reads of both collections give, line for line."""
import os
import subprocess

import numpy as np
import pytest

from kmer_inputs import decode
from kmer_join_inputs import brute_pair, classes, pair_reads
from test_gpu_sequences_cli import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")
pytestmark = pytest.mark.gpu
K = 12


def lines_of(want):
    letters = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    return ["%s\t%d\t%d" % (bytes(letters[row]).decode(), a, b) for row, a, b in zip(decode(want[0], K, 5), want[1].tolist(), want[2].tolist())]


def test_cli_ingest_kmer_compare(bwtm, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    ra, rb = pair_reads()
    ra[7, 20] = 5; rb[9, 3] = 5                                                  # an N each: the alphabet of the files has it, no k-mer does
    files = []
    for name, rows in (("a", ra), ("b", rb)):
        (tmp_path / (name + ".txt")).write_text("\n".join("".join("$ACGTN"[v] for v in row) for row in rows) + "\n")
        files.append(str(tmp_path / (name + ".bwt")))
        run([os.path.join(HOST, "bwt_ingest"), "-l", "128", str(tmp_path / (name + ".txt")), files[-1]])
    compare = os.path.join(HOST, "bwt_kmer_compare")
    want = brute_pair(ra, rb, K, 5)
    out = run([compare, "-k", str(K)] + files + [str(tmp_path / "all.tsv")])
    got = (tmp_path / "all.tsv").read_text().split("\n")
    assert got == lines_of(want) + [""] and got[:-1] == sorted(got[:-1])
    only_a, only_b, both = classes(want)[:3]
    assert "Kept %d distinct %d-mers: %d only in input 1, %d only in input 2, %d in both" % (want[0].size, K, only_a, only_b, both) in out.stdout
    run([compare, "-i", "native", "-k", str(K), "-S"] + files + [str(tmp_path / "summary.tsv")])
    rows = [line.split("\t") for line in (tmp_path / "summary.tsv").read_text().split("\n")[:-1]]
    assert len(rows) == 7 and [int(v) for _, v in rows] == classes(want) and len({name for name, _ in rows}) == 7
    assert min(only_a, only_b, both) >= 500
    fresh = brute_pair(ra, rb, K, 5, max_a=0, min_b=2)
    run([compare, "-k", str(K), "-A", "0", "-b", "2"] + files + [str(tmp_path / "fresh.tsv")])
    assert (tmp_path / "fresh.tsv").read_text().split("\n") == lines_of(fresh) + [""] and 50 <= fresh[0].size < only_b
    solid = brute_pair(ra, rb, K, 5, min_a=1, max_b=40, min_sum=30)
    run([compare, "-k", str(K), "-a", "1", "-B", "40", "-s", "30"] + files + [str(tmp_path / "solid.tsv")])
    assert (tmp_path / "solid.tsv").read_text().split("\n") == lines_of(solid) + [""] and solid[0].size >= 50
    out = subprocess.run([compare, "-k", "33"] + files + [str(tmp_path / "long.tsv")], capture_output=True, text=True)
    assert out.returncode != 0 and "1 to 32" in out.stderr
    out = subprocess.run([compare, "-z", "1"] + files + [str(tmp_path / "bad.tsv")], capture_output=True, text=True)
    assert out.returncode != 0 and not (tmp_path / "bad.tsv").exists()
    out = subprocess.run([compare, "-a", "3", "-A", "2"] + files + [str(tmp_path / "bad.tsv")], capture_output=True, text=True)
    assert out.returncode != 0 and "exceeds" in out.stderr
