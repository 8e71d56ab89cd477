"""bwt_ingest -> bwt_kmers on the genome collection of the k-mer tests: the list and the spectrum are the sliding-window count of the reads,
line for line."""
import os
import subprocess

import numpy as np
import pytest

from kmer_inputs import brute, decode, folded_histogram, genome_reads
from test_gpu_sequences_cli import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")
pytestmark = pytest.mark.gpu
K = 12


def lines_of(codes, counts):
    letters = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    return ["%s\t%d" % (bytes(letters[row]).decode(), c) for row, c in zip(decode(codes, K, 5), counts.tolist())]


def test_cli_ingest_kmers(bwtm, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    rows = genome_reads()
    rows[7, 20] = 5                                                              # one N: the alphabet of the file has it, no k-mer does
    (tmp_path / "reads.txt").write_text("\n".join("".join("$ACGTN"[v] for v in row) for row in rows) + "\n")
    bwt = str(tmp_path / "reads.bwt")
    run([os.path.join(HOST, "bwt_ingest"), "-l", "128", str(tmp_path / "reads.txt"), bwt])
    codes, counts, _ = brute(list(rows), K, 5)
    kmers = os.path.join(HOST, "bwt_kmers")
    out = run([kmers, "-k", str(K), bwt, str(tmp_path / "all.tsv")])
    got = (tmp_path / "all.tsv").read_text().split("\n")
    assert got == lines_of(codes, counts) + [""] and got[:-1] == sorted(got[:-1])
    assert "Found %d distinct %d-mers of count 1 or more, %d occurrences" % (codes.size, K, int(counts.sum())) in out.stdout
    run([kmers, "-i", "native", "-k", str(K), "-H", "64", bwt, str(tmp_path / "hist.tsv")])
    hist = folded_histogram(counts, 64)
    assert (tmp_path / "hist.tsv").read_text().split("\n") == ["%d\t%d" % (j, v) for j, v in enumerate(hist.tolist()) if v > 0] + [""]
    assert hist[0] == 0 and int(hist.sum()) == codes.size
    kept = brute(list(rows), K, 5, 3)
    run([kmers, "-k", str(K), "-c", "3", bwt, str(tmp_path / "solid.tsv")])
    assert (tmp_path / "solid.tsv").read_text().split("\n") == lines_of(kept[0], kept[1]) + [""] and 2500 <= kept[0].size < codes.size - 1000
    out = subprocess.run([kmers, "-k", "33", bwt, str(tmp_path / "long.tsv")], capture_output=True, text=True)
    assert out.returncode != 0 and "1 to 32" in out.stderr
