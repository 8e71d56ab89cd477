"""bwt_ingest -> bwt_merge -> bwt_extract: the reads that went in come out, line by line."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")
pytestmark = pytest.mark.gpu


def ragged_text_reads(seed=21, n=900):
    """n reads over ACGTN of 0..139 symbols, with empty lines, lower case and one foreign character; and what the tools make of them:
    upper case, foreign characters as N."""
    rng = np.random.default_rng(seed)
    chars = np.frombuffer(b"ACGTN", dtype=np.uint8)
    reads = []
    for k in range(n):
        length = int(rng.integers(0, 140)) if k % 9 else 100
        reads.append(bytes(chars[rng.integers(0, 5, size=length)]).decode())
    reads[3] = ""; reads[4] = ""; reads[400] = ""; reads[n - 1] = ""
    reads[6] = reads[5]
    reads[17] = "acgtnacgtX"
    reads[405] = reads[405].lower()
    normal = ["".join(c if c in "ACGTN" else "N" for c in r.upper()) for r in reads]
    return reads, normal


def run(args):
    out = subprocess.run(args, capture_output=True, text=True)
    assert out.returncode == 0, " ".join(args) + "\n" + out.stdout + out.stderr
    return out


def test_cli_round_trip_ingest_merge_extract(bwtm, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    reads, normal = ragged_text_reads()
    assert normal[17] == "ACGTNACGTN" and normal != reads
    for name, part in (("a", reads[:400]), ("b", reads[400:])):
        (tmp_path / (name + ".txt")).write_text("\n".join(part) + "\n")
        run([os.path.join(HOST, "bwt_ingest"), "-l", "150", str(tmp_path / (name + ".txt")), str(tmp_path / (name + ".bwt"))])
    run([os.path.join(HOST, "bwt_merge"), str(tmp_path / "a.bwt"), str(tmp_path / "b.bwt"), str(tmp_path / "ab.bwt")])
    extract = os.path.join(HOST, "bwt_extract")
    out = run([extract, str(tmp_path / "ab.bwt"), str(tmp_path / "ab.txt")])
    assert "Wrote 900 reads of total length %d" % sum(len(r) for r in normal) in out.stdout
    assert (tmp_path / "ab.txt").read_text() == "\n".join(normal) + "\n"
    run([extract, "-f", "400", "-n", "10", str(tmp_path / "ab.bwt"), str(tmp_path / "ten.txt")])
    assert (tmp_path / "ten.txt").read_text().split("\n") == normal[400:410] + [""]
    run([extract, "-i", "native", "-f", "895", "-n", "1000", "-m", "139", str(tmp_path / "ab.bwt"), str(tmp_path / "tail.txt")])      # -n beyond the end: what is there
    assert (tmp_path / "tail.txt").read_text() == "\n".join(normal[895:]) + "\n"
    # a bound that a read exceeds is an error, not a truncated file
    out = subprocess.run([extract, "-m", "20", str(tmp_path / "ab.bwt"), str(tmp_path / "short.txt")], capture_output=True, text=True)
    assert out.returncode != 0 and "longer than max_len" in out.stderr
