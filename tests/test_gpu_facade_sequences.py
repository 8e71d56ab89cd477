"""FMI::sequences of the C++ facade on the GPU (csrc/host/host_sequences_test.cpp): ranges of ids of an ingested index against the
lines of the reads file it was built from."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")


@pytest.mark.gpu
def test_facade_sequences_on_gpu(bwtm, tmp_path):
    from test_gpu_sequences_cli import ragged_text_reads
    subprocess.check_call(["make", "-C", HOST, "-s"])
    reads, normal = ragged_text_reads(seed=22, n=700)
    (tmp_path / "reads.txt").write_text("\n".join(reads) + "\n")
    (tmp_path / "normal.txt").write_text("\n".join(normal) + "\n")
    out = subprocess.run([os.path.join(HOST, "bwt_ingest"), "-l", "256", str(tmp_path / "reads.txt"), str(tmp_path / "reads.bwt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    out = subprocess.run([os.path.join(HOST, "host_sequences_test"), str(tmp_path / "reads.bwt"), str(tmp_path / "normal.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and "sequences ok" in out.stdout, out.stdout + out.stderr
    # the program does compare: the same index against the reads in another order fails
    (tmp_path / "wrong.txt").write_text("\n".join(normal[1:] + normal[:1]) + "\n")
    out = subprocess.run([os.path.join(HOST, "host_sequences_test"), str(tmp_path / "reads.bwt"), str(tmp_path / "wrong.txt")], capture_output=True, text=True)
    assert out.returncode == 1 and "differs from the read" in out.stderr, out.stdout + out.stderr
