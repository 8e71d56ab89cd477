"""bench.py's options without a GPU: what only --full measures is refused in a plain run, before anything touches the device."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra", [["--target", "on"], ["--profile-all"]])
def test_parts_of_full_are_refused_in_a_plain_run(extra):
    out = subprocess.run([sys.executable, "bench.py", "--steps", "1", "--warmup", "0"] + extra, cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "parts of --full" in out.stderr and not out.stdout


def test_full_is_documented():
    out = subprocess.run([sys.executable, "bench.py", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--full" in out.stdout
