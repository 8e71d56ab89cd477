"""The unitig kernels in the gfx950 ISA (no GPU needed): every kernel of kernels/unitigs.hip.h is compiled into the library's device code
once and keeps its state in registers -- no scratch memory.
Compiles the device code to ISA text and reads the per-kernel metadata, like tests/test_isa_correct.py, with a list of its own."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "bwt-merge_amd", "csrc", "bwtm_api.hip")
OUT = os.path.join(ROOT, "tests", "_build", "bwtm_api_unitigs.s")
KERNELS = (r"k_unitig_countsE", r"k_unitig_linksE", r"k_unitig_nextE", r"k_unitig_walkE", r"k_unitig_unreachedE", r"k_unitig_cycle_initE",
           r"k_unitig_cycle_jumpE", r"k_unitig_cycle_startsE", r"k_unitig_numberE", r"k_unitig_textE", r"k_unitig_fill_linksE", r"k_unitig_placeE")


@pytest.fixture(scope="module")
def isa():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", OUT, SRC],
                          stderr=subprocess.DEVNULL)
    kernels, cur = {}, None
    for line in open(OUT):
        m = re.match(r"^(_ZN4bwtm\w+):", line)
        if m:
            cur = m.group(1); kernels[cur] = {}
            continue
        m = re.match(r"; (ScratchSize|NumVgprs|Occupancy): (\d+)", line)
        if m and cur:
            kernels[cur].setdefault(m.group(1), int(m.group(2)))
    return kernels


def test_unitig_kernels_are_present_and_use_no_scratch(isa):
    for kernel in KERNELS:
        found = [(name, meta) for name, meta in isa.items() if re.match(r"_ZN4bwtm\d+%s" % kernel, name)]
        assert len(found) == 1, "%s: %d kernels of that name in the ISA" % (kernel, len(found))
        name, meta = found[0]
        assert "ScratchSize" in meta and meta["ScratchSize"] == 0, "%s uses %s bytes of scratch per lane" % (name, meta.get("ScratchSize"))
        print(name, meta)
