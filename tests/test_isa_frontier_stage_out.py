"""The staged form of k_frontier_step (template flag STAGE, bwtm_tune frontier_stage_out = 1) in the ISA, compiled here for gfx950 (no GPU
needed): full occupancy, no scratch, the coordinates leave through ONE non-temporal 8-byte store per lane, and nothing behind the second
barrier waits for memory (a vmcnt wait there would expose the latency of the emits that are still in flight)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "bwt-merge_amd", "csrc", "bwtm_api.hip")
OUT = os.path.join(ROOT, "tests", "_build", "bwtm_api_stage_out.s")


@pytest.fixture(scope="module")
def step_kernels():
    """{mangled name: (metadata, instruction lines)} of every k_frontier_step instantiation."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", OUT, SRC], stderr=subprocess.DEVNULL)
    kernels, cur, in_body = {}, None, False
    for line in open(OUT):
        m = re.match(r"^(_ZN4bwtm15k_frontier_step\w+):", line)
        if m:
            cur = m.group(1); kernels[cur] = ({}, []); in_body = True
            continue
        if re.match(r"^_Z\w+:", line):
            cur = None
        if cur is None:
            continue
        m = re.match(r"; (ScratchSize|NumVgprs|Occupancy|LDSByteSize): (\d+)", line)
        if m:
            kernels[cur][0].setdefault(m.group(1), int(m.group(2)))
        elif in_body and line.startswith("\t") and not line.startswith("\t."):
            kernels[cur][1].append(line.strip())
            if line.strip() == "s_endpgm":
                in_body = False
    return kernels


@pytest.mark.parametrize("hi", [False, True])
@pytest.mark.parametrize("pull", [False, True])
def test_staged_step_kernel(step_kernels, hi, pull):
    flag = lambda b: "Lb1E" if b else "Lb0E"
    name = "_ZN4bwtm15k_frontier_stepILi0E" + flag(hi) + "Lb0E" + flag(pull) + "Lb1EEEvNS_9IndexViewES1_NS_12FrontierViewE"
    assert name in step_kernels, sorted(step_kernels)
    meta, code = step_kernels[name]
    assert meta["Occupancy"] == 8 and meta["ScratchSize"] == 0, meta
    assert meta["LDSByteSize"] <= 4096, meta                           # 8 workgroups per CU stay far inside the CU's LDS
    barriers = [k for k, ins in enumerate(code) if ins.startswith("s_barrier")]
    assert len(barriers) == 3, barriers                                # the staging of the segment table, the class totals, the staged output
    tail = code[barriers[-1]:]
    coords = [ins for ins in code if re.match(r"global_store_dwordx2 .* nt$", ins)]
    assert len(coords) == 1 and coords[0] in tail, coords              # thread t stores s_out[t]: one 8-byte non-temporal store, behind the last barrier
    if hi:
        assert len([ins for ins in tail if re.match(r"global_store_short .* nt$", ins)]) == 1
    assert not [ins for ins in tail if "vmcnt" in ins], [ins for ins in tail if "vmcnt" in ins]
    assert [ins for ins in tail if ins.startswith("global_atomic_umin")], "lane 0's tile marker is issued behind the stores"


def test_unstaged_form_keeps_its_lds(step_kernels):
    """The old form (STAGE = false) carries no staging array: it is the code of rounds 1 - 6."""
    for name, (meta, code) in step_kernels.items():
        if name.endswith("Lb0EEEvNS_9IndexViewES1_NS_12FrontierViewE"):
            assert meta["LDSByteSize"] < 1024 and len([ins for ins in code if ins.startswith("s_barrier")]) == 2, (name, meta)
