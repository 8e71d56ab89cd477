"""The merge over partitioned records with every part in a PROCESS of its own, as it is deployed (bench.py --gpus N,
one rank per GPU): each part exports its buffers through HIP IPC handles and its kernels read the other parts' buffers with system-scope
loads.  The parts run in fresh child processes (tests/parts_child.py) on GPU 0; the parent lays their slices end to end and compares them
with the oracle's merge bit for bit, as tests/test_gpu_parts.py does for parts that are threads of one process.

On a shared card: at most four children at a time, each with BWTM_GROUP_TIMEOUT=60, all waited on under one time limit per case and killed
when it runs out.  A child that dies by a signal or by the time limit fails its case and skips every later case of this module (nothing more
is started on a card that may have faulted).  Nothing is retried."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from parts_inputs import ODD_CASES, check_against_oracle, odd_collection, truly_empty, wide_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "parts_child.py")
MAX_CHILDREN = 4
GROUP_TIMEOUT = 60
BWTM_ENOMEM, BWTM_EPEER = 3, 5

_stopped = []                       # why no more children may be started in this module


@pytest.fixture(autouse=True)
def _card_still_trusted():
    if _stopped:
        pytest.skip(_stopped[0])


@pytest.fixture(scope="module")
def partitioned(bwtm):
    from bwt_merge_amd import partitioned
    return partitioned


def save_input(directory, tag, x):
    """Writes an oracle FMI as the child reads it; returns its prefix."""
    prefix = os.path.join(str(directory), tag)
    np.save(prefix + "_data.npy", np.ascontiguousarray(x.data, dtype=np.uint8))
    np.save(prefix + "_cum.npy", np.ascontiguousarray(x.samples[1], dtype=np.uint64))
    with open(prefix + ".json", "w") as f:
        json.dump({"sequences": int(x.sequences), "bases": int(x.bases)}, f)
    return prefix


def run_parts(partitioned, directory, parts, merges, limit):
    """Starts `parts` children that run `merges` (dicts of parts_child.py's spec; "group": a small number, the same for merges that share a
    group) and waits for all of them within `limit` seconds.  Returns records[merge][part]: the child's record, with data / be / cum arrays
    for the merges that succeeded."""
    assert 1 <= parts <= MAX_CHILDREN
    directory = str(directory)
    names = {}
    merges = [dict(m, group=names.setdefault(m["group"], partitioned.unique_group_name("proc"))) for m in merges]
    env = dict(os.environ, BWTM_GROUP_TIMEOUT=str(GROUP_TIMEOUT))
    procs, logs = [], []
    try:
        for g in range(parts):
            spec = os.path.join(directory, "spec%d.json" % g)
            with open(spec, "w") as f:
                json.dump({"part": g, "parts": parts, "out": directory, "merges": merges}, f)
            logs.append(open(os.path.join(directory, "part%d.log" % g), "w"))
            procs.append(subprocess.Popen([sys.executable, CHILD, spec], cwd=ROOT, env=env, stdout=logs[-1], stderr=subprocess.STDOUT))
        deadline = time.monotonic() + limit
        for p in procs:
            p.wait(timeout=max(0.0, deadline - time.monotonic()))
    except subprocess.TimeoutExpired:
        _stopped.append("a child of an earlier case ran past its time limit")
        pytest.fail("the parts did not finish within %d s:\n%s" % (limit, tails(directory, parts)))
    finally:
        for p in procs:                                                  # (the time limit, or the parent failed while starting them)
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
        for f in logs:
            f.close()
    rcs = [p.returncode for p in procs]
    if any(rc < 0 for rc in rcs):
        _stopped.append("a child of an earlier case died by a signal (return codes %s)" % rcs)
        pytest.fail("a part died by a signal: return codes %s\n%s" % (rcs, tails(directory, parts)))
    assert all(rc == 0 for rc in rcs), "return codes %s\n%s" % (rcs, tails(directory, parts))
    records = [[None] * parts for _ in merges]
    for g in range(parts):
        with open(os.path.join(directory, "part%d.json" % g)) as f:
            for rec in json.load(f):
                k = rec["merge"]
                if "error" not in rec:
                    for tag in ("data", "be", "cum"):
                        rec[tag] = np.load(os.path.join(directory, "part%d_%d_%s.npy" % (g, k, tag)))
                records[k][g] = rec
    return records


def tails(directory, parts):
    out = []
    for g in range(parts):
        path = os.path.join(directory, "part%d.log" % g)
        text = open(path).read() if os.path.exists(path) else ""
        out.append("--- part %d ---\n%s" % (g, text[-2000:]))
    return "\n".join(out)


def assemble(recs):
    """-> (data, block_end, cum, stats) of one merge's slices laid end to end; every part must have succeeded."""
    errors = [(g, r.get("code"), r["error"]) for g, r in enumerate(recs) if "error" in r]
    assert not errors, errors
    total = recs[0]["total_nbytes"]
    assert all(r["total_nbytes"] == total for r in recs)
    offsets = [r["byte_offset"] for r in recs]
    assert offsets == sorted(offsets) and offsets[0] == 0
    for r, nxt in zip(recs, offsets[1:] + [total]):
        assert r["byte_offset"] + r["data"].size == nxt                  # the slices tile the stream
    data = np.concatenate([r["data"] for r in recs]); be = np.concatenate([r["be"] for r in recs]); cum = np.concatenate([r["cum"] for r in recs], axis=1)
    assert data.size == total
    return data, be, cum, [r["stats"] for r in recs]


@pytest.fixture(scope="module")
def iid(oracle, tmp_path_factory):
    """2.4 M + 1.9 M positions (several encoder segments per part), written once for all the iid cases."""
    d = tmp_path_factory.mktemp("iid")
    a = oracle.FMI.from_text(oracle.generate_reads(9801, 24000, 100)); b = oracle.FMI.from_text(oracle.generate_reads(9802, 19000, 100))
    return a, b, save_input(d, "a", a), save_input(d, "b", b)


@pytest.mark.parametrize("parts,kmer,range_ratio", [(2, 1, 8), (3, 3, 0), (4, 4, 8), (4, 2, 1)])
def test_processes_merge_equals_oracle(partitioned, oracle, iid, tmp_path, parts, kmer, range_ratio):
    """Node phase of a few levels, none at all (elements from the roots on), and the whole search on nodes (range_ratio = 1)."""
    a, b, pa, pb = iid
    recs = run_parts(partitioned, tmp_path, parts, [dict(group=0, a=pa, b=pb, kmer=kmer, knobs={"range_ratio": range_ratio})], limit=240)
    data, be, cum, stats = assemble(recs[0])
    check_against_oracle(oracle, a, b, data, be, cum)
    if range_ratio == 0:
        assert all(s["node_levels"] == 0 for s in stats)
        assert sum(s["elements"] for s in stats) == b.bases              # every element of every step was advanced by exactly one part
        assert all(s["steps"] == 101 for s in stats)
    elif range_ratio == 8:
        assert all(s["node_levels"] > 0 for s in stats) and all(s["steps"] + s["node_levels"] == 101 for s in stats)
    # records and bitvector are partitioned, not replicated: all parts together hold them once (+ margins and boundary tiles)
    whole = 64 * ((a.bases >> 7) + 1 + (b.bases >> 7) + 1)
    margins = parts * 2 * (2 * 2 * 65536 // 128 + 4) * 64
    assert sum(s["record_bytes"] for s in stats) <= whole + margins
    assert sum(s["bitvector_bytes"] for s in stats) <= (a.bases + b.bases) // 8 + parts * 4 * 8192 + 8192
    if parts > 1:
        assert all(s["boundary_bytes"] == 8192 for s in stats)


@pytest.mark.parametrize("case", ODD_CASES)
def test_processes_merge_of_odd_collections(partitioned, oracle, tmp_path, case):
    """Collections on which most parts end up with nothing, three parts; the second merge runs on the same group (its buffers re-used)."""
    ta, tb = odd_collection(case)
    a, b = oracle.FMI.from_text(ta), oracle.FMI.from_text(tb)
    pa, pb = save_input(tmp_path, "a", a), save_input(tmp_path, "b", b)
    recs = run_parts(partitioned, tmp_path, 3, [dict(group=0, a=pa, b=pb, kmer=2, knobs={"range_ratio": 8}),
                                                dict(group=0, a=pa, b=pb, kmer=3, knobs={"range_ratio": 0})], limit=180)
    for k in range(2):
        data, be, cum, _ = assemble(recs[k])
        check_against_oracle(oracle, a, b, data, be, cum, threads=1)


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("parts", [2, 3])
def test_processes_merge_with_a_truly_empty_input(partitioned, oracle, tmp_path, which, parts):
    """An input of 0 sequences and 0 bytes: the merge is the other input, as the oracle's is."""
    a, b = truly_empty(oracle, which)
    pa, pb = save_input(tmp_path, "a", a), save_input(tmp_path, "b", b)
    recs = run_parts(partitioned, tmp_path, parts, [dict(group=0, a=pa, b=pb, kmer=2, knobs={"range_ratio": 8}),
                                                    dict(group=0, a=pa, b=pb, kmer=3, knobs={"range_ratio": 0})], limit=180)
    other = b if which == "a" else a
    for k in range(2):
        data, be, cum, stats = assemble(recs[k])
        m = check_against_oracle(oracle, a, b, data, be, cum, threads=1)
        assert np.array_equal(m.data, other.data) and np.array_equal(data, other.data)
        if which == "b":
            assert all(s["elements"] == 0 and s["steps"] == 0 for s in stats)


def test_processes_chain_through_one_group(partitioned, oracle, tmp_path):
    """Three merges of growing size on one group in every process: the exported buffers are re-allocated and re-mapped between merges (the
    peers open new IPC handles); every merge is the oracle's."""
    sets = [oracle.FMI.from_text(oracle.generate_reads(9100 + k, n, 80)) for k, n in enumerate((1500, 4000, 12000, 30000))]
    prefixes = [save_input(tmp_path, "s%d" % k, x) for k, x in enumerate(sets)]
    recs = run_parts(partitioned, tmp_path, 3, [dict(group=0, a=prefixes[k], b=prefixes[k + 1], kmer=3) for k in range(3)], limit=240)
    for k in range(3):
        data, be, cum, _ = assemble(recs[k])
        check_against_oracle(oracle, sets[k], sets[k + 1], data, be, cum)


@pytest.mark.parametrize("capacity,range_ratio", [(2000, 8), (-3000, 0)])
def test_processes_out_of_room_stop_every_part(partitioned, oracle, iid, tmp_path, capacity, range_ratio):
    """A part that overflows (the knob part_capacity: at the expansion of the node levels / in an element step) stops every process from the
    same collective call, well inside BWTM_GROUP_TIMEOUT: itself with BWTM_ENOMEM, the others with BWTM_EPEER (or their own ENOMEM).  The
    same processes then run a clean merge on a fresh group, and it is the oracle's."""
    a, b, pa, pb = iid
    recs = run_parts(partitioned, tmp_path, 4, [dict(group=0, a=pa, b=pb, kmer=3, knobs={"part_capacity": capacity, "range_ratio": range_ratio}),
                                                dict(group=1, a=pa, b=pb, kmer=3)], limit=240)
    failed = recs[0]
    assert all("error" in r for r in failed), failed
    codes = [r["code"] for r in failed]
    assert set(codes) <= {BWTM_ENOMEM, BWTM_EPEER}, failed
    assert any(r["code"] == BWTM_ENOMEM and "capacity" in r["error"] for r in failed), failed
    assert all(r["seconds"] < GROUP_TIMEOUT / 2 for r in failed), [r["seconds"] for r in failed]
    data, be, cum, _ = assemble(recs[1])
    check_against_oracle(oracle, a, b, data, be, cum)


@pytest.mark.parametrize("rr", [0, 4])
def test_processes_wide_coordinates(partitioned, bwtm, oracle, tmp_path, rr):
    """Coordinates beyond 2^32: their high bytes travel through the peers' exported buffers.  Compared with the single-GPU merge of the same
    inputs (in this process, after the children have exited)."""
    a, b = wide_inputs(oracle)
    pa, pb = save_input(tmp_path, "a", a), save_input(tmp_path, "b", b)
    recs = run_parts(partitioned, tmp_path, 3, [dict(group=0, a=pa, b=pb, kmer=2, knobs={"frontier_epoch": 5, "range_ratio": rr})], limit=240)
    data, be, cum, _ = assemble(recs[0])
    bwtm.init(0)
    A = bwtm.Index.upload(a.data, a.sequences, a.bases); B = bwtm.Index.upload(b.data, b.sequences, b.bases)
    M = bwtm.merge(A, B)
    try:
        assert np.array_equal(data, M.data())
        mbe, mcum = M.samples()
        assert np.array_equal(be, mbe) and np.array_equal(cum, mcum[:, :-1])
    finally:
        M.free(); A.free(); B.free()
