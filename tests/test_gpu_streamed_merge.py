"""bwtm_merge_host_streamed: the merged BWT leaves the device slice by slice, at most two slices alive, and reaches the caller's sink in
pieces.  Laid end to end the pieces must be the oracle's merged stream and samples, whatever the slice size: many slices, a short last
slice, one slice, the library's own choice; slices without a run head, with bytes but no block start, runs that end on a cut, a block
opened slices earlier -- also in an earlier super block of 2^25 positions, where the encoder answers the block's counts from the slice's
first record and the super table instead of a record it does not hold.  The checks themselves live in tests/streamed_child.py, which is
also the child process of the cases on poisoned device memory."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from streamed_child import COMPACT, FULL, check_streamed, collect, inp, long_run_symbols, read_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "streamed_child.py")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    yield bwtm
    bwtm.tune("stream_samples_query", 0)


@pytest.fixture(scope="module")
def reads(gpu, oracle):
    """The read sets, the oracle's merge and the one-shot call's compact samples, computed once (read only)."""
    a, b, m = read_sets(oracle)
    r = gpu.merge_host(inp(a), inp(b), samples=2)
    assert r.out.sample_width in (1, 2, 4) and np.array_equal(r.data, m.data)
    oneshot = (r.out.sample_width, r.fields.copy(), r.anchors.copy())
    r.free()
    return a, b, m, oneshot


@pytest.mark.parametrize("slice_records", [512, 1024, 1536, 1 << 30, 0])
def test_streamed_merge_of_read_sets(gpu, reads, slice_records):
    a, b, m, oneshot = reads
    check_streamed(gpu, inp(a), inp(b), m, slice_records, oneshot=oneshot, bound=slice_records in (512, 1536))
    pieces, out, stats = collect(gpu, inp(a), inp(b), slice_records, COMPACT)
    nrecs = (m.bases >> 7) + 1
    if slice_records == 1 << 30:
        assert len(pieces) == 1 and stats.slice_records == (nrecs + 511) // 512 * 512
    elif slice_records != 0:
        assert len(pieces) == (nrecs + slice_records - 1) // slice_records           # reads: every slice has heads, bytes and blocks
    else:
        assert stats.slice_records >= 512 and stats.slice_records % 512 == 0


def test_slice_records_must_be_whole_segments(gpu, reads):
    a, b, m, _ = reads
    with pytest.raises(gpu.BwtmError, match="multiple of 512"):
        gpu.capi.merge_host_streamed(inp(a), inp(b), 1000)
    with pytest.raises(gpu.BwtmError):
        gpu.capi.merge_host_streamed(inp(a), inp(b), 512, samples=-1)                 # a result on the device is what the other calls are for


@pytest.mark.parametrize("slice_records", [512, 2048])
@pytest.mark.parametrize("case", ["long_runs", "one_run", "runs_on_cuts", "tiny"])
def test_streamed_across_long_runs(gpu, oracle, case, slice_records):
    """The recipe of test_slices_across_long_runs: merging with an empty increment makes the interleave a copy, so any string can be
    put through the streamed second half."""
    f = oracle.FMI.from_symbols(long_run_symbols(case))
    e = oracle.FMI.from_symbols(np.zeros(0, dtype=np.uint8))
    check_streamed(gpu, inp(f), inp(e), f, slice_records)
    if case == "one_run" and slice_records == 512:
        pieces, out, stats = collect(gpu, inp(f), inp(e), slice_records, FULL)
        assert len(pieces) < (f.bases >> 16) // 2                                      # the slices inside the run yield no piece


RUN = 40_000_000


@pytest.fixture(scope="module", params=["seven", "head_opens_block", "block_inside_run"])
def across_super(request, oracle):
    """`seven`: 7 x symbol 2, ONE run of 40 000 000, then 100 000 short runs -- 2^25 falls inside the run.  With that prefix the run's few
    bytes sit at offsets 1 .. of block 0 and open no block.  The other two prefixes put a block start INTO the run's bytes, which is what
    makes the encoder answer a block that starts in an earlier super block than the segment (and, sliced, before the slice): 64
    one-position runs (the run's head byte opens block 1, at position 64) and 62 (its bytes straddle the block boundary, so Run::write
    splits it and block 1 starts inside the run)."""
    from test_gpu_parity import run_symbols
    rng = np.random.default_rng(23)
    tail = run_symbols(rng, 100000, [1, 2, 3, 5, 41, 42, 90])
    tail = tail[int(np.argmax(tail != 4)):]                   # the run must end where the tail begins
    singles = {"seven": 0, "head_opens_block": 64, "block_inside_run": 62}[request.param]
    prefix = np.full(7, 2, np.uint8) if singles == 0 else np.tile(np.array([2, 3], np.uint8), singles // 2)
    sym = np.concatenate([prefix, np.full(RUN, 4, np.uint8), tail])
    f = oracle.FMI.from_symbols(sym)
    be = f.samples[0]
    if singles:
        # block 1 starts inside [prefix, prefix + run), below 2^25, and ends behind 2^25
        assert prefix.size <= int(be[0]) + 1 < (1 << 25) < int(be[1]) and int(be[0]) + 1 < prefix.size + RUN
    return f, oracle.FMI.from_symbols(np.zeros(0, dtype=np.uint8))


@pytest.mark.parametrize("slice_records", [262144, 512])
def test_streamed_across_a_super_block(gpu, across_super, slice_records):
    """262 144 records: a cut exactly on the super boundary; 512: about 610 slices, most of them inside the run."""
    f, e = across_super
    check_streamed(gpu, inp(f), inp(e), f, slice_records)


def test_streamed_empty_inputs(gpu, oracle):
    from parts_inputs import odd_collection, truly_empty
    ta, tb = odd_collection("empty_b")                         # b is one "$"
    a, b = oracle.FMI.from_text(ta), oracle.FMI.from_text(tb)
    m, _ = oracle.merge(a.clone(), b.clone(), threads=2)
    check_streamed(gpu, inp(a), inp(b), m, 512)
    for which in ("a", "b"):
        a, b = truly_empty(oracle, which)
        m, _ = oracle.merge(a.clone(), b.clone(), threads=2)
        check_streamed(gpu, inp(a), inp(b), m, 512)
    e = oracle.FMI.from_text(np.zeros(0, dtype=np.uint8))      # nothing at all: one empty final piece
    for want in (0, 1, 2):
        pieces, out, stats = collect(gpu, inp(e), inp(e), 0, want)
        assert len(pieces) == 1 and pieces[0].last and pieces[0].nbytes == 0 and pieces[0].sample_blocks == 0
        assert (out.nbytes, out.blocks, out.bases, out.sequences) == (0, 0, 0, 0)


def test_streamed_after_a_chained_merge(gpu, oracle):
    """a kept on the device by a BWTM_RESULT_ON_DEVICE merge (records only), then streamed with a third input: the three-way merge."""
    sets = [oracle.generate_reads(4100 + k, 2500 + 300 * k, 100) for k in range(3)]
    fm = [oracle.FMI.from_text(t) for t in sets]
    direct = oracle.FMI.from_text(np.concatenate(sets))

    def kept():
        r = gpu.merge_host(inp(fm[0]), inp(fm[1]), samples=gpu.RESULT_ON_DEVICE, keep=True)
        k, r.keep = r.keep, None
        r.free()
        return k

    check_streamed(gpu, None, inp(fm[2]), direct, 1024, chained=kept)


def test_a_sink_that_stops_the_merge(gpu, reads):
    a, b, m, _ = reads
    seen = []

    def sink(piece):
        seen.append(piece)
        return len(seen) == 2

    with pytest.raises(gpu.BwtmError, match="sink"):
        gpu.capi.merge_host_streamed(inp(a), inp(b), 512, COMPACT, sink=sink)
    assert len(seen) == 2
    data, width, be, cum, out, stats = gpu.capi.merge_host_streamed(inp(a), inp(b), 512, FULL)     # right after: bit-exact
    obe, ocum = m.samples
    assert width == 8 and np.array_equal(data, m.data) and np.array_equal(be, obe) and np.array_equal(cum, ocum)

    def raising(piece):
        raise KeyError("from the sink")

    with pytest.raises(KeyError):
        gpu.capi.merge_host_streamed(inp(a), inp(b), 512, COMPACT, sink=raising)
    r = gpu.merge_host(inp(a), inp(b))                          # the one-shot call works in the same process afterwards
    assert np.array_equal(r.data, m.data)
    r.free()


def test_streamed_on_poisoned_memory(bwtm):
    """The read sets (1024) and long_runs (512) in a child per poison word: every block the library hands itself -- the slices' records,
    bytes, block starts and cum32, the pieces' staging, the carried block -- is filled with the word first.  The child compares with
    the oracle; here: both words give the same arrays, and fills were made."""
    digests = []
    for word in ("0x00000000", "0xA5A5A5A5"):
        out = subprocess.run([sys.executable, CHILD], cwd=ROOT, env=dict(os.environ, BWTM_POOL_POISON=word), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "OK" in out.stdout.split(), "%s: exit status %s\n%s%s" % (word, out.returncode, out.stdout[-3000:], out.stderr[-3000:])
        got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
        assert got and int(got.group(1)) > 0 and int(got.group(2)) >= 256 * int(got.group(1)), out.stdout[-3000:]
        digests.append(re.search(r"DIGEST (\w+)", out.stdout).group(1))
    assert digests[0] == digests[1]


def test_cli_streamed_flag_writes_the_same_files(bwtm, oracle, tmp_path):
    """bwt_merge with and without -z (two inputs, and a chain of three whose first merge stays on the device) writes byte-identical
    native files, verifies the same patterns after uploading the result again, and equals the oracle's BWT of the whole collection."""
    host = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")
    subprocess.check_call(["make", "-C", host, "-s"])
    chars = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    sets = [oracle.generate_reads(4200 + k, 900 + 100 * k, 100) for k in range(3)]
    names = []
    for k, t in enumerate(sets):
        names.append(str(tmp_path / ("in%d.plain" % k)))
        chars[oracle.FMI.from_text(t).symbols].tofile(names[-1])
    pats = [chars[t[p: p + 12]].tobytes().decode() for t in sets for p in (5, 1000, 30000) if np.all(t[p: p + 12] != 0)] + ["ACGTACGTACGTACGTACGT"]
    (tmp_path / "patterns.txt").write_text("\n".join(pats) + "\n")
    exe = os.path.join(host, "bwt_merge")
    for inputs in (names[:2], names):
        files = []
        for label, extra in (("oneshot", []), ("z512", ["-z", "512"]), ("z0", ["-z", "0"])):
            files.append(str(tmp_path / ("%s_%d.native" % (label, len(inputs)))))
            out = subprocess.run([exe] + extra + ["-i", "plain_default", "-v", str(tmp_path / "patterns.txt")] + inputs + [files[-1]], capture_output=True, text=True)
            assert out.returncode == 0 and "Verification successful" in out.stdout, out.stdout + out.stderr
        whole = [open(f, "rb").read() for f in files]
        assert whole[0] == whole[1] == whole[2] and len(whole[0]) > 1000
    direct = oracle.FMI.from_text(np.concatenate(sets))
    conv = subprocess.run([os.path.join(host, "bwt_convert"), "-i", "native", "-o", "plain_default", files[1], str(tmp_path / "all.plain")], capture_output=True, text=True)
    assert conv.returncode == 0, conv.stdout + conv.stderr
    assert np.array_equal(np.fromfile(tmp_path / "all.plain", dtype=np.uint8), chars[direct.symbols])
    bad = subprocess.run([exe, "-z", "100", "-i", "plain_default"] + names[:2] + [str(tmp_path / "bad.native")], capture_output=True, text=True)
    assert bad.returncode != 0 and "multiple of 512" in bad.stderr
