"""bwtm_index_upload_streamed: the index from chunks of the native bytes through a ring of chunk buffers, the running position and symbol
counts carried on the device, the header validated once at the end.  Against plain symbols and the oracle's bytes at every chunk size,
at the edges of a chunk, across a super block, with bounded staging, on bytes that contradict their header, inside the streamed merge
(the stream_upload knob) and on poisoned device memory.  The inputs and checks live in tests/upload_streamed_child.py, which is also
the child process of the poisoned run."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from streamed_child import check_streamed, inp, read_sets
from test_gpu_parity import check_index, run_symbols
from upload_streamed_child import (CHUNKS, DEFAULT_CHUNK, EDGE_NAMES, GROUP_BYTES, MIXES, check_edge_shape, check_upload, edge_shapes, mix_symbols,
                                   upload_streamed)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "upload_streamed_child.py")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    yield bwtm
    bwtm.tune("upload_chunk", DEFAULT_CHUNK); bwtm.tune("recs_uniform", 0); bwtm.tune("stream_upload", 0)


_mixes = {}


def mix(oracle, k):
    """The symbols of mix k and the oracle's FMI of them, computed once (read only)."""
    if k not in _mixes:
        sym = mix_symbols(k)
        _mixes[k] = (sym, oracle.FMI.from_symbols(sym))
    return _mixes[k]


@pytest.mark.parametrize("uniform", [0, 1, -1])
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("k", range(len(MIXES)))
def test_parity_against_plain_symbols(gpu, oracle, k, chunk, uniform):
    sym, f = mix(oracle, k)
    assert f.nbytes > GROUP_BYTES                                  # more than one chunk at the smallest chunk size
    check_upload(gpu, f, sym, np.random.default_rng(1), chunk, uniform)


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_chunk_edge_shapes(gpu, oracle, name):
    name, sym, nbytes = next(s for s in edge_shapes() if s[0] == name)
    check_edge_shape(gpu, oracle, name, sym, nbytes, np.random.default_rng(2))


RUN = 40_000_000


@pytest.fixture(scope="module")
def across_super(oracle):
    """The shape of across_super in test_gpu_streamed_merge.py: a short prefix, ONE run of 40 000 000, then 100 000 short runs.  2^25 falls
    inside a run that began in chunk 0; the supers from 1 on belong to positions reached in later chunks.  With the runs' starts and the
    symbol counts before every run: ranks by run arithmetic, no 6 x n table."""
    rng = np.random.default_rng(23)
    tail = run_symbols(rng, 100000, [1, 2, 3, 5, 41, 42, 90])
    tail = tail[int(np.argmax(tail != 4)):]
    sym = np.concatenate([np.full(7, 2, np.uint8), np.full(RUN, 4, np.uint8), tail])
    f = oracle.FMI.from_symbols(sym)
    starts = np.concatenate([[0], np.flatnonzero(sym[1:] != sym[:-1]) + 1]).astype(np.int64)
    lens = np.diff(np.concatenate([starts, [sym.size]]))
    rsym = sym[starts]
    before = np.zeros((6, starts.size), dtype=np.int64)            # occurrences of c before the run
    for c in range(6):
        before[c, 1:] = np.cumsum(np.where(rsym == c, lens, 0))[:-1]
    assert (starts[1], lens[1], rsym[1]) == (7, RUN, 4) and starts[1] < (1 << 25) < starts[2]
    return sym, f, starts, rsym, before


@pytest.mark.parametrize("chunk", [GROUP_BYTES, DEFAULT_CHUNK])
def test_across_a_super_block(gpu, across_super, chunk):
    sym, f, starts, rsym, before = across_super
    n = sym.size
    rng = np.random.default_rng(3)
    ix, stats = upload_streamed(gpu, f, chunk)
    try:
        assert stats.chunks == (-(-f.blocks // 62) if chunk else 1) and (ix.bases, ix.sequences, ix.nbytes) == (n, f.sequences, 0)
        assert np.array_equal(ix.C, f.C)
        special = [0, 7, 8, (1 << 25) - 1, 1 << 25, (1 << 25) + 1, 7 + RUN - 1, 7 + RUN, 7 + RUN + 1, n - 1, n]
        pos = np.concatenate([rng.integers(0, n + 1, 2000), rng.integers(7 + RUN, n + 1, 2000), special]).astype(np.int64)
        run = np.searchsorted(starts, pos, side="right") - 1        # the run that holds position p (p = n: the last run, all of it)
        for c in range(6):
            want = before[c, run] + np.where(rsym[run] == c, pos - starts[run], 0)
            got = ix.rank(pos.astype(np.uint64), np.full(pos.size, c, dtype=np.uint8))
            assert np.array_equal(got.astype(np.int64), want), c
        for end in (7, 7 + RUN):
            first = max(end - 150, 0)
            assert np.array_equal(ix.extract(first, 300), sym[first: first + 300])
        assert np.array_equal(ix.extract(n - 300, 300), sym[n - 300:])
        ipos = pos[pos < n]
        r, c = ix.inverse_select(ipos.astype(np.uint64))
        irun = np.searchsorted(starts, ipos, side="right") - 1
        assert np.array_equal(c, sym[ipos]) and np.array_equal(r.astype(np.int64), before[sym[ipos], irun] + ipos - starts[irun])
        ix.encode()
        assert ix.nbytes == f.nbytes and np.array_equal(ix.data(), f.data)
        be, cum = ix.samples()
        assert np.array_equal(be, f.samples[0]) and np.array_equal(cum, f.samples[1])
    finally:
        ix.free()


def test_bounded_staging(gpu, oracle):
    """17 chunks of five groups: what the call holds besides the records and the super table does not grow with the stream (holding the
    stream whole would be 17 chunks, eight times the bound's 4 chunks + 64 KiB of the pool's rounding)."""
    rng = np.random.default_rng(4)
    sym = run_symbols(rng, 330000, [1, 1, 2, 3])
    f = oracle.FMI.from_symbols(sym)
    ngroups = -(-f.blocks // 62)
    assert ngroups >= 5 * 16
    stats = check_upload(gpu, f, sym, rng, 5 * GROUP_BYTES)
    assert stats.chunks == -(-ngroups // 5) and stats.chunk_bytes == 5 * GROUP_BYTES
    assert stats.staging_bytes_peak <= 4 * stats.chunk_bytes + 65536 and f.nbytes > 2 * (4 * stats.chunk_bytes + 65536)


def short_block():
    """64 bytes that encode ONE run of 42 positions: the head of a long run of symbol 1 and 63 redundant continuation bytes."""
    return np.array([247] + [0x80] * 62 + [0x00], dtype=np.uint8)


def test_untrusted_bytes(gpu, oracle):
    """Bytes that contradict their header: the streamed upload refuses them with the one-shot upload's verdict, word for word, and a correct
    upload right after is exact.  The stores are bounded by what the header allocated, whatever the bytes say."""
    rng = np.random.default_rng(5)
    sym = run_symbols(rng, 20000, [1, 2, 3])
    f = oracle.FMI.from_symbols(sym)
    assert f.blocks > 5 * 62                                        # six chunks of one group
    other_sym = run_symbols(rng, 9000, [1, 2, 3, 50])
    other = oracle.FMI.from_symbols(other_sym)
    wrong_C = f.C.copy(); wrong_C[3] += 1
    spoiled = []
    for block in (3, 3 * 62 + 5):                                   # in the first chunk and in a later one
        data = f.data.copy()
        data[64 * block: 64 * block + 64] = short_block()
        spoiled.append(data)
    cases = [("bases - 1", f.data, f.sequences, f.bases - 1, None), ("half the bases", f.data, f.sequences, f.bases // 2, None),
             ("bases + 1000", f.data, f.sequences, f.bases + 1000, None), ("sequences", f.data, f.sequences + 1, f.bases, None),
             ("C", f.data, f.sequences, f.bases, wrong_C), ("short block, first chunk", spoiled[0], f.sequences, f.bases, None),
             ("short block, later chunk", spoiled[1], f.sequences, f.bases, None)]
    for name, data, sequences, bases, C_array in cases:
        with pytest.raises(gpu.BwtmError) as oneshot:
            gpu.Index.upload(data, sequences, bases, C_array)
        gpu.tune("upload_chunk", GROUP_BYTES)
        try:
            with pytest.raises(gpu.BwtmError) as streamed:
                gpu.Index.upload_streamed(data, sequences, bases, C_array)
        finally:
            gpu.tune("upload_chunk", DEFAULT_CHUNK)
        print("%s: %s" % (name, streamed.value))
        assert str(streamed.value) == str(oneshot.value), name
        if name.startswith("short block"):
            assert "canonical" in str(streamed.value)
        ix, _ = upload_streamed(gpu, other, GROUP_BYTES)
        try:
            check_index(ix, other_sym, rng, nq=1000)
        finally:
            ix.free()


@pytest.fixture(scope="module")
def reads(gpu, oracle):
    a, b, m = read_sets(oracle)
    r = gpu.merge_host(inp(a), inp(b), samples=2)
    assert r.out.sample_width in (1, 2, 4) and np.array_equal(r.data, m.data)
    oneshot = (r.out.sample_width, r.fields.copy(), r.anchors.copy())
    r.free()
    return a, b, m, oneshot


@pytest.mark.parametrize("slice_records", [512, 0])
def test_streamed_merge_with_chunked_uploads(gpu, reads, slice_records):
    a, b, m, oneshot = reads
    gpu.tune("stream_upload", 1); gpu.tune("upload_chunk", GROUP_BYTES)
    try:
        check_streamed(gpu, inp(a), inp(b), m, slice_records, oneshot=oneshot)
    finally:
        gpu.tune("stream_upload", 0); gpu.tune("upload_chunk", DEFAULT_CHUNK)


def test_chained_streamed_merge_with_a_chunked_upload(gpu, oracle):
    """a kept on the device stays as it is; b goes through the chunked upload."""
    sets = [oracle.generate_reads(4100 + k, 2500 + 300 * k, 100) for k in range(3)]
    fm = [oracle.FMI.from_text(t) for t in sets]
    direct = oracle.FMI.from_text(np.concatenate(sets))

    def kept():
        r = gpu.merge_host(inp(fm[0]), inp(fm[1]), samples=gpu.RESULT_ON_DEVICE, keep=True)
        k, r.keep = r.keep, None
        r.free()
        return k

    gpu.tune("stream_upload", 1); gpu.tune("upload_chunk", GROUP_BYTES)
    try:
        check_streamed(gpu, None, inp(fm[2]), direct, 1024, chained=kept)
    finally:
        gpu.tune("stream_upload", 0); gpu.tune("upload_chunk", DEFAULT_CHUNK)


def test_on_poisoned_memory(bwtm):
    """One mix at three chunk sizes and the chunk-edge shapes in a child whose pool fills every block it hands out with 0xA5A5A5A5: a
    record at a chunk border that nobody wrote cannot pass by luck."""
    out = subprocess.run([sys.executable, CHILD], cwd=ROOT, env=dict(os.environ, BWTM_POOL_POISON="0xA5A5A5A5"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), "exit status %s\n%s%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
    assert got and int(got.group(1)) > 0 and int(got.group(2)) >= 256 * int(got.group(1)), out.stdout[-3000:]
