"""Memory whose contents the library never defined, and memory it must not touch.

1. The parity cases on POISONED device memory.  DevBuf::alloc does not zero unless asked, a fresh hipMalloc block is usually zero and a
recycled block of the same size holds the bytes of the same buffer of the previous call, so a kernel that reads a record plane, a tile word
or a table entry nobody wrote passes every other test.  With BWTM_POOL_POISON=<word> every block the library hands itself (the pool's, and the
parts' exported arena) is filled with the word first.  The library reads the variable once per process: every case is one child
(tests/poison_child.py FAMILY), which compares bit for bit with the CPU oracle; the parent demands exit status 0, "OK", and a fill count
above 0 from bwtm_pool_poison_stats -- a misspelt variable cannot pass with nothing checked.  Two words: 0x00000000 (code that relies on
left-over 0xFF of the `bound` tables or on left-over non-zero tags of the one-launch scans) and 0xA5A5A5A5 (everything that relies on
zeros); two pool shapes: the default, and every buffer of 64 KiB and more as a mapped block rounded up to 2 MiB (the largest unwritten tails).

2. GUARDS of 4096 bytes of 0xA5 on both sides of every caller-visible buffer, in this process and without poison: the guards are intact
afterwards and the region between them holds the oracle's answer."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CHILD = os.path.join(ROOT, "tests", "poison_child.py")
POOLS = {"default_pool": {}, "mapped_2mib": {"BWTM_POOL_VMM_CHUNK": "2097152", "BWTM_POOL_VMM_MIN": "65536"}}
FAMILIES = ["reads", "odd", "runs", "encoder", "epochs", "host", "slices", "parts", "ingest", "transcode_forms"]
MAPPED_TOO = ["reads", "odd", "runs", "parts"]
CASES = [(f, w, "default_pool") for f in FAMILIES for w in ("0x00000000", "0xA5A5A5A5")] + [(f, w, "mapped_2mib") for f in MAPPED_TOO for w in ("0x00000000", "0xA5A5A5A5")]


def run_child(family, env):
    out = subprocess.run([sys.executable, CHILD, family], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), "%s %s: exit status %s\n%s%s" % (family, env, out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
    assert got, out.stdout[-3000:]
    return int(got.group(1)), int(got.group(2))


@pytest.mark.parametrize("family,word,pool", CASES)
def test_parity_on_poisoned_memory(bwtm, family, word, pool):
    fills, nbytes = run_child(family, dict(POOLS[pool], BWTM_POOL_POISON=word))
    assert fills > 0 and nbytes >= 256 * fills, (fills, nbytes)


@pytest.mark.parametrize("word", ["0x00000000", "0xA5A5A5A5"])
@pytest.mark.parametrize("family", ["exact_builders", "exact_merges"])
def test_exact_sizes_on_poisoned_memory(bwtm, family, word):
    """The small builder and merge cases of tests/test_gpu_exact_sizes.py once more on poisoned memory: at sizes that are a multiple of a
    record, a chunk or a segment, the last unit holds no position and is the one nobody may have written."""
    fills, nbytes = run_child(family, dict(BWTM_POOL_POISON=word))
    assert fills > 0 and nbytes >= 256 * fills, (fills, nbytes)


def test_poison_mode_is_off_by_default_and_counted_when_on(bwtm):
    """The proof of activity proves something: without the variable (or with a misspelt one) the child reports no fill at all."""
    env = {k: v for k, v in os.environ.items() if k != "BWTM_POOL_POISON"}
    out = subprocess.run([sys.executable, CHILD, "ingest"], cwd=ROOT, env=dict(env, BWTM_POOL_POISSON="0xA5A5A5A5"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), out.stdout[-3000:] + out.stderr[-3000:]
    assert "POISON fills=0 bytes=0" in out.stdout, out.stdout[-3000:]


# ------------------------------------------------------------------------------------------------------------------------------------
# Guards

GUARD = 4096


class Guarded:
    """`nbytes` of host memory between two guards; .region is what the callee may write, .ptr its address."""

    def __init__(self, nbytes, dtype=np.uint8):
        self.nbytes = int(nbytes)
        self.buf = np.full(self.nbytes + 2 * GUARD, 0xA5, dtype=np.uint8)
        self.region = self.buf[GUARD: GUARD + self.nbytes].view(dtype)
        self.ptr = self.buf.ctypes.data + GUARD
        assert self.ptr % 16 == 0

    def p(self, ctype):
        return C.cast(C.c_void_p(self.ptr), C.POINTER(ctype))

    def assert_intact(self, written=None):
        """Nothing before the region and nothing behind its first `written` bytes (default: all of it) has changed."""
        written = self.nbytes if written is None else int(written)
        assert written <= self.nbytes
        assert np.all(self.buf[:GUARD] == 0xA5), "bytes before the buffer were written"
        assert np.all(self.buf[GUARD + written:] == 0xA5), "bytes behind the buffer were written"


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    bwtm.tune("search_algo", 0)
    yield bwtm
    bwtm.tune("search_algo", 0)


@pytest.fixture(scope="module")
def reads(oracle):
    """The `reads` pair of the poisoned cases and the oracle's answers about it, computed once (read only)."""
    from poison_child import READS
    ta = oracle.generate_reads(*READS[0]); tb = oracle.generate_reads(*READS[1])
    a, b = oracle.FMI.from_text(ta), oracle.FMI.from_text(tb)
    m, _ = oracle.merge(a.clone(), b.clone(), threads=2)
    ranks, counts, _ = oracle.search(a, b, threads=2)
    return {"ta": ta, "tb": tb, "a": a, "b": b, "m": m, "ranks": ranks, "counts": counts, "ra": oracle.ra_from_runs(ranks, counts)}


def test_host_outputs_stay_inside_their_buffers(gpu, reads):
    """bwtm_index_download_data (capacity > nbytes), bwtm_ra_download, bwtm_ra_download_bits, bwtm_ra_download_runs, bwtm_extract and
    bwtm_index_download_samples, each into a buffer with more room than it needs: the call writes what the contract names and nothing else.
    (The binding's own wrappers allocate the arrays; the calls go through the same ctypes prototypes with the guarded addresses.)"""
    lib = gpu.capi.lib()
    a, b, m = reads["a"], reads["b"], reads["m"]
    A = gpu.Index.upload(a.data, a.sequences, a.bases); B = gpu.Index.upload(b.data, b.sequences, b.bases)
    ra = gpu.RankArray(A, B)
    ra.search(A, B, 0, b.sequences - 1)
    ra.finalize()
    u64, u8 = C.c_uint64, C.c_uint8

    g = Guarded(b.bases * 8, np.uint64)
    gpu.capi.check(lib.bwtm_ra_download(ra.h, g.p(u64), b.bases + GUARD // 8))
    g.assert_intact(); assert np.array_equal(g.region, reads["ra"])

    words = (a.bases + b.bases + 63) // 64
    g = Guarded(words * 8, np.uint64)
    gpu.capi.check(lib.bwtm_ra_download_bits(ra.h, g.p(u64), words + GUARD // 8))
    g.assert_intact()
    expect = np.zeros(words * 64, dtype=np.uint8)
    expect[np.arange(b.bases, dtype=np.uint64) + reads["ra"]] = 1
    assert np.array_equal(np.unpackbits(g.region.view(np.uint8), bitorder="little"), expect)

    nruns = reads["ranks"].size
    gr, gc = Guarded(nruns * 8, np.uint64), Guarded(nruns * 8, np.uint64)
    n = u64(0)
    gpu.capi.check(lib.bwtm_ra_download_runs(ra.h, gr.p(u64), gc.p(u64), nruns + GUARD // 8, C.byref(n)))
    assert n.value == nruns
    gr.assert_intact(); gc.assert_intact()
    assert np.array_equal(gr.region, reads["ranks"]) and np.array_equal(gc.region, reads["counts"])

    M = gpu.interleave(A, B, ra)
    sym = m.symbols
    for first, count in ((0, 1), (12345, 100001), (sym.size - 129, 129), (0, sym.size)):
        g = Guarded(count)
        gpu.capi.check(lib.bwtm_extract(M.h, first, count, g.p(u8)))
        g.assert_intact(); assert np.array_equal(g.region, sym[first: first + count])

    M.encode()
    assert M.nbytes == m.nbytes and M.blocks == m.blocks
    g = Guarded(m.nbytes)
    gpu.capi.check(lib.bwtm_index_download_data(M.h, g.p(u8), m.nbytes + GUARD))
    g.assert_intact(); assert np.array_equal(g.region, m.data)

    obe, ocum = m.samples
    gb, gc = Guarded(m.blocks * 8, np.uint64), Guarded(6 * (m.blocks + 1) * 8, np.uint64)
    gpu.capi.check(lib.bwtm_index_download_samples(M.h, gb.p(u64), gc.p(u64)))
    gb.assert_intact(); gc.assert_intact()
    assert np.array_equal(gb.region, obe) and np.array_equal(gc.region.reshape(6, m.blocks + 1), ocum)
    for x in (ra, M, A, B):
        x.free()


@pytest.mark.parametrize("chunks", [(0, 0), (8192, 4096)])
def test_merge_host_fills_the_callers_buffers_and_nothing_else(gpu, reads, chunks):
    """The buffers bwtm_merge_host's allocation callback returns are pre-filled: every byte up to the reported sizes is written (it equals
    the oracle's) and nothing behind them, also when the download runs in many small chunks."""
    capi = gpu.capi
    a, b, m = reads["a"], reads["b"], reads["m"]
    handed = {}

    def alloc(user, what, nbytes):
        handed[what] = Guarded(nbytes)
        return handed[what].ptr

    cb = capi.ALLOC_FN(alloc)
    da, db = a.data, b.data                                     # (the oracle's properties return fresh arrays: kept alive across the call)
    ha, hb = capi._host_input(da, a.sequences, a.bases), capi._host_input(db, b.sequences, b.bases)
    out = capi.HostOutput()
    gpu.tune("upload_chunk", chunks[0]); gpu.tune("download_chunk", chunks[1])
    try:
        capi.check(capi.lib().bwtm_merge_host(C.byref(ha), C.byref(hb), cb, None, 1, C.byref(out), None))
    finally:
        gpu.tune("upload_chunk", 0); gpu.tune("download_chunk", 0)
    assert (out.nbytes, out.blocks, out.sequences, out.bases, out.sample_width) == (m.nbytes, m.blocks, m.sequences, m.bases, 8)
    assert sorted(handed) == [0, 1, 2]
    assert (out.data, out.block_end, out.cum) == (handed[0].ptr, handed[1].ptr, handed[2].ptr)
    obe, ocum = m.samples
    for what, expect in ((0, m.data), (1, obe), (2, ocum.reshape(-1))):
        g = handed[what]
        nbytes = expect.size * expect.dtype.itemsize
        g.assert_intact(written=nbytes)
        assert np.array_equal(g.buf[GUARD: GUARD + nbytes].view(expect.dtype), expect), what


def test_search_finalize_and_interleave_stay_inside_a_callers_bitvector(gpu, reads):
    """A caller-owned rank-array buffer (bwtm_ra_create_on) of exactly bwtm_ra_buffer_bytes between two guards, under every dispatch of
    the search: where an out-of-range store of the tile builds or of the atomicOr fallback would land."""
    import torch
    a, b, m = reads["a"], reads["b"], reads["m"]
    A = gpu.Index.upload(a.data, a.sequences, a.bases); B = gpu.Index.upload(b.data, b.sequences, b.bases)
    nbytes = gpu.ra_buffer_bytes(A, B)
    try:
        for st in (dict(search_algo=2), dict(search_algo=2, range_ratio=0), dict(search_algo=1), dict(search_algo=0), dict(search_algo=1, emit_path=1)):
            for k, v in st.items():
                gpu.tune(k, v)
            t = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
            t[GUARD: GUARD + nbytes] = 0
            torch.cuda.synchronize()
            ra = gpu.RankArray(A, B, t.data_ptr() + GUARD, nbytes)
            ra.search(A, B, 0, b.sequences - 1)
            ra.finalize()
            assert ra.values == b.bases and np.array_equal(ra.download(), reads["ra"]), st
            M = gpu.interleave(A, B, ra).encode()
            assert np.array_equal(M.data(), m.data), st
            gpu.synchronize()
            host = t.cpu().numpy()
            assert np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + nbytes:] == 0xA5), st
            M.free(); ra.free()
            for k in st:
                gpu.tune(k, -1 if k == "range_ratio" else 0)
    finally:
        gpu.tune("search_algo", 0); gpu.tune("range_ratio", -1); gpu.tune("emit_path", 0)
    A.free(); B.free()


def test_device_inputs_are_read_only(gpu, oracle, reads):
    """The buffer of bwtm_index_from_device_borrowed, its garbage tail included, and the rows given to the builder's device-pointer add
    hold the same bytes after the index / the builder has been used and freed."""
    import torch
    a, b, m = reads["a"], reads["b"], reads["m"]
    host = np.full(GUARD + a.nbytes + GUARD, 0xFF, dtype=np.uint8)             # 0xFF = continuation bytes of a long run
    host[GUARD: GUARD + a.nbytes] = a.data
    buf = torch.from_numpy(host).to("cuda:0")
    A = gpu.Index.from_device(buf.data_ptr() + GUARD, a.nbytes, a.sequences, a.bases, borrow=True)
    B = gpu.Index.upload(b.data, b.sequences, b.bases)
    assert np.array_equal(A.data(), a.data) and np.array_equal(A.C, a.C)
    M = gpu.merge(A, B)
    assert np.array_equal(M.data(), m.data)
    for x in (M, A, B):
        x.free()
    gpu.synchronize()
    assert np.array_equal(buf.cpu().numpy(), host)

    n, L = 3000, 100
    rows = reads["ta"].reshape(n, L + 1)
    padded = np.full((n + 2 * GUARD // (L + 1) + 2, L + 1), 0xA5, dtype=np.uint8)
    first = GUARD // (L + 1) + 1
    padded[first: first + n] = rows
    t = torch.from_numpy(padded).to("cuda:0")
    bld = gpu.Builder(512)
    bld.add_device(t.data_ptr() + first * (L + 1), n, L, stride=L + 1)
    X = bld.finish()
    assert np.array_equal(X.extract(0, X.bases), a.symbols)
    X.free()
    gpu.synchronize()
    assert np.array_equal(t.cpu().numpy(), padded)
