"""Every instantiation of k_build_recs and k_build_recs_chunk (kernels/transcode.hip.h) on the streams of tests/transcode_inputs.py: groups
whose density disagrees with the stream's average, blocks and runs placed on the kernel's window edges, runs at the fill thresholds,
degenerate last groups, and native bytes that Run::read decodes but Run::write never writes.

Every stream goes through recs_window in {0, 8192, 16384, 32768} x recs_uniform in {-1, 0, 1} x four entry points (the one-shot upload, a
borrowed device buffer with 0xFF behind the stream, the chunked upload at one and at five groups per chunk).  After every upload
bwtm_transcode_forms must show launches of exactly the instantiation the setting implies (at (0, 0): the class that
tests/test_transcode_inputs_host.py proves for the stream), and the index is compared with plain numpy over the symbols: extract of the whole
stream; rank of all six symbols and inverse_select at every record header, every window edge +- 1, run starts +- 1, 0, n and random
positions; C; and, where the native form is kept, the samples and the bytes.  All integers, bit for bit.  Also the child code of the
`transcode_forms` family of tests/poison_child.py."""
import numpy as np
import pytest

import transcode_inputs as ti
from streamed_child import FULL, collect, inp
from upload_streamed_child import DEFAULT_CHUNK, GROUP_BYTES, expected_chunks

pytestmark = pytest.mark.gpu

WINDOWS = (0, 8192, 16384, 32768)
UNIFORMS = (-1, 0, 1)
ENTRIES = ("upload", "borrowed", "streamed_1", "streamed_5")
SEEN = np.zeros(16, dtype=np.int64)                                  # launches per form over the whole module


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    yield bwtm
    bwtm.tune("recs_window", 0); bwtm.tune("recs_uniform", 0); bwtm.tune("upload_chunk", DEFAULT_CHUNK); bwtm.tune("stream_upload", 0)


class Case:
    """A stream and what plain numpy says about it at the probe positions; computed once, read only."""

    def __init__(self, orc, name):
        s = ti.Stream(orc, name)
        self.name, self.s = name, s
        self.data, self.sequences, self.bases, self.nbytes = s.data, s.sequences, s.bases, s.nbytes
        self.sym = s.symbols
        self.C = s.f.C
        self.samples = s.f.samples
        n = s.bases
        bs = s.block_starts()
        group_start = bs[:-1][::ti.GROUP]
        group_end = np.concatenate([group_start[1:], [n]])
        edges = [base + np.arange(0, end - base + 8192 + 1, 8192) for base, end in zip((group_start & ~np.int64(127)).tolist(), group_end.tolist())]
        edges = np.concatenate(edges)                               # (the edges of the 8192 window include those of the larger ones)
        starts = np.concatenate([[0], np.flatnonzero(self.sym[1:] != self.sym[:-1]) + 1])
        if starts.size > 20000:
            starts = starts[np.unique(np.concatenate([np.linspace(0, starts.size - 1, 20000).astype(np.int64), [0, starts.size - 1]]))]
        rng = np.random.default_rng(77)
        pos = np.concatenate([np.arange(0, n + 1, 128), edges - 1, edges, edges + 1, starts - 1, starts, starts + 1, [0, n], rng.integers(0, n + 1, 3000)])
        self.pos = np.unique(pos[(pos >= 0) & (pos <= n)]).astype(np.uint64)
        at = self.pos.astype(np.int64)
        self.want = np.zeros((6, at.size), dtype=np.int64)
        for c in range(6):
            self.want[c] = np.concatenate([[0], np.cumsum(self.sym == c)])[at]
        below = at < n
        self.ipos = self.pos[below]
        self.isym = self.sym[at[below]]
        self.irank = self.want[:, below][self.isym, np.arange(self.isym.size)]
        self.comps = [np.full(at.size, c, dtype=np.uint8) for c in range(6)]
        self.device = None

    def borrowed(self):
        """The bytes on the device with 64 bytes of 0xFF (continuation bytes of a long run) behind them."""
        import torch
        if self.device is None:
            self.host = np.concatenate([self.data, np.full(64, 0xFF, dtype=np.uint8)])
            self.device = torch.from_numpy(self.host).to("cuda:0")
            torch.cuda.synchronize()
        return self.device


_cases = {}


def case(orc, name):
    if name not in _cases:
        _cases[name] = Case(orc, name)
    return _cases[name]


def upload_under(pkg, c, window, uniform, entry):
    """One upload under the knobs, all restored afterwards: (index, chunks or None, launches per form of this upload alone)."""
    chunk = {"streamed_1": GROUP_BYTES, "streamed_5": 5 * GROUP_BYTES}.get(entry, DEFAULT_CHUNK)
    pkg.tune("recs_window", window); pkg.tune("recs_uniform", uniform); pkg.tune("upload_chunk", chunk)
    try:
        pkg.profile_reset()
        stats = None
        if entry == "upload":
            ix = pkg.Index.upload(c.data, c.sequences, c.bases)
        elif entry == "borrowed":
            ix = pkg.Index.from_device(c.borrowed().data_ptr(), c.nbytes, c.sequences, c.bases, borrow=True)
        else:
            ix, stats = pkg.Index.upload_streamed(c.data, c.sequences, c.bases)
        forms = np.array(pkg.transcode_forms(), dtype=np.int64)
    finally:
        pkg.tune("recs_window", 0); pkg.tune("recs_uniform", 0); pkg.tune("upload_chunk", DEFAULT_CHUNK)
    return ix, (None if stats is None else (stats.chunks, chunk)), forms


def check_forms(c, window, uniform, entry, chunks, forms):
    """Exactly the instantiation the setting implies was launched: once, or once per chunk."""
    chunked = entry.startswith("streamed")
    want_form = ti.form_index(chunked, *ti.dispatch(c.bases, c.nbytes, window, uniform))
    if (window, uniform) == (0, 0):
        assert want_form == ti.form_index(chunked, *ti.DEFAULT_CLASS[c.name])
    launches = 1
    if chunked:
        launches = expected_chunks(c.nbytes, chunks[1])[0]
        assert chunks[0] == launches
    want = np.zeros(16, dtype=np.int64); want[want_form] = launches
    assert np.array_equal(forms, want), (c.name, window, uniform, entry, forms.tolist(), want_form)


def check_index(ix, c, native):
    """The index against plain numpy over the symbols."""
    n = c.bases
    assert (ix.bases, ix.sequences) == (n, c.sequences) and np.array_equal(ix.C, c.C)
    assert np.array_equal(ix.extract(0, n), c.sym)
    for comp in range(6):
        got = ix.rank(c.pos, c.comps[comp]).astype(np.int64)
        if not np.array_equal(got, c.want[comp]):
            bad = np.flatnonzero(got != c.want[comp])
            raise AssertionError("rank of %d: %d of %d positions differ, first at %d: %d, numpy says %d" % (comp, bad.size, got.size, int(c.pos[bad[0]]), got[bad[0]], c.want[comp][bad[0]]))
    r, sym = ix.inverse_select(c.ipos)
    assert np.array_equal(sym, c.isym) and np.array_equal(r.astype(np.int64), c.irank)
    if native:
        assert (ix.nbytes, ix.blocks) == (c.nbytes, c.s.blocks)
        be, cum = ix.samples()
        assert np.array_equal(be, c.samples[0]) and np.array_equal(cum, c.samples[1])
        assert np.array_equal(ix.data(), c.data)
    else:
        assert (ix.nbytes, ix.blocks) == (0, 0)


def check_setting(pkg, c, window, uniform, entry):
    ix, chunks, forms = upload_under(pkg, c, window, uniform, entry)
    try:
        check_forms(c, window, uniform, entry, chunks, forms)
        try:
            check_index(ix, c, native=not entry.startswith("streamed"))
        except AssertionError as e:
            raise AssertionError("%s recs_window=%d recs_uniform=%d %s: %s" % (c.name, window, uniform, entry, e)) from None
    finally:
        ix.free()
    return forms


def check_stream(pkg, orc, name):
    c = case(orc, name)
    seen = np.zeros(16, dtype=np.int64)
    for window in WINDOWS:
        for uniform in UNIFORMS:
            for entry in ENTRIES:
                seen += check_setting(pkg, c, window, uniform, entry)
    if c.device is not None:
        pkg.synchronize()
        assert np.array_equal(c.device.cpu().numpy(), c.host)        # the borrowed buffer, its tail included, was only read
    return seen


@pytest.mark.parametrize("name", ti.STREAMS)
def test_every_form_on(gpu, oracle, name):
    seen = check_stream(gpu, oracle, name)
    SEEN[:] += seen
    assert np.count_nonzero(seen) == 12                               # 3 windows x 2 deposits x 2 upload paths (FILL or not: by the stream)


def merged_equals(r_data, r_be, r_cum, r_C, m):
    obe, ocum = m.samples
    assert np.array_equal(r_data, m.data) and np.array_equal(r_C, m.C)
    assert np.array_equal(r_be, obe) and np.array_equal(r_cum, ocum)


def test_merge_of_rewritten_and_canonical_inputs(gpu, oracle):
    """bwtm_merge_host of (rewritten A, canonical B), of (canonical A, rewritten B), and the streamed merge with chunked uploads of
    (rewritten A, rewritten B): the bytes, samples and C of the oracle's merge of the canonical pair."""
    A = case(oracle, "rewritten_reads")
    a = A.s.canonical
    b = oracle.FMI.from_text(ti.read_set(oracle, ti.READS_B))
    b_bytes = ti.rewritten(*ti.runs_of(b.symbols), seed=ti.READS_SEED + 1)
    assert not np.array_equal(b_bytes, b.data) and np.array_equal(oracle.FMI.from_native(b_bytes, b.sequences, b.bases).symbols, b.symbols)
    m, _ = oracle.merge(a.clone(), b.clone(), threads=2)
    rewritten_a, rewritten_b = (A.data, a.sequences, a.bases), (b_bytes, b.sequences, b.bases)
    for x, y in ((rewritten_a, inp(b)), (inp(a), rewritten_b)):
        r = gpu.merge_host(x, y, samples=1)
        try:
            assert (r.out.sequences, r.out.bases, r.out.nbytes, r.out.blocks) == (m.sequences, m.bases, m.nbytes, m.blocks)
            merged_equals(r.data, r.block_end, r.cum, r.C, m)
        finally:
            r.free()
    gpu.tune("stream_upload", 1); gpu.tune("upload_chunk", GROUP_BYTES)
    try:
        gpu.profile_reset()
        pieces, out, stats = collect(gpu, rewritten_a, rewritten_b, 1024, FULL)
        forms = gpu.transcode_forms()
    finally:
        gpu.tune("stream_upload", 0); gpu.tune("upload_chunk", DEFAULT_CHUNK)
    assert sum(forms[:8]) == 0 and sum(forms[8:]) == expected_chunks(A.nbytes, GROUP_BYTES)[0] + expected_chunks(b_bytes.size, GROUP_BYTES)[0]
    data, width, be, cum = gpu.capi.assemble_pieces(pieces, list(out.C))
    assert width == 8
    merged_equals(data, be, cum, np.array(list(out.C), dtype=np.uint64), m)


def test_all_sixteen_forms_were_seen(gpu, oracle):
    """Over the whole module every instantiation has run.  (When only a part of the module was selected, the two smallest streams of both
    density kinds go through the matrix first.)"""
    if np.count_nonzero(SEEN) < 16:
        for name in ("tail_three_blocks_in_last_group", "fill_thresholds"):
            SEEN[:] += check_stream(gpu, oracle, name)
    print("k_build_recs launches per form:", SEEN[:8].tolist(), " k_build_recs_chunk:", SEEN[8:].tolist())
    assert np.all(SEEN > 0), SEEN.tolist()
