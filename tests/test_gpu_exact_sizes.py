"""Indexes whose SIZE lands exactly on a unit of the device structure (tests/boundary_inputs.py; tests/test_boundary_inputs_host.py proves
that every input has the size it is named after): a record (128 positions: num_records(n) = (n >> 7) + 1 leaves a last record without a
position), a transcode group (3968 bytes), a bitvector chunk (8192), an encoder segment (65 536), a super row (2^25), an ingest tile (4096
suffixes).  Every builder of records and super table -- k_build_recs / k_build_sup (upload, borrowed buffer), k_build_sup_chunk (streamed
upload), k_sym_sup (from symbols, ingest leaves), k_interleave / k_interleave_sup (merge), k_interleave_sup_window (slices, parts) -- at
every such size, every form of the merge at every exact n_out, and the consumers (find, sequences, locate) on the results.  Expected values
are the oracle's or plain numpy on the test's own symbols and reads, never the library's.  The check functions take the library and the
oracle as arguments: tests/poison_child.py runs the small cases once more on poisoned device memory."""
import numpy as np
import pytest

import boundary_inputs as bi
from locate_inputs import locate_raw, suffix_order
from parts_inputs import merge_parts
from streamed_child import check_streamed, inp
from test_gpu_ingest import check_against_oracle as check_ingest
from test_gpu_parity import check_index, cum_counts
from test_gpu_second_half_forms import check_index_by_probes
from test_gpu_slices import sliced_result
from upload_streamed_child import DEFAULT_CHUNK, GROUP_BYTES, expected_chunks, upload_streamed

pytestmark = pytest.mark.gpu

BUILDERS = ("upload", "upload_streamed", "borrowed", "from_symbols")
SUPER_BUILDERS = ("upload", "upload_streamed", "from_symbols")
FORMS = ("staged", "merge", "host", "sliced", "streamed", "parts")
FILL = 0xEEEEEEEEEEEEEEEE


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    bwtm.tune("ingest_verify", 1)
    yield bwtm
    bwtm.tune("ingest_verify", 0); bwtm.tune("search_algo", 0); bwtm.tune("upload_chunk", DEFAULT_CHUNK)
    bwtm.trim()


# ------------------------------------------------------------------------------------------------------------------------------------
# Checks shared with the poisoned run

def built(gpu, f, sym, builder, chunk=GROUP_BYTES):
    """-> (index, what it borrows): the index of the oracle FMI f / the symbols sym through one of the four single-index builders."""
    import torch
    if builder == "upload":
        return gpu.Index.upload(f.data, f.sequences, f.bases), None
    if builder == "upload_streamed":                                     # chunks of whole groups: every chunk ends on a block end
        ix, stats = upload_streamed(gpu, f, chunk)
        assert (stats.chunks, stats.chunk_bytes) == expected_chunks(f.nbytes, chunk)
        return ix, None
    if builder == "borrowed":
        host = np.full(f.nbytes + 64, 0xFF, dtype=np.uint8)                # 0xFF = continuation bytes of a long run
        host[: f.nbytes] = f.data
        buf = torch.from_numpy(host).to("cuda:0")
        return gpu.Index.from_device(buf.data_ptr(), f.nbytes, f.sequences, f.bases, borrow=True), buf
    assert builder == "from_symbols"
    d = torch.from_numpy(np.ascontiguousarray(sym)).to("cuda:0")
    torch.cuda.synchronize()
    return gpu.Index.from_symbols_device(d.data_ptr(), sym.size), d


def check_every_position(ix, sym):
    """rank of all six symbols at EVERY position 0 .. n and inverse_select at every position 0 .. n - 1, against plain counts."""
    n = sym.size
    cum = cum_counts(sym)
    pos = np.arange(n + 1, dtype=np.uint64)
    for c in range(6):
        assert np.array_equal(ix.rank(pos, np.full(pos.size, c, dtype=np.uint8)).astype(np.int64), cum[c]), c
    r, c = ix.inverse_select(pos[:n])
    assert np.array_equal(c, sym) and np.array_equal(r.astype(np.int64), cum[sym, np.arange(n)])


def check_find_edges(ix, f, sym):
    """bwtm_find_batch where its last LF step queries rank(n): the empty pattern, the largest symbol present (its range ends at n - 1)
    once and twice, patterns with a 0, against the oracle's FMI.find, compared as in test_find_batch_matches_oracle_backward_search.
    A code >= 6 is outside the oracle's C array (its find would read behind it); no symbol of the index equals it, so its range is empty."""
    n = sym.size
    top = int(sym.max())
    pats = [[], [top], [top, top], [top, top, top], [0], [1, 0], [0, 2], [2, 0, 3], [top, 0], [0, top]]
    sp, ep = ix.find([np.array(p, dtype=np.uint8) for p in pats])
    assert (int(sp[0]), int(ep[0])) == (0, n - 1) and f.find(np.array([top], dtype=np.uint8))[1] == n - 1
    for k, p in enumerate(pats):
        osp, oep = f.find(np.array(p, dtype=np.uint8))
        empty_o = (osp + 1) % (1 << 64) > (oep + 1) % (1 << 64)
        empty_g = (int(sp[k]) + 1) % (1 << 64) > (int(ep[k]) + 1) % (1 << 64)
        assert empty_o == empty_g, (k, p)
        assert empty_o or (int(sp[k]), int(ep[k])) == (osp, oep), (k, p)
    foreign = [[6], [1, 6, 2], [7, top], [top, 200], [255]]
    sp, ep = ix.find([np.array(p, dtype=np.uint8) for p in foreign])
    for k, p in enumerate(foreign):
        assert (int(sp[k]) + 1) % (1 << 64) > (int(ep[k]) + 1) % (1 << 64), (k, p)


def check_native(ix, f):
    assert (ix.nbytes, ix.blocks) == (f.nbytes, f.blocks) and np.array_equal(ix.data(), f.data)
    be, cum = ix.samples()
    obe, ocum = f.samples
    assert np.array_equal(be, obe) and np.array_equal(cum, ocum)


def check_small_builder(gpu, oracle, kind, n, builder):
    """One small stream through one builder: sizes and C, check_index's probes (n - 1, n, n + 5, a comp >= 6), every position, the
    samples, and the bytes and samples the encoder makes of the records alone."""
    sym = bi.small_stream(kind, n)
    f = oracle.FMI.from_symbols(sym)
    ix, borrowed = built(gpu, f, sym, builder)
    try:
        assert (ix.bases, ix.sequences) == (n, f.sequences) and np.array_equal(ix.C, f.C)
        check_index(ix, sym, np.random.default_rng(n), nq=64)
        check_every_position(ix, sym)
        check_find_edges(ix, f, sym)
        if builder in ("upload", "borrowed"):
            check_native(ix, f)                                          # the samples of the upload itself
        ix.drop_native()                                                 # the records alone from here on (and no claim on a borrowed buffer)
        assert (ix.nbytes, ix.blocks) == (0, 0)
        ix.encode()
        check_native(ix, f)
        check_every_position(ix, sym)
    finally:
        ix.free()
        del borrowed


class PairCase:
    """One read pair: the reads, the oracle's FMIs, rank array and merge, the BWT of the concatenated text, and the uploaded inputs."""

    def __init__(self, gpu, oracle, name):
        self.name = name
        (ra, la), (rb, lb) = bi.read_pair(oracle, name)
        self.rows, self.lengths = np.concatenate([ra, rb]), np.concatenate([la, lb])
        self.reads_a, self.reads_b = (ra, la), (rb, lb)
        ta, tb = bi.text_of(ra, la), bi.text_of(rb, lb)
        self.a, self.b = oracle.FMI.from_text(ta), oracle.FMI.from_text(tb)
        self.n = self.a.bases + self.b.bases
        assert self.n == bi.N_OUT[name]
        self.m, _ = oracle.merge(self.a.clone(), self.b.clone(), threads=2)
        direct = oracle.FMI.from_text(np.concatenate([ta, tb]))            # the BWT of the concatenated text
        assert np.array_equal(self.m.data, direct.data) and np.array_equal(self.m.C, direct.C)
        assert np.array_equal(self.m.samples[0], direct.samples[0]) and np.array_equal(self.m.samples[1], direct.samples[1])
        self.ranks, self.counts, _ = oracle.search(self.a, self.b, threads=2)
        self.sym = self.m.symbols
        self.obe, self.ocum = self.m.samples
        self.A = gpu.Index.upload(*inp(self.a)); self.B = gpu.Index.upload(*inp(self.b))
        self._order = None

    def free(self):
        self.A.free(); self.B.free()

    def order(self):
        if self._order is None:
            self._order = suffix_order(self.rows, self.lengths)
        return self._order

    def searched(self, gpu):
        ra = gpu.RankArray(self.A, self.B)
        ra.search(self.A, self.B, 0, self.b.sequences - 1)
        ra.finalize()
        assert ra.values == self.b.bases
        ranks, counts = ra.runs()
        assert np.array_equal(ranks, self.ranks) and np.array_equal(counts, self.counts)
        return ra

    def check_laid_out(self, data, be, cum, blocks=None):
        """Bytes and samples laid end to end (cum with or without the column behind the last block)."""
        assert data.dtype == np.uint8 and np.array_equal(data, self.m.data)
        assert np.array_equal(be, self.obe)
        assert np.array_equal(cum, self.ocum if cum.shape[1] == self.ocum.shape[1] else self.ocum[:, :-1])
        assert blocks is None or blocks == self.m.blocks

    def check_index(self, M):
        m = self.m
        assert (M.sequences, M.bases, M.nbytes, M.blocks) == (m.sequences, m.bases, m.nbytes, m.blocks) and np.array_equal(M.C, m.C)
        self.check_laid_out(M.data(), *M.samples())


def check_sequences_and_locations(gpu, ix, rows, lengths, order):
    """extract_sequences of ALL ids against the reads, and a locator over ALL positions against the sorted suffixes of the reads."""
    offsets, text = ix.extract_sequences()
    want = np.zeros(lengths.size + 1, dtype=np.uint64)
    want[1:] = np.cumsum(lengths.astype(np.uint64))
    assert np.array_equal(offsets, want) and np.array_equal(text, np.concatenate([rows[j, : int(lengths[j])] for j in range(lengths.size)]))
    loc = ix.locator()
    try:
        ids, offs = locate_raw(gpu, loc, np.arange(ix.bases))
        assert np.array_equal(ids, order[0]) and np.array_equal(offs, order[1])
    finally:
        loc.free()


def check_merge_form(gpu, oracle, case, form, algo, consumers=True):
    """One form of the merge of one pair under one dispatch of the search, against the oracle's merge (= the BWT of the concatenated text,
    PairCase checks that).  A slice or piece that holds one record and no position (n_out = 65 536, 131 072) is correct behaviour: the
    assembled result is what is compared."""
    gpu.tune("search_algo", algo)
    try:
        if form == "staged":
            ra = case.searched(gpu)
            M = gpu.interleave(case.A, case.B, ra)
            assert (M.sequences, M.bases) == (case.m.sequences, case.n)
            check_index(M, case.sym, np.random.default_rng(3), nq=64)
            check_every_position(M, case.sym)
            M.encode()
            case.check_index(M)
            if consumers:
                check_find_edges(M, case.m, case.sym)
                if case.n <= 65537:
                    check_sequences_and_locations(gpu, M, case.rows, case.lengths, case.order())
            M.free(); ra.free()
        elif form == "merge":
            M = gpu.merge(case.A, case.B)
            case.check_index(M)
            check_every_position(M, case.sym)
            M.free()
        elif form == "host":
            r = gpu.merge_host(inp(case.a), inp(case.b), samples=2)
            try:
                m = case.m
                assert (r.out.sequences, r.out.bases, r.out.nbytes, r.out.blocks) == (m.sequences, m.bases, m.nbytes, m.blocks)
                assert np.array_equal(r.C, m.C)
                case.check_laid_out(r.data, *r.expanded_samples())
            finally:
                r.free()
        elif form == "sliced":
            ra = case.searched(gpu)
            try:
                for parts in (2, 3):
                    case.check_laid_out(*sliced_result(gpu, case.A, case.B, ra, parts))
            finally:
                ra.free()
        elif form == "streamed":
            for slice_records in (512, 1024):
                check_streamed(gpu, inp(case.a), inp(case.b), case.m, slice_records)
        else:
            assert form == "parts"
            for parts in (2, 4):
                data, be, cum, _, _ = merge_parts(gpu, case.a, case.b, parts, 2)
                case.check_laid_out(data, be, cum)
    finally:
        gpu.tune("search_algo", 0)


def check_input_consumers(gpu, case):
    """find, sequences and locate on the UPLOADED inputs of a pair whose own size is on a boundary (a or b alone of 65 536 positions)."""
    for ix, f, (rows, lengths) in ((case.A, case.a, case.reads_a), (case.B, case.b, case.reads_b)):
        if f.bases == 65536:
            check_find_edges(ix, f, f.symbols)
            check_sequences_and_locations(gpu, ix, rows, lengths, suffix_order(rows, lengths))


# ------------------------------------------------------------------------------------------------------------------------------------
# Every single-index builder at every small size

@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("kind,n", bi.SMALL_STREAMS)
def test_small_builders(gpu, oracle, kind, n, builder):
    check_small_builder(gpu, oracle, kind, n, builder)


@pytest.mark.parametrize("chunk", [2 * GROUP_BYTES, 16 * GROUP_BYTES])
@pytest.mark.parametrize("n", [3968, 7936, 65536])
def test_streamed_upload_when_the_stream_ends_with_the_chunk(gpu, oracle, n, chunk):
    """The alternating streams of one and two groups (and 65 536 bytes) in chunks of two and sixteen groups: the last chunk is full to the
    byte (7936 in chunks of two groups) or the stream ends inside the first one."""
    sym = bi.alternating(n)
    f = oracle.FMI.from_symbols(sym)
    ix, _ = built(gpu, f, sym, "upload_streamed", chunk)
    try:
        assert np.array_equal(ix.C, f.C)
        check_every_position(ix, sym)
        ix.encode()
        check_native(ix, f)
    finally:
        ix.free()


# ------------------------------------------------------------------------------------------------------------------------------------
# The super-sized streams

_super = {}


def super_case(oracle, n):
    """(symbols, the oracle's FMI) of one super-sized stream; one at a time (read only)."""
    if n not in _super:
        _super.clear()
        sym = bi.super_stream(n)
        _super[n] = (sym, oracle.FMI.from_symbols(sym))
    return _super[n]


def edge_probes(n):
    """n - 129 .. n, and 129 positions on both sides of every multiple of 2^25 up to n."""
    around = [np.arange(k - 129, k + 130, dtype=np.int64) for k in range(bi.SUPER, n + 1, bi.SUPER)]
    return np.concatenate([np.arange(n - 129, n + 1, dtype=np.int64)] + around)


@pytest.mark.parametrize("builder", SUPER_BUILDERS)
@pytest.mark.parametrize("n", bi.SUPER_SIZES)
def test_super_sized_builders(gpu, oracle, n, builder):
    sym, f = super_case(oracle, n)
    ix, borrowed = built(gpu, f, sym, builder, 5 * GROUP_BYTES)
    try:
        assert (ix.bases, ix.sequences) == (n, f.sequences) and np.array_equal(ix.C, f.C)
        check_index_by_probes(ix, f, sym, np.random.default_rng(n % 1000), extra=edge_probes(n))
        check_find_edges(ix, f, sym)
        if builder == "upload":
            check_native(ix, f)
        ix.drop_native()
        ix.encode()
        check_native(ix, f)
    finally:
        ix.free()
        del borrowed
        gpu.trim()


# ------------------------------------------------------------------------------------------------------------------------------------
# Every form of the merge at every exact n_out

@pytest.fixture(scope="module")
def pair(request, gpu, oracle):
    case = PairCase(gpu, oracle, request.param)
    yield case
    case.free()
    gpu.trim()


@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pair", list(bi.READ_PAIRS), indirect=True)
def test_merge_forms_at_exact_n_out(gpu, oracle, pair, form, algo):
    check_merge_form(gpu, oracle, pair, form, algo, consumers=(algo == 2))


@pytest.mark.parametrize("pair", ["a_65536", "b_65536"], indirect=True)
def test_consumers_on_an_input_that_ends_on_a_segment(gpu, pair):
    check_input_consumers(gpu, pair)


# ------------------------------------------------------------------------------------------------------------------------------------
# The 2^25 chain

class Chain:
    def __init__(self, gpu, oracle):
        a, b = bi.chain_base(oracle)
        A, B = gpu.Index.upload(*inp(a)), gpu.Index.upload(*inp(b))
        self.BASE = gpu.merge(A, B)                                      # stays on the device for the three tails
        A.free(); B.free()
        self.base, _ = oracle.merge(a, b, threads=2)
        assert self.BASE.bases == self.base.bases == bi.CHAIN_BASE and np.array_equal(self.BASE.data(), self.base.data)
        self.tails = {}

    def tail(self, gpu, oracle, name):
        """-> (rows, lengths, the tail's FMI, the oracle's merge, its symbols), computed once per tail."""
        if name not in self.tails:
            rows, lengths = bi.chain_tail(oracle, name)
            t = oracle.FMI.from_text(bi.text_of(rows, lengths))
            m, _ = oracle.merge(self.base.clone(), t.clone(), threads=2)
            assert m.bases == bi.CHAIN_BASE + int(name)
            self.tails[name] = (rows, lengths, t, m, m.symbols)
        return self.tails[name]


@pytest.fixture(scope="module")
def chain(gpu, oracle):
    c = Chain(gpu, oracle)
    yield c
    c.BASE.free()
    gpu.trim()


@pytest.mark.parametrize("name", list(bi.CHAIN_TAILS))
def test_chain_to_the_super_block(gpu, oracle, chain, name):
    """bwtm_merge (non-consuming) of a tail of 511, 512, 513 positions into the base kept on the device: 2^25 - 1, 2^25, 2^25 + 1."""
    rows, lengths, t, m, sym = chain.tail(gpu, oracle, name)
    n = m.bases
    T = gpu.Index.upload(*inp(t))
    M = gpu.merge(chain.BASE, T)
    try:
        assert (M.sequences, M.bases, M.nbytes, M.blocks) == (m.sequences, n, m.nbytes, m.blocks) and np.array_equal(M.C, m.C)
        assert np.array_equal(M.data(), m.data)
        be, cum = M.samples()
        assert np.array_equal(be, m.samples[0]) and np.array_equal(cum, m.samples[1])
        check_index_by_probes(M, m, sym, np.random.default_rng(int(name)), extra=edge_probes(n))
        check_find_edges(M, m, sym)
        # 2000 sequences: the tail's (the last ones of the merge, against the reads themselves) and random ones of the base (LF walks of the oracle)
        rng = np.random.default_rng(5)
        first_tail = m.sequences - lengths.size
        ids = np.concatenate([rng.integers(0, m.sequences, 2000 - lengths.size - 1), [0], np.arange(first_tail, m.sequences)]).astype(np.uint64)
        offsets, text = M.extract_sequences(ids=ids)
        for k, j in enumerate(ids):
            got = text[int(offsets[k]): int(offsets[k + 1])]
            assert np.array_equal(got, bi.sequence_by_walk(m, int(j))), j
            if j >= first_tail:
                assert np.array_equal(got, rows[int(j) - first_tail, : int(lengths[int(j) - first_tail])]), j
        # 2000 positions: the last one, those around 2^25, the endmarker suffixes of the last sequences, random ones
        around = np.arange(bi.SUPER - 3, bi.SUPER + 4)
        around = around[around < n]
        pos = np.concatenate([rng.integers(0, n, 2000 - around.size - 4), around, [n - 1, 0, m.sequences - 1, m.sequences]]).astype(np.uint64)
        loc = M.locator()
        try:
            got_ids, got_offs = locate_raw(gpu, loc, pos)
        finally:
            loc.free()
        Cm = m.C
        for k, p in enumerate(pos):
            assert (int(got_ids[k]), int(got_offs[k])) == bi.locate_by_walk(m, int(p), Cm), p
    finally:
        M.free(); T.free()
        gpu.trim()


@pytest.mark.parametrize("form", ["sliced", "streamed"])
def test_chain_at_the_super_block_cut_every_512_records(gpu, oracle, chain, form):
    """n_out = 2^25 exactly, one slice per segment: 262 145 records, the last slice holds the one empty record and lies behind the last
    super boundary."""
    rows, lengths, t, m, sym = chain.tail(gpu, oracle, "512")
    assert m.bases == bi.SUPER
    if form == "streamed":
        check_streamed(gpu, inp(chain.base), inp(t), m, 512)
        return
    T = gpu.Index.upload(*inp(t))
    nrecs = gpu.merged_records(chain.BASE, T)
    assert nrecs == (bi.SUPER >> 7) + 1 and gpu.slice_bounds(nrecs, 513, 512) == (512 * 512, nrecs)
    ra = gpu.RankArray(chain.BASE, T)
    ra.search(chain.BASE, T, 0, t.sequences - 1)
    ra.finalize()
    try:
        data, be, cum, blocks = sliced_result(gpu, chain.BASE, T, ra, 513)
        assert np.array_equal(data, m.data) and blocks == m.blocks
        assert np.array_equal(be, m.samples[0]) and np.array_equal(cum, m.samples[1][:, :-1])
    finally:
        ra.free(); T.free()
        gpu.trim()


# ------------------------------------------------------------------------------------------------------------------------------------
# Ingest

@pytest.mark.parametrize("name", list(bi.INGEST_SHAPES))
def test_ingest_totals_on_tile_and_grid_edges(gpu, oracle, name):
    """One leaf; leaves of 128 reads (x 32 suffixes: a leaf ends exactly on a tile of 4096), of 64 reads (x 64 suffixes: the same for the
    reads of 63 bases) and of 100 reads (no leaf ends on a tile)."""
    rows, lengths, total = bi.ingest_shape(oracle, name)
    for leaf in (0, 128, 64, 100):
        check_ingest(gpu, oracle, rows, lengths, leaf_reads=leaf)
    check_ingest(gpu, oracle, rows, lengths, leaf_reads=128, batches=2, device=True)


# ------------------------------------------------------------------------------------------------------------------------------------
# The two argument checks: refused calls only (without the checks these calls read outside device buffers)

@pytest.fixture(scope="module")
def small_index(gpu, oracle):
    sym = bi.alternating(129)
    f = oracle.FMI.from_symbols(sym)
    ix = gpu.Index.upload(*inp(f))
    yield ix, sym
    ix.free()


@pytest.mark.parametrize("offsets,k", [([0, 5, 3, 8], 1), ([0, 12, 8], 1), ([9, 4, 9], 0), ([0, 2, 4, 1 << 63, 6], 3)])
def test_find_batch_refuses_offsets_that_decrease(gpu, small_index, offsets, k):
    """bwtm_find_batch through the raw prototype: an end before its begin, a middle entry beyond the last one (the device text holds
    offsets[count] bytes).  BWTM_EINVAL names the pattern, and nothing is written."""
    ix, _ = small_index
    capi = gpu.capi
    text = np.full(16, 1, dtype=np.uint8)
    off = np.array(offsets, dtype=np.uint64)
    count = off.size - 1
    sp = np.full(count, FILL, dtype=np.uint64); ep = np.full(count, FILL, dtype=np.uint64)
    rc = capi.lib().bwtm_find_batch(ix.h, text.ctypes.data_as(capi.p_u8), off.ctypes.data_as(capi.p_u64), count, sp.ctypes.data_as(capi.p_u64), ep.ctypes.data_as(capi.p_u64))
    assert rc == 1                                                         # BWTM_EINVAL
    assert capi.lib().bwtm_last_error().decode() == "bwtm_find_batch: offsets must not decrease (pattern %d)" % k
    assert np.all(sp == FILL) and np.all(ep == FILL)
    good = ix.find([np.array([1], dtype=np.uint8), np.zeros(0, dtype=np.uint8)])     # and the index still answers
    assert (int(good[0][1]), int(good[1][1])) == (0, 128)


def test_extract_refuses_a_range_whose_end_wraps(gpu, small_index):
    """bwtm_extract through the raw prototype: first + count wraps (2^64 - 1 and 2), first = n with one position; first = n with none is
    accepted and writes nothing."""
    ix, sym = small_index
    capi = gpu.capi
    n = sym.size
    out = np.full(64, 0xEE, dtype=np.uint8)
    for first, count in (((1 << 64) - 1, 2), (n, 1), (n + 1, 0), ((1 << 64) - 2, 3), (1, (1 << 64) - 1), (n - 1, 2)):
        rc = capi.lib().bwtm_extract(ix.h, first, count, out.ctypes.data_as(capi.p_u8))
        assert rc == 1, (first, count)                                     # BWTM_EINVAL
        assert capi.lib().bwtm_last_error().decode() == "bwtm_extract: range past the end"
        assert np.all(out == 0xEE)
    assert capi.lib().bwtm_extract(ix.h, n, 0, out.ctypes.data_as(capi.p_u8)) == 0 and np.all(out == 0xEE)
    assert capi.lib().bwtm_extract(ix.h, n - 1, 1, out.ctypes.data_as(capi.p_u8)) == 0 and out[0] == sym[n - 1] and np.all(out[1:] == 0xEE)
