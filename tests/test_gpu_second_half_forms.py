"""Every form of the merge's second half (interleave, encode, samples) on the SAME pairs of collections, whose merged BWT holds long runs
made of pieces of both inputs (tests/second_half_inputs.py; tests/test_second_half_inputs_host.py proves that they do): one shot, staged
and through bwtm_merge / bwtm_merge_host; sliced by output range; the ranged finalize behind a reduce-scatter; streamed; partitioned
records.  A two-source run is open at slice cuts, fills whole slices and sits behind 2^25 positions, which is where the sliced forms carry
state across cuts (the halo symbol and record, the last head, the size table as a function of the byte offset, the carried open block and
the re-guessed sample width of the streamed form, the halo words of the ranged finalize).  Every bitvector is the library's own search and
equals the oracle's rank array; every result is compared bit for bit with the oracle's merge: data, C, block_end, cum."""
import numpy as np
import pytest

import second_half_inputs as shi
from parts_inputs import check_against_oracle, merge_parts
from streamed_child import COMPACT, check_streamed, collect
from test_gpu_parity import check_index
from test_gpu_slices import check_range_finalize, sliced_result

pytestmark = pytest.mark.gpu

every_pair = pytest.mark.parametrize("case", shi.PAIRS, indirect=True)
TINY = ("tiny_into_runs", "runs_into_tiny")


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    yield bwtm
    bwtm.tune("search_algo", 0); bwtm.tune("range_ratio", -1); bwtm.tune("stream_samples_query", 0)
    bwtm.trim()


class Case:
    """One pair: the oracle's FMIs, rank array runs and merge, and the uploaded inputs (read only)."""

    def __init__(self, gpu, oracle, name):
        self.name = name
        self.a, self.b = shi.pair(oracle, name)
        self.ranks, self.counts, self.m = shi.searched_and_merged(oracle, self.a, self.b)
        self.n = self.a.bases + self.b.bases
        self.data = self.m.data
        self.obe, self.ocum = self.m.samples
        self.longest_block = int(np.diff(np.concatenate([[-1], self.obe.astype(np.int64)])).max())
        self.inp_a = (self.a.data, self.a.sequences, self.a.bases); self.inp_b = (self.b.data, self.b.sequences, self.b.bases)
        self.A = gpu.Index.upload(*self.inp_a); self.B = gpu.Index.upload(*self.inp_b)
        self.segments = (gpu.merged_records(self.A, self.B) + 511) // 512

    def searched(self, gpu):
        """A finalized rank array of the library's own search, checked against the oracle's."""
        ra = gpu.RankArray(self.A, self.B)
        ra.search(self.A, self.B, 0, self.b.sequences - 1)
        ra.finalize()
        assert ra.values == self.b.bases
        ranks, counts = ra.runs()
        assert np.array_equal(ranks, self.ranks) and np.array_equal(counts, self.counts)
        return ra

    def check_samples(self, be, cum, blocks=None):
        """block_end and cum (with or without the column behind the last block) are the oracle's."""
        assert np.array_equal(be, self.obe)
        assert np.array_equal(cum, self.ocum if cum.shape[1] == self.ocum.shape[1] else self.ocum[:, :-1]) and cum.shape[1] >= self.m.blocks
        assert blocks is None or blocks == self.m.blocks


@pytest.fixture(scope="module")
def case(request, gpu, oracle):
    c = Case(gpu, oracle, request.param)
    yield c
    c.A.free(); c.B.free()
    gpu.trim()


def narrowest_width(longest_block):
    """The compact rule: the narrowest field that holds the longest block (streamed_child.narrowest states it per piece)."""
    return 1 if longest_block < 0xFF else 2 if longest_block < 0xFFFF else 4


def check_index_by_probes(ix, m, sym, rng, extra=(), nq=4000):
    """check_index for an index too large for a table of all counts: the symbols, then rank of every symbol, clamping and
    inverse_select at nq random positions, around every cut of 65 536 positions and around 2^25, and at the caller's `extra` positions
    (those outside 0 .. n are dropped), against the oracle's own rank."""
    n = sym.size
    assert ix.bases == n and np.array_equal(ix.extract(0, n), sym)
    cuts = np.arange(shi.SEGMENT, n, shi.SEGMENT, dtype=np.int64)
    pos = np.concatenate([rng.integers(0, n + 1, nq), cuts - 1, cuts, cuts + 1, [(1 << 25) - 1, 1 << 25, (1 << 25) + 1], [0, n, n - 1, 127, 128, 129],
                          np.asarray(extra, dtype=np.int64)])
    pos = np.unique(pos[(pos >= 0) & (pos <= n)]).astype(np.uint64)
    for c in range(6):
        got = ix.rank(pos, np.full(pos.size, c, dtype=np.uint8))
        assert np.array_equal(got, np.array([m.rank(int(p), c) for p in pos], dtype=np.uint64)), c
    assert int(ix.rank([n + 5], [2])[0]) == m.rank(n, 2) and int(ix.rank([3], [7])[0]) == 0
    ipos = pos[pos < n]
    r, c = ix.inverse_select(ipos)
    assert np.array_equal(c, sym[ipos.astype(np.int64)])
    assert np.array_equal(r, np.array([m.rank(int(p), int(s)) for p, s in zip(ipos, c)], dtype=np.uint64))


def check_subset_check(gpu, case, whole):
    """bwtm_ra_subset_check (k_bits_subset): the searches of the two halves of b lie inside the search of all of it and outside each
    other; one bit more, in a caller-owned copy, is one word outside; rank arrays of different shapes are refused."""
    import torch
    A, B, b = case.A, case.B, case.b
    half = b.sequences // 2
    parts = []
    for first, last in ((0, half - 1), (half, b.sequences - 1)):
        ra = gpu.RankArray(A, B)
        ra.search(A, B, first, last)
        parts.append(ra)
    wbits = whole.bits()
    pbits = [p.bits() for p in parts]
    ones = [int(np.unpackbits(x.view(np.uint8)).sum()) for x in pbits]
    assert sum(ones) == b.bases and ones[0] == half * (b.bases // b.sequences)        # reads of one length
    assert np.array_equal(pbits[0] | pbits[1], wbits) and not np.any(pbits[0] & pbits[1])
    for p, mine in zip(parts, ones):
        assert p.subset_check(whole) == (mine, 0)
    assert whole.subset_check(whole) == (b.bases, 0)
    assert parts[0].subset_check(parts[1]) == (ones[0], int(np.count_nonzero(pbits[0])))       # disjoint: every word with a bit is outside
    assert whole.subset_check(parts[1]) == (b.bases, int(np.count_nonzero(pbits[0])))
    # one bit the whole lacks -- in the first word, in the middle, in the last word of the output -- in a caller-owned copy of part 0
    nbytes = gpu.ra_buffer_bytes(A, B)
    lacking = ~wbits
    lacking[-1] &= np.uint64((1 << ((case.n - 1) % 64 + 1)) - 1)         # positions of the output only
    candidates = np.flatnonzero(lacking)
    for word in (candidates[0], candidates[candidates.size // 2], candidates[-1]):
        free = int(lacking[word])
        words = np.zeros(nbytes // 8, dtype=np.uint64)
        words[: pbits[0].size] = pbits[0]
        words[word] |= np.uint64(free & -free)
        t = torch.from_numpy(words.view(np.int64)).to("cuda:0")
        edited = gpu.RankArray(A, B, t.data_ptr(), nbytes)
        assert edited.subset_check(whole) == (ones[0] + 1, 1), word
        edited.free()
        del t
    other = gpu.RankArray(A, A)
    with pytest.raises(gpu.BwtmError, match="shapes"):
        parts[0].subset_check(other)
    with pytest.raises(gpu.BwtmError, match="shapes"):
        other.subset_check(whole)
    for x in parts + [other]:
        x.free()


@every_pair
def test_staged_one_shot(gpu, case):
    """bwtm_search under three dispatches (the frontier search with the node phase and without it, the per-chain walk) gives the
    oracle's runs; bwtm_interleave gives the merged symbols and their ranks; bwtm_index_encode the bytes and both forms of the samples."""
    A, B, m = case.A, case.B, case.m
    ras = []
    try:
        for algo, ratio in ((2, -1), (2, 0), (1, -1)):
            gpu.tune("search_algo", algo); gpu.tune("range_ratio", ratio)
            ras.append(case.searched(gpu))
    finally:
        gpu.tune("search_algo", 0); gpu.tune("range_ratio", -1)
    if case.name == "genome60":
        check_subset_check(gpu, case, ras[0])
    M = gpu.interleave(A, B, ras[0])
    assert (M.sequences, M.bases) == (m.sequences, m.bases)
    rng = np.random.default_rng(3)
    if case.name in shi.SUPER_SIZED:
        check_index_by_probes(M, m, m.symbols, rng)
    else:
        check_index(M, m.symbols, rng, nq=2000)
    M.encode()
    assert M.nbytes == m.nbytes and np.array_equal(M.data(), case.data) and np.array_equal(M.C, m.C)
    case.check_samples(*M.samples(), blocks=M.blocks)
    width, fields, anchors = M.samples_compact()
    assert width == narrowest_width(case.longest_block)
    case.check_samples(*gpu.capi.expand_samples(width, fields, anchors, m.blocks, m.bases))
    for x in ras + [M]:
        x.free()
    gpu.trim()


@every_pair
def test_merge_entry_points(gpu, case):
    """bwtm_merge on the device and bwtm_merge_host with the compact samples, at the narrowest width that holds the longest block."""
    m = case.m
    M = gpu.merge(case.A, case.B)
    assert (M.sequences, M.bases, M.nbytes, M.blocks) == (m.sequences, m.bases, m.nbytes, m.blocks)
    assert np.array_equal(M.data(), case.data) and np.array_equal(M.C, m.C)
    case.check_samples(*M.samples())
    M.free()
    r = gpu.merge_host(case.inp_a, case.inp_b, samples=2)
    try:
        assert (r.out.sequences, r.out.bases, r.out.nbytes, r.out.blocks) == (m.sequences, m.bases, m.nbytes, m.blocks)
        assert np.array_equal(r.data, case.data) and np.array_equal(r.C, m.C)
        assert r.out.sample_width == narrowest_width(case.longest_block)
        case.check_samples(*r.expanded_samples())
    finally:
        r.free()
    gpu.trim()


@every_pair
def test_sliced_by_output_range(gpu, case):
    """bwtm_interleave_range + bwtm_slice_*: two-source runs open at the cuts, down to one slice per segment (slices without a head)."""
    parts = [1, 2, 5, 16]
    if case.segments >= 16:
        parts.append(64 if case.name == "repeated_super" else case.segments)
    ra = case.searched(gpu)
    try:
        for p in parts:
            data, be, cum, blocks = sliced_result(gpu, case.A, case.B, ra, p)
            assert np.array_equal(data, case.data), p
            case.check_samples(be, cum, blocks)
        # a slice answers for its own positions: the first and the last ones of slices that begin inside a run
        sym = case.m.symbols
        nrecs = gpu.merged_records(case.A, case.B)
        for g in range(5):
            f, l = gpu.slice_bounds(nrecs, 5, g)
            s = gpu.Slice(case.A, case.B, ra, f, l)
            lo, hi = f * 128, min(l * 128, case.n)
            count = min(1000, hi - lo)
            assert np.array_equal(s.extract(lo, count), sym[lo: lo + count]) and np.array_equal(s.extract(hi - count, count), sym[hi - count: hi]), g
            s.free()
    finally:
        ra.free()
    gpu.trim()


@every_pair
def test_ranged_finalize_behind_a_reduce_scatter(gpu, oracle, case):
    """bwtm_ra_range_counts / bwtm_ra_finalize_range: halo chunks with set bits, ranges that begin inside a two-source run."""
    ra = case.searched(gpu)
    full_bits = ra.bits()
    ra.free()
    for parts in (3, 8):
        check_range_finalize(gpu, oracle, case.a, case.b, case.A, case.B, parts, m=case.m, full_bits=full_bits)
    gpu.trim()


@every_pair
@pytest.mark.parametrize("slice_records", [512, 2048, 0])
def test_streamed(gpu, case, slice_records):
    """bwtm_merge_host_streamed without samples, with the full and with the compact ones: the block a two-source run opened slices
    earlier, pieces of different widths."""
    check_streamed(gpu, case.inp_a, case.inp_b, case.m, slice_records)
    if case.name == "repeated_super" and slice_records == 512:
        pieces, out, stats = collect(gpu, case.inp_a, case.inp_b, slice_records, COMPACT)
        # every block of this stream holds 36 000 positions or more, all but one more than 65 535: the first guess of the width is wrong
        # and no piece with block starts is narrow (check_streamed's `narrowest`), while a piece of bytes alone states the narrowest width
        print("pieces (blocks, width, bytes):", [(p.sample_blocks, p.sample_width, p.nbytes) for p in pieces])
        assert 4 in {p.sample_width for p in pieces if p.sample_blocks > 0}
        assert 1 in {p.sample_width for p in pieces}
        assert len(pieces) < case.segments                               # the slices inside a run have no head and yield no piece
    gpu.trim()


@pytest.mark.parametrize("case", [name for name in shi.PAIRS if name not in TINY], indirect=True)      # test_parts_merge_of_odd_collections owns that shape
@pytest.mark.parametrize("parts,kmer", [(3, 2), (5, 3)])
def test_partitioned_records(gpu, oracle, case, parts, kmer):
    """bwtm_part_finish: every part interleaves and encodes its range from windows of the records; the homopolymer collections also
    without the node phase and with it (all live chains of a step in one class of the step kernel's 5-way split)."""
    for ratio in ((0, 8) if "homopolymer" in case.name else (-1,)):      # -1: the default
        gpu.tune("range_ratio", ratio)
        try:
            data, be, cum, _, _ = merge_parts(gpu, case.a, case.b, parts, kmer)
        finally:
            gpu.tune("range_ratio", -1)
        check_against_oracle(oracle, case.a, case.b, data, be, cum)
    gpu.trim()
