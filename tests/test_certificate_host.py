"""The inversion certificate (tests/bwt_certificate.py) shown sound on the host before any GPU test rests on it: it accepts the BWT of
every collection however the oracle or the tensor-op builder made it, and it rejects every mutant of the symbols or of the reads
that differs from the original -- a condition, not a rate.  Also a second anchor for the oracle itself beyond brute-force sizes: its
merge of two sets of 10^5-read scale passes the certificate, which knows nothing of a suffix sort."""
import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from bwt_certificate import certify, certify_native, invert

FAMILIES = ["uniform", "skewed", "homopolymer", "two_symbols", "duplicates"]
MUTANT_KINDS = ["adjacent_swap", "far_swap", "rotate_window", "replace_symbol", "moved_rank", "exchange_reads", "shortened_read"]
MUTANTS_PER_CASE = 10


def draw_reads(rng, family, nseq):
    """-> (reads [nseq, 300] zero padded, lengths): the kinds tests/test_gpu_random_collections.py draws (lengths 0 .. 300, symbols 1 .. 5
    with N), and `duplicates`: sequences drawn with repetition from a pool of four, so equal suffixes of every length meet."""
    lengths = rng.choice([0, 1, 2, 7, 63, 64, 65, 100, 150, 300], nseq, p=[.08, .07, .05, .1, .1, .1, .1, .2, .1, .1]).astype(np.int64)
    reads = np.zeros((nseq, 300), dtype=np.uint8)
    pool = [rng.integers(1, 6, int(rng.choice([0, 3, 64, 100]))) for _ in range(4)]
    for k in range(nseq):
        L = int(lengths[k])
        if family == "uniform":
            s = rng.integers(1, 6, L)
        elif family == "skewed":
            s = rng.choice([1, 2, 3, 4, 5], L, p=[.7, .1, .1, .05, .05])
        elif family == "homopolymer":
            s = np.full(L, int(rng.integers(1, 6)))
        elif family == "two_symbols":
            s = rng.choice([2, 5], L)
        else:
            s = pool[int(rng.integers(0, 4))]
            lengths[k] = s.size
        reads[k, :s.size] = s
    return reads, lengths


def text_of(reads, lengths):
    """The oracle's text: every sequence followed by a 0."""
    parts = []
    for k in range(reads.shape[0]):
        parts.append(reads[k, :int(lengths[k])]); parts.append(np.zeros(1, dtype=np.uint8))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def mutate_symbols(rng, kind, sym):
    out = sym.copy()
    n = sym.size
    if kind == "adjacent_swap":
        i = int(rng.integers(0, n - 1))
        out[i], out[i + 1] = sym[i + 1], sym[i]
    elif kind == "far_swap":
        i, j = (int(v) for v in rng.integers(0, n, 2))
        out[i], out[j] = sym[j], sym[i]
    elif kind == "rotate_window":
        w = int(rng.integers(2, min(n, 9) + 1))
        i = int(rng.integers(0, n - w + 1))
        out[i:i + w] = np.roll(sym[i:i + w], int(rng.integers(1, w)))
    elif kind == "replace_symbol":
        i = int(rng.integers(0, n))
        out[i] = (int(sym[i]) + int(rng.integers(1, 6))) % 6
    else:
        raise ValueError(kind)
    return out


@st.composite
def cases(draw):
    return draw(st.sampled_from(FAMILIES)), draw(st.integers(0, 40)), draw(st.integers(0, 2 ** 31)), draw(st.integers(0, 2 ** 31))


def test_certificate_accepts_every_bwt_and_rejects_every_effective_mutant(oracle):
    """Per collection: the BWT by suffix sort, by the oracle's merge of a split in two and of a chain of three, pass; then mutants of seven kinds.
    A mutant equal to the original (symbols and reads) is skipped; every other one must be rejected, and every kind must yield at least 100
    effective mutants over the run, so the test cannot pass by skipping."""
    effective = {k: 0 for k in MUTANT_KINDS}
    rejected = {k: 0 for k in MUTANT_KINDS}
    accepted = [0]

    @settings(max_examples=80, deadline=None, derandomize=True, database=None)
    @given(cases())
    def run(case):
        family, nseq, seed, mseed = case
        rng = np.random.default_rng(seed)
        reads, lengths = draw_reads(rng, family, nseq)
        text = text_of(reads, lengths)
        sym = oracle.FMI.from_text(text).symbols
        assert certify(sym, reads, lengths) is None
        assert certify(sym, reads) is None                                           # lengths from the zero padding
        got, got_len, visited = invert(sym, nseq)
        assert visited == sym.size and np.array_equal(got_len, lengths) and np.array_equal(got, reads[:, :got.shape[1]])
        # the oracle's merge of a split in two, and of three chained sets
        c1, c2 = sorted(int(v) for v in rng.integers(0, nseq + 1, 2))
        ends = np.concatenate([[0], np.cumsum(lengths + 1)]).astype(np.int64)
        piece = lambda lo, hi: oracle.FMI.from_text(text[ends[lo]:ends[hi]])
        a, b = piece(0, c2), piece(c2, nseq)
        ra = None
        if b.bases > 0:
            ranks, counts, _ = oracle.search(a, b, threads=1)
            ra = oracle.ra_from_runs(ranks, counts)
            sa, sb = a.symbols, b.symbols
            assert np.array_equal(oracle.interleave_symbols(sa, sb, ra), sym)
        two, _ = oracle.merge(a, b, threads=2)
        assert certify(two.symbols, reads, lengths) is None
        first, _ = oracle.merge(piece(0, c1), piece(c1, c2), threads=1)
        three, _ = oracle.merge(first, piece(c2, nseq), threads=2)
        assert certify(three.symbols, reads, lengths) is None
        accepted[0] += 1

        mrng = np.random.default_rng(mseed)
        for kind in MUTANT_KINDS:
            for _ in range(MUTANTS_PER_CASE):
                msym, mreads, mlen = sym, reads, lengths
                if kind in ("adjacent_swap", "far_swap", "rotate_window", "replace_symbol"):
                    if sym.size < 2:
                        continue
                    msym = mutate_symbols(mrng, kind, sym)
                elif kind == "moved_rank":                                           # one suffix of B one place off in the interleaving
                    if ra is None:
                        continue
                    j = int(mrng.integers(0, ra.size))
                    moved = ra.copy()
                    moved[j] = min(int(ra[j]) + 1, sa.size) if (mrng.random() < 0.5 or ra[j] == 0) else int(ra[j]) - 1
                    msym = oracle.interleave_symbols(sa, sb, moved)
                elif kind == "exchange_reads":                                       # two sequences exchanged in the reads, not in the BWT
                    if nseq < 2:
                        continue
                    i, j = (int(v) for v in mrng.choice(nseq, 2, replace=False))
                    mreads = reads.copy(); mlen = lengths.copy()
                    mreads[[i, j]] = reads[[j, i]]; mlen[[i, j]] = lengths[[j, i]]
                else:                                                                # a read shortened by one
                    longer = np.flatnonzero(lengths > 0)
                    if longer.size == 0:
                        continue
                    i = int(mrng.choice(longer))
                    mreads = reads.copy(); mlen = lengths.copy()
                    mlen[i] -= 1
                    if mrng.random() < 0.5:
                        mreads[i, mlen[i]] = 0                                       # ... at its end
                    else:
                        mreads[i, :-1] = reads[i, 1:]; mreads[i, -1] = 0             # ... at its start
                if np.array_equal(msym, sym) and np.array_equal(mreads, reads):
                    continue
                effective[kind] += 1
                verdict = certify(msym, mreads, mlen)
                assert verdict is not None, (kind, case)
                assert isinstance(verdict, str) and len(verdict) < 2000
                rejected[kind] += 1

    run()
    print("certificate: %d collections accepted; mutants effective / rejected: %s"
          % (accepted[0], ", ".join("%s %d / %d" % (k, effective[k], rejected[k]) for k in MUTANT_KINDS)))
    for kind in MUTANT_KINDS:
        assert rejected[kind] == effective[kind], kind
        assert effective[kind] >= 100, (kind, effective[kind])


@pytest.mark.parametrize("workload,args", [("iid", {}), ("mixed", {}), ("genome", {"coverage": 30}), ("genome", {"coverage": 300})])
def test_certificate_accepts_the_tensor_op_leaf_builder(bwtm, workload, args):
    """synth.leaf_bwt (LSD radix sort of the suffixes, pinned to the oracle by tests/test_synth_tooling.py) of the three bench workloads."""
    from bwt_merge_amd import synth
    n = 3000
    reads = synth.make_reads(workload, 4242, 17, n, 100, n, **args)
    lengths = synth.read_lengths(workload, 17, n, 100)
    sym = synth.leaf_bwt(reads, lengths).numpy()
    assert certify(sym, reads.numpy(), None if lengths is None else lengths.numpy()) is None
    if args.get("coverage") == 300:
        assert np.unique(reads.numpy(), axis=0).shape[0] < n                        # equal reads: ties go by sequence index
    bad = sym.copy()
    edges = np.flatnonzero(sym[:-1] != sym[1:])
    i = int(edges[edges.size // 4])
    bad[i], bad[i + 1] = sym[i + 1], sym[i]
    assert "sequence" in certify(bad, reads.numpy())


ANCHOR_READS = 30_000


@pytest.mark.parametrize("workload,args", [("iid", {}), ("genome", {"coverage": 300})])
def test_oracle_merge_passes_the_certificate_beyond_brute_force(bwtm, oracle, workload, args):
    """The oracle's merge (its restated search + interleave) of two sets of 10^5 reads x 100: the merged native stream, its samples and C are
    the BWT of the 2 x 10^5 generated reads in order -- by inversion, which shares nothing with the oracle but its byte codec."""
    from bwt_merge_amd import synth
    n = ANCHOR_READS
    sets = [synth.make_reads(workload, seed, 0, n, 100, n, **args).numpy() for seed in (3001, 3002)]
    fm = []
    for reads in sets:
        text = np.zeros((n, 101), dtype=np.uint8)
        text[:, :100] = reads
        fm.append(oracle.FMI.from_text(text.reshape(-1)))
        del text
    m, _ = oracle.merge(fm[0], fm[1], threads=8)
    be, cum = m.samples
    assert (m.sequences, m.bases) == (2 * n, 2 * n * 101)
    assert certify_native(oracle, m.data, m.sequences, m.bases, be, cum, m.C, np.concatenate(sets)) is None


def test_certificate_on_empty_collections():
    none = np.zeros((0, 100), dtype=np.uint8)
    assert certify(np.zeros(0, dtype=np.uint8), none) is None
    assert "wrong size" in certify(np.zeros(1, dtype=np.uint8), none)
    assert invert(np.zeros(0, dtype=np.uint8), 0)[2] == 0
    empties = np.zeros((7, 3), dtype=np.uint8)
    assert certify(np.zeros(7, dtype=np.uint8), empties) is None
    assert certify(np.zeros(7, dtype=np.uint8), np.zeros((7, 0), dtype=np.uint8)) is None
    assert certify(np.zeros(7, dtype=np.uint8), empties, np.zeros(7, dtype=np.int64)) is None
    assert "wrong size" in certify(np.zeros(6, dtype=np.uint8), empties)
    assert "zeros" in certify(np.array([0, 0, 0, 0, 0, 0, 1], dtype=np.uint8), empties)


def test_certificate_diagnosis_names_what_is_wrong(oracle):
    """The three findings a failing assert prints: the size, the rows no walk reaches, the first sequence that differs."""
    reads = np.array([[1, 2, 3, 0], [1, 2, 0, 0], [4, 4, 4, 4]], dtype=np.uint8)
    sym = oracle.FMI.from_text(text_of(reads, np.array([3, 2, 4]))).symbols
    assert certify(sym, reads) is None
    assert "wrong size" in certify(sym[:-1], reads)
    assert "outside the alphabet" in certify(np.where(sym == 4, 6, sym).astype(np.uint8), reads)
    other = reads.copy(); other[1, 1] = 3
    verdict = certify(sym, other)
    assert "first: sequence 1 (walk from row 1)" in verdict and "expected AG (2), found AC (2)" in verdict
    # a cycle that no endmarker row reaches: "4 4 4 4 $" rotated so that its walk ends early leaves rows unvisited
    cyc = np.array([4, 0, 4], dtype=np.uint8)                       # one sequence; row 0 reads T, goes to row 1 and stops: row 2 is its own cycle
    verdict = certify(cyc, np.array([[4, 4]], dtype=np.uint8))
    assert "rows not all visited: 1 of 3" in verdict and "sequence 0" in verdict
    with pytest.raises(ValueError):
        certify(sym, np.array([[1, 0, 2, 0]], dtype=np.uint8))     # a symbol behind the end of a row
