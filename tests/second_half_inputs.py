"""Pairs of collections whose merge holds long runs made of pieces of BOTH inputs, shared by tests/test_second_half_inputs_host.py (the
pairs reach what they are for: conditions on the oracle's results alone) and tests/test_gpu_second_half_forms.py (every form of the merge's
second half -- one shot, sliced, ranged finalize, streamed, partitioned records -- on the same pairs).  Not a test module.  Texts are the
oracle's: symbols 1..5, each sequence followed by a 0 ("$"); everything is built from oracle.generate_reads, oracle.FMI.from_text,
oracle.FMI.from_runs and seeded numpy generators, so the pairs are deterministic.

What properties() measures on each pair (on the CPU, with the oracle alone; tests/test_second_half_inputs_host.py keeps floors below these):

genome60          3600 + 2700 reads of 100 bases of ONE genome of 6000 bases (both sets pass genome_seed: with the genome drawn from the
                  set's own seed the two sets are reads of different genomes, 1034 two-source runs >= 42 and no cut inside one).
                  636 300 positions, 39 767 runs, longest 445; 5548 two-source runs >= 42 (the encoder's two-byte forms); all 9 cuts of
                  65 536 positions inside a two-source run; halo from b / a 4 / 5.
repeated_super    48 reads x 36 000 copies + 40 reads x 25 000 copies of 12 bases: 22 464 000 + 13 000 000 = 35 464 000 positions (more than
                  2^25), 1 728 000 + 1 000 000 sequences, 897 runs, longest 180 000; native stream 3588 bytes in 57 blocks, longest block
                  862 000 positions (compact width 4), shortest 36 000; 24 two-source runs >= 65 536; 99 of 541 cuts inside a two-source
                  run, 5 of them beyond 2^25; 13 head-less slices inside two-source runs; halo from b / a 200 / 341; chunks of 8192
                  positions all from a / all from b 2505 / 1348.
homopolymer       3000 reads of symbol 3 of 0 .. 150 bases + 2500 of 0 .. 200: 475 290 positions, 10 656 runs, longest 1943; 255 two-source
                  runs >= 42; 12 and 10 blocks of 256 frontier elements, one class, a frontier that shrinks with every step.
two_homopolymers  1500 reads of symbol 1 then 1500 of symbol 4 (0 .. 150) + 1200 of symbol 4 (0 .. 200) then 1300 of symbol 1 (0 .. 90):
                  412 901 positions, 10 584 runs, longest 1024; 395 two-source runs >= 42; two classes with empty ones between them.
tiny_into_runs    repeated_super's a + three reads of 5, 7 and 9 bases (24 positions, a single record): 22 464 024 positions, 508 runs,
                  longest 216 000, longest block 916 426; 2724 of 2743 chunks all from a, up to the last one; every halo from a.
runs_into_tiny    the same pair swapped: 504 runs, longest block 988 426; 2724 chunks all from b; every halo from b.
"""
import numpy as np

PAIRS = ["genome60", "repeated_super", "homopolymer", "two_homopolymers", "tiny_into_runs", "runs_into_tiny"]
SUPER_SIZED = ("repeated_super", "tiny_into_runs", "runs_into_tiny")       # more than 2^24 positions: no 6-row count table of them in a test
SEGMENT = 65536                                                           # positions of an encoder segment (512 records): where slices are cut
GENOME60_SEED = 30                                                        # both read sets of genome60 are reads of this one genome
CHUNK = 8192                                                              # positions of a bitvector chunk: what the interleave stages at a time


def repetitive_reads(seed, genome_len, nreads, readlen, genome_seed=None):
    """Text of `nreads` reads of `readlen` bases from random places of a random genome of `genome_len` bases.  Without `genome_seed` the
    genome is drawn from `seed` too, so two sets of different seeds are reads of two DIFFERENT genomes (what tests/test_gpu_parts.py
    merges); with it the genome has a generator of its own, and sets of different seeds are reads of one genome."""
    rng = np.random.default_rng(seed)
    genome = (rng if genome_seed is None else np.random.default_rng(genome_seed)).integers(1, 5, genome_len, dtype=np.uint8)
    starts = rng.integers(0, genome_len - readlen, nreads)
    out = np.zeros((nreads, readlen + 1), dtype=np.uint8)
    for k, s in enumerate(starts):
        out[k, :readlen] = genome[s: s + readlen]
    return out.reshape(-1)


def repeated_collection(oracle, seed, nreads, readlen, copies):
    """Oracle FMI of the collection (read 0 x copies, read 1 x copies, ...)."""
    small = oracle.FMI.from_text(oracle.generate_reads(seed, nreads, readlen))
    sym = small.symbols.astype(np.uint64)
    return oracle.FMI.from_runs(sym, np.full(sym.size, copies, dtype=np.uint64))


def homopolymer_text(symbols, lengths):
    """Text of the reads (symbols[k] x lengths[k]), each followed by its 0."""
    lengths = np.asarray(lengths, dtype=np.int64)
    sym = np.stack([np.asarray(symbols, dtype=np.uint8), np.zeros(lengths.size, dtype=np.uint8)], axis=1).reshape(-1)
    return np.repeat(sym, np.stack([lengths, np.ones_like(lengths)], axis=1).reshape(-1))


def tiny(oracle):
    """Three reads of 5, 7 and 9 bases: 24 positions, a single record."""
    return oracle.FMI.from_text(np.concatenate([oracle.generate_reads(503 + k, 1, n) for k, n in enumerate((5, 7, 9))]))


def pair(oracle, name):
    """-> (a, b): the oracle FMIs of the pair `name`."""
    if name == "genome60":
        ta = repetitive_reads(31, 6000, 3600, 100, genome_seed=GENOME60_SEED); tb = repetitive_reads(32, 6000, 2700, 100, genome_seed=GENOME60_SEED)
        return oracle.FMI.from_text(ta), oracle.FMI.from_text(tb)
    if name == "repeated_super":
        return repeated_collection(oracle, 501, 48, 12, 36000), repeated_collection(oracle, 502, 40, 12, 25000)
    if name == "homopolymer":
        rng = np.random.default_rng(3)
        la = rng.integers(0, 151, 3000); lb = rng.integers(0, 201, 2500)
        return oracle.FMI.from_text(homopolymer_text(np.full(3000, 3), la)), oracle.FMI.from_text(homopolymer_text(np.full(2500, 3), lb))
    if name == "two_homopolymers":
        rng = np.random.default_rng(4)
        ta = homopolymer_text(np.repeat([1, 4], 1500), np.concatenate([rng.integers(0, 151, 1500), rng.integers(0, 151, 1500)]))
        tb = homopolymer_text(np.repeat([4, 1], [1200, 1300]), np.concatenate([rng.integers(0, 201, 1200), rng.integers(0, 91, 1300)]))
        return oracle.FMI.from_text(ta), oracle.FMI.from_text(tb)
    if name == "tiny_into_runs":
        return repeated_collection(oracle, 501, 48, 12, 36000), tiny(oracle)
    if name == "runs_into_tiny":
        return tiny(oracle), repeated_collection(oracle, 501, 48, 12, 36000)
    raise ValueError(name)


def searched_and_merged(oracle, a, b):
    """-> (ranks, counts, m): the oracle's rank array of inserting b into a as maximal runs, and its merge (a and b stay valid)."""
    ranks, counts, _ = oracle.search(a, b, capacity=min(b.bases, 1 << 22) + 1, threads=2)
    m, _ = oracle.merge(a.clone(), b.clone(), threads=2)
    return ranks, counts, m


def run_starts(sym):
    """Start positions of the maximal runs of a symbol array."""
    return np.concatenate([[0], np.flatnonzero(sym[1:] != sym[:-1]) + 1]).astype(np.int64) if sym.size else np.zeros(0, dtype=np.int64)


def properties(oracle, a, b, searched=None):
    """What the merge of a and b offers the second half, from the oracle's results alone (no GPU).  A run of the merged BWT is two-source
    when it takes positions from a and from b; the cuts are the multiples of 65 536 positions (512 records) inside the output, where
    slices may end; a cut lies inside a run when the run holds the positions on both sides of it.  searched: searched_and_merged()'s
    result when the caller has it already."""
    ranks, counts, m = searched if searched is not None else searched_and_merged(oracle, a, b)
    n = a.bases + b.bases
    src = np.zeros(n, dtype=np.uint8)
    ra = oracle.ra_from_runs(ranks, counts)
    assert ra.size == b.bases
    src[(np.arange(b.bases, dtype=np.uint64) + ra).astype(np.int64)] = 1
    sym = m.symbols
    assert sym.size == n
    starts = run_starts(sym)
    lengths = np.diff(np.concatenate([starts, [n]]))
    from_b = np.add.reduceat(src, starts, dtype=np.int64) if n else np.zeros(0, dtype=np.int64)
    two = (from_b > 0) & (from_b < lengths)
    cuts = np.arange(SEGMENT, n, SEGMENT, dtype=np.int64)
    run_of_cut = np.searchsorted(starts, cuts, side="right") - 1
    inside = (starts[run_of_cut] < cuts) & two[run_of_cut]
    headless = inside[:-1] & inside[1:] & (run_of_cut[:-1] == run_of_cut[1:])
    per_chunk = np.add.reduceat(src, np.arange(0, n, CHUNK), dtype=np.int64)
    chunk_len = np.minimum(CHUNK, n - np.arange(0, n, CHUNK))
    be = m.samples[0].astype(np.int64)
    return {
        "positions": n,
        "runs": int(starts.size),
        "longest_run": int(lengths.max()),
        "cuts": int(cuts.size),
        "two_source_runs_ge_42": int(np.count_nonzero(two & (lengths >= 42))),
        "two_source_runs_ge_65536": int(np.count_nonzero(two & (lengths >= SEGMENT))),
        "cuts_inside_two_source_run": int(np.count_nonzero(inside)),
        "beyond_2_25": int(np.count_nonzero(inside & (cuts > (1 << 25)))),
        "headless_slices_in_two_source_runs": int(np.count_nonzero(headless)),
        "halo_from_b": int(np.count_nonzero(src[cuts - 1] == 1)),
        "halo_from_a": int(np.count_nonzero(src[cuts - 1] == 0)),
        "chunks_all_a": int(np.count_nonzero(per_chunk == 0)),
        "chunks_all_b": int(np.count_nonzero(per_chunk == chunk_len)),
        "longest_block": int(np.diff(np.concatenate([[-1], be])).max()),
        "native_bytes": int(m.nbytes),
        "blocks": int(m.blocks),
    }
