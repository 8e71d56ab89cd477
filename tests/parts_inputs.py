"""Inputs and helpers of the merge over partitioned records shared by tests/test_gpu_parts.py (parts as threads), tests/test_gpu_parts_processes.py
(parts as processes) and tests/test_gpu_second_half_forms.py.  Texts are the oracle's: symbols 1..5, each sequence followed by a 0 ("$")."""
import numpy as np

ODD_CASES = ["short", "one_base", "with_n", "tiny_b", "unequal", "empty_b"]


def odd_collection(case):
    """(text_a, text_b) of collections on which most parts end up with nothing: windows of a single record, coinciding cuts, empty output
    ranges.  'empty_b' holds one empty sequence (a single "$")."""
    rng = np.random.default_rng({"short": 1, "one_base": 2, "with_n": 3, "tiny_b": 4, "unequal": 5, "empty_b": 6}[case])

    def reads(n, lo, hi, alphabet):
        out = []
        for _ in range(n):
            out.append(rng.choice(alphabet, rng.integers(lo, hi + 1)).astype(np.uint8)); out.append(np.zeros(1, dtype=np.uint8))
        return np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)

    if case == "short":
        return reads(400, 0, 3, [1, 2, 3, 4]), reads(300, 0, 4, [1, 2, 3, 4])
    if case == "one_base":
        return reads(200, 5, 40, [3]), reads(150, 1, 60, [3])
    if case == "with_n":
        return reads(300, 20, 50, [1, 2, 3, 4, 5, 5]), reads(250, 10, 70, [1, 2, 3, 4, 5])
    if case == "tiny_b":
        return reads(500, 30, 60, [1, 2, 3, 4]), reads(3, 5, 9, [1, 2, 3, 4])
    if case == "unequal":
        return reads(40, 10, 20, [1, 2, 3, 4]), reads(900, 40, 80, [1, 2, 3, 4])
    if case == "empty_b":
        return reads(300, 20, 50, [1, 2, 3, 4]), reads(1, 0, 0, [1])
    raise ValueError(case)


def truly_empty(oracle, which):
    """(a, b) oracle FMIs where input `which` ("a" or "b") holds 0 sequences and 0 bases; the other is 3000 reads of 60 bases."""
    e = oracle.FMI.from_text(np.zeros(0, dtype=np.uint8))
    x = oracle.FMI.from_text(oracle.generate_reads(9601, 3000, 60))
    assert e.sequences == 0 and e.bases == 0 and e.data.size == 0
    return (e, x) if which == "a" else (x, e)


def wide_inputs(oracle):
    """(a, b) with a of more than 2^32 positions (runs of 120 000): coordinates whose high bytes matter."""
    small_a = oracle.FMI.from_text(oracle.generate_reads(9301, 600, 60)); small_b = oracle.FMI.from_text(oracle.generate_reads(9302, 500, 70))
    a = oracle.FMI.from_runs(small_a.symbols.astype(np.uint64), np.full(small_a.symbols.size, 120000, dtype=np.uint64))
    b = oracle.FMI.from_runs(small_b.symbols.astype(np.uint64), np.full(small_b.symbols.size, 2000, dtype=np.uint64))
    assert a.bases > (1 << 32)
    return a, b


def host(gpu, x):
    return gpu.host_index(x.data, x.samples[1], x.sequences, x.bases)


def merge_parts(gpu, a, b, parts, kmer=0):
    """-> (data, block_end, cum, stats, cuts): the parts' bytes and samples laid end to end."""
    from bwt_merge_amd import partitioned
    out = partitioned.merge_parts(gpu, host(gpu, a), host(gpu, b), parts, kmer=kmer, collect=lambda g, s: partitioned.slice_arrays(s))
    try:
        got = out["collected"]
        total = out["slices"][0].total_nbytes
        assert all(s.total_nbytes == total for s in out["slices"])
        offsets = [s.byte_offset for s in out["slices"]]
        assert offsets == sorted(offsets) and offsets[0] == 0
        data = np.concatenate([g[0] for g in got]); be = np.concatenate([g[1] for g in got]); cum = np.concatenate([g[2] for g in got], axis=1)
        assert data.size == total
        return data, be, cum, out["stats"], out["cuts"]
    finally:
        out["release"]()


def check_against_oracle(oracle, a, b, data, be, cum, threads=2):
    """The parts' bytes and samples laid end to end (cum without its last column) equal the oracle's merge, bit for bit."""
    m, _ = oracle.merge(a.clone(), b.clone(), threads=threads)
    assert data.dtype == m.data.dtype and np.array_equal(data, m.data)
    obe, ocum = m.samples
    assert np.array_equal(be, obe) and np.array_equal(cum, ocum[:, :-1])
    return m
