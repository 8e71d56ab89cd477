"""The two forms in which k_frontier_step stores the next frontier (bwtm_tune frontier_stage_out: 1 = in slot order through LDS, whole
lines per wave; 0 = every lane its own element) put the same values at the same addresses.  The frontier search runs with the knob at
0 and at 1 on the same inputs; the rank array's bits and its run download are compared with the CPU oracle and with each other, bit
for bit."""
import numpy as np
import pytest

from parts_inputs import check_against_oracle, wide_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    yield bwtm
    for k, v in (("frontier_stage_out", 1), ("search_algo", 0), ("range_ratio", -1), ("frontier_epoch", 0)):
        bwtm.tune(k, v)
    bwtm.make_default_current()
    bwtm.trim()


def expected_bits(oracle, ranks, counts, n_out):
    """The rank array as the bitvector the search builds: bit j + rank[j] is set for the j-th smallest rank (64-bit words)."""
    ora = oracle.ra_from_runs(ranks, counts).astype(np.uint64)
    p = ora + np.arange(ora.size, dtype=np.uint64)                        # strictly increasing
    words = np.zeros((n_out + 63) // 64, dtype=np.uint64)
    if p.size:
        idx, start = np.unique(p >> np.uint64(6), return_index=True)
        words[idx.astype(np.int64)] = np.add.reduceat(np.uint64(1) << (p & np.uint64(63)), start)      # distinct bits of a word: the sum is the OR
    return words


def search_both_forms(gpu, oracle, a, b, algo, range_ratio, oracle_kw):
    """Searches all of b's sequences in a with the knob at 0 and at 1 -> the profiles of the two runs."""
    oranks, ocounts, _ = oracle.search(a, b, **oracle_kw)
    obits = expected_bits(oracle, oranks, ocounts, a.bases + b.bases)
    A = gpu.Index.upload(a.data, a.sequences, a.bases); B = gpu.Index.upload(b.data, b.sequences, b.bases)
    bits, profs = {}, {}
    try:
        for stage in (0, 1):
            gpu.tune("frontier_stage_out", stage); gpu.tune("search_algo", algo); gpu.tune("range_ratio", range_ratio)
            gpu.profile_enable(True); gpu.profile_reset()
            ra = gpu.RankArray(A, B)
            ra.search(A, B, 0, b.sequences - 1)
            ra.finalize()
            profs[stage] = gpu.profile_read()
            gpu.profile_enable(False)
            assert ra.values == b.bases, stage
            ranks, counts = ra.runs()
            bits[stage] = ra.bits()
            ra.free()
            assert np.array_equal(ranks, oranks) and np.array_equal(counts, ocounts), stage
            assert np.array_equal(bits[stage], obits), stage
        assert np.array_equal(bits[0], bits[1])
    finally:
        gpu.tune("frontier_stage_out", 1); gpu.tune("search_algo", 0); gpu.tune("range_ratio", -1)
        A.free(); B.free()
        gpu.trim()
    return profs


def test_expected_bits_helper(oracle):
    ranks = np.array([0, 2, 2, 2, 70], dtype=np.uint64); counts = np.array([1, 1, 1, 1, 2], dtype=np.uint64)       # positions 0, 3, 4, 5, 74, 75
    w = expected_bits(oracle, ranks, counts, 200)
    assert w.size == 4 and int(w[0]) == 0b111001 and int(w[1]) == (1 << 10) | (1 << 11) and int(w[2]) == 0 and int(w[3]) == 0


def test_iid_reads_above_the_frontier_threshold(gpu, oracle):
    """More than 2^21 iid reads: the dispatch itself picks the frontier search; every block of the early steps is full and holds
    all four classes (range_ratio = 0: elements from the roots on, no node levels)."""
    b = oracle.FMI.from_text(oracle.generate_reads(7702, (1 << 21) + 70000, 16))
    a = oracle.FMI.from_text(oracle.generate_reads(7701, 120000, 100))
    assert b.sequences > (1 << 21)
    profs = search_both_forms(gpu, oracle, a, b, 0, 0, dict(threads=8))
    for prof in profs.values():
        assert prof["frontier_step"][1] >= 16 and "lf_walk" not in prof and "range_step" not in prof, sorted(prof)


@pytest.mark.parametrize("range_ratio", [0, 8])
def test_reads_of_mixed_lengths(gpu, oracle, range_ratio):
    """Chains end at different steps: blocks whose survivors do not fill their slot, classes that run empty, and blocks past the
    shrunken frontier (which only publish empty segments)."""
    ta = oracle.generate_reads(9400, 2500, 90)
    tb = np.concatenate([oracle.generate_reads(9500 + j, 700, int(n)) for j, n in enumerate([1, 17, 60, 100, 139, 33, 2, 250])])
    a, b = oracle.FMI.from_text(ta), oracle.FMI.from_text(tb)
    profs = search_both_forms(gpu, oracle, a, b, 2, range_ratio, dict(threads=2))
    for prof in profs.values():
        assert prof["frontier_step"][1] + prof.get("range_step", (0, 0))[1] >= 250 and prof["frontier_step"][1] > 0, sorted(prof)


def test_coordinates_beyond_32_bits(gpu, oracle):
    """An index of more than 2^32 positions: the high bytes of the coordinates take the same way through LDS (the HI instantiation)."""
    a, b = wide_inputs(oracle)
    gpu.tune("frontier_epoch", 5)
    try:
        profs = search_both_forms(gpu, oracle, a, b, 2, 0, dict(capacity=1 << 21, threads=8))
    finally:
        gpu.tune("frontier_epoch", 0)
    for prof in profs.values():
        assert prof["frontier_step"][1] >= 70, sorted(prof)


def test_partitioned_merge_of_three_parts(gpu, oracle):
    """The PULL instantiation: three parts (contexts of this GPU) whose step kernels read each other's output buffers; reads of mixed
    lengths, elements from the roots on."""
    from bwt_merge_amd import partitioned
    ta = oracle.generate_reads(9400, 2500, 90)
    tb = np.concatenate([oracle.generate_reads(9500 + j, 400, int(n)) for j, n in enumerate([1, 17, 60, 100, 139, 33])])
    a, b = oracle.FMI.from_text(ta), oracle.FMI.from_text(tb)
    merged = {}
    try:
        for stage in (0, 1):
            gpu.tune("frontier_stage_out", stage); gpu.tune("range_ratio", 0)
            ha = gpu.host_index(a.data, a.samples[1], a.sequences, a.bases); hb = gpu.host_index(b.data, b.samples[1], b.sequences, b.bases)
            out = partitioned.merge_parts(gpu, ha, hb, 3, kmer=3, collect=lambda g, s: partitioned.slice_arrays(s))
            try:
                got = out["collected"]
                data = np.concatenate([g[0] for g in got]); be = np.concatenate([g[1] for g in got]); cum = np.concatenate([g[2] for g in got], axis=1)
                assert all(s["steps"] + s["node_levels"] == 140 and s["node_levels"] == 0 for s in out["stats"]), out["stats"]
            finally:
                out["release"]()
            check_against_oracle(oracle, a, b, data, be, cum)
            merged[stage] = (data, be, cum)
        assert all(np.array_equal(x, y) for x, y in zip(merged[0], merged[1]))
    finally:
        gpu.tune("frontier_stage_out", 1); gpu.tune("range_ratio", 8)
