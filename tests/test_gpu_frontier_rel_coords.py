"""The two forms of the coordinates k_frontier_step keeps in the frontier buffers (bwtm_tune frontier_rel): absolute (i, r) with a 2-byte
array of high bytes when an index has 2^32 positions or more, or the offsets inside the element's symbol class, (i - C_B[c], r - C_A[c]) in 32
bits each and no high bytes, the class being the row of the segment table the element is read through.  The frontier search runs with the
knob at 0 and at the other value on the same uploads; ranks, counts and the rank array's bits are compared with the CPU oracle and with
each other, and bwtm_frontier_step_forms tells which form the launches took: the first step of a relative search reads the absolute
frontier (form 1), every later one is relative (form 2)."""
import numpy as np
import pytest

from parts_inputs import wide_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    yield bwtm
    for k, v in (("frontier_rel", 1), ("search_algo", 0), ("range_ratio", -1), ("frontier_epoch", 0)):
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


def search_forms(gpu, oracle, a, b, algo, range_ratio, oracle_kw, knobs=(0, 2)):
    """Searches all of b's sequences in a once per value of the knob, on the same uploads -> {knob: (profile, launches per form)}."""
    oranks, ocounts, _ = oracle.search(a, b, **oracle_kw)
    obits = expected_bits(oracle, oranks, ocounts, a.bases + b.bases)
    A = gpu.Index.upload(a.data, a.sequences, a.bases); B = gpu.Index.upload(b.data, b.sequences, b.bases)
    bits, out = {}, {}
    try:
        for knob in knobs:
            gpu.tune("frontier_rel", knob); gpu.tune("search_algo", algo); gpu.tune("range_ratio", range_ratio)
            gpu.profile_enable(True); gpu.profile_reset()
            ra = gpu.RankArray(A, B)
            ra.search(A, B, 0, b.sequences - 1)
            ra.finalize()
            out[knob] = (gpu.profile_read(), gpu.frontier_step_forms())
            gpu.profile_enable(False)
            assert ra.values == b.bases, knob
            ranks, counts = ra.runs()
            bits[knob] = ra.bits()
            ra.free()
            assert np.array_equal(ranks, oranks) and np.array_equal(counts, ocounts), knob
            assert np.array_equal(bits[knob], obits), knob
        for knob in knobs[1:]:
            assert np.array_equal(bits[knobs[0]], bits[knob]), knob
    finally:
        gpu.tune("frontier_rel", 1); gpu.tune("search_algo", 0); gpu.tune("range_ratio", -1)
        A.free(); B.free()
        gpu.trim()
    return out


def assert_forms(out, absolute, relative):
    """The knob values in `absolute` ran form 0 only; those in `relative` one launch of form 1 and form 2 for all others.  The launches
    counted are the ones the profile names frontier_step."""
    for knob in absolute:
        prof, forms = out[knob]
        assert forms[0] == prof["frontier_step"][1] > 0 and forms[1] == 0 and forms[2] == 0, (knob, forms)
    for knob in relative:
        prof, forms = out[knob]
        assert forms[0] == 0 and forms[1] == 1 and forms[2] == prof["frontier_step"][1] - 1 > 0, (knob, forms)


def class_counts(x):
    """Occurrences of the symbols 1 .. 5 (the classes of the frontier) from the index's C array."""
    C = [int(v) for v in x.C]
    return [C[c + 1] - C[c] for c in range(1, 6)]


def mixed_inputs(oracle):
    ta = oracle.generate_reads(9400, 2500, 90)
    tb = np.concatenate([oracle.generate_reads(9500 + j, 700, int(n)) for j, n in enumerate([1, 17, 60, 100, 139, 33, 2, 250])])
    return oracle.FMI.from_text(ta), oracle.FMI.from_text(tb)


@pytest.mark.parametrize("range_ratio", [0, 8])
def test_reads_of_mixed_lengths(gpu, oracle, range_ratio):
    """Chains end at different steps: classes that run empty, blocks whose elements lie in two or three rows of the table, blocks past the
    frontier; the first step reads the absolute frontier of k_frontier_init (ratio 0) or of range_expand (ratio 8)."""
    a, b = mixed_inputs(oracle)
    out = search_forms(gpu, oracle, a, b, 2, range_ratio, dict(threads=2))
    assert_forms(out, absolute=(0,), relative=(2,))
    for prof, _ in out.values():
        assert prof["frontier_step"][1] + prof.get("range_step", (0, 0))[1] >= 250, sorted(prof)
    assert ("range_step" in out[2][0]) == (range_ratio == 8)


def test_elements_beyond_the_staged_entries(gpu, oracle):
    """nb_max = 37 blocks per class, more than the 31 table entries a block stages: from step 9 on the 300 survivors fill two blocks whose
    classes lie 37 entries apart, so the lanes behind a class boundary find their segment by the binary search of seg_prefix and take
    their class from it."""
    ta = oracle.generate_reads(9400, 2500, 90)
    tb = np.concatenate([oracle.generate_reads(9600, 9000, 8), oracle.generate_reads(9601, 300, 120)])
    a, b = oracle.FMI.from_text(ta), oracle.FMI.from_text(tb)
    assert (b.sequences + 255) // 256 > 31
    out = search_forms(gpu, oracle, a, b, 2, 0, dict(threads=2))
    assert_forms(out, absolute=(0,), relative=(2,))
    assert out[2][0]["frontier_step"][1] >= 120


def test_iid_reads_above_the_frontier_threshold(gpu, oracle):
    """More than 2^21 iid reads: the dispatch itself picks the frontier search; every block of the early steps is full and holds all
    four classes."""
    b = oracle.FMI.from_text(oracle.generate_reads(7702, (1 << 21) + 70000, 16))
    a = oracle.FMI.from_text(oracle.generate_reads(7701, 120000, 100))
    assert b.sequences > (1 << 21)
    out = search_forms(gpu, oracle, a, b, 0, 0, dict(threads=8))
    assert_forms(out, absolute=(0,), relative=(2,))
    for prof, _ in out.values():
        assert prof["frontier_step"][1] >= 16 and "lf_walk" not in prof and "range_step" not in prof, sorted(prof)


def test_coordinates_beyond_32_bits(gpu, oracle):
    """a has 4.39 * 10^9 positions: the default knob takes the relative form, the first step reads the high bytes of the roots and no
    later step has any.  Every class is narrower than 2^32 and 2^32 falls inside a class (the last of the four bases; the few N
    follow it), so the absolute coordinates of that class need their high bytes while the offsets inside it do not."""
    a, b = wide_inputs(oracle)
    Ca = [int(v) for v in a.C]
    assert max(class_counts(a)) < (1 << 32) and max(class_counts(b)) < (1 << 32)
    inside = [c for c in range(1, 6) if Ca[c] < (1 << 32) < Ca[c + 1]]
    assert inside == [4] and sum(class_counts(a)[4:]) < (1 << 26), Ca
    gpu.tune("frontier_epoch", 5)
    try:
        out = search_forms(gpu, oracle, a, b, 2, 0, dict(capacity=1 << 21, threads=8), knobs=(0, 1))
    finally:
        gpu.tune("frontier_epoch", 0)
    assert_forms(out, absolute=(0,), relative=(1,))
    for prof, _ in out.values():
        assert prof["frontier_step"][1] >= 70, sorted(prof)


def test_guard_a_symbol_of_2_to_32_occurrences(gpu, oracle):
    """The same construction with the runs of one symbol four times as long, so that this symbol occurs 2^32 times or more in a
    (7.65 * 10^9 positions): the default knob must keep the absolute form.  The symbol is a's most frequent one (G, 9057 runs): with
    symbol 1 (8930 runs of 480 000 = 4.286 * 10^9 < 2^32) the guard would not bind."""
    small_a = oracle.FMI.from_text(oracle.generate_reads(9301, 600, 60)); small_b = oracle.FMI.from_text(oracle.generate_reads(9302, 500, 70))
    sym = small_a.symbols
    longest = 1 + int(np.argmax(np.bincount(sym, minlength=6)[1:6]))
    a = oracle.FMI.from_runs(sym.astype(np.uint64), np.where(sym == longest, 480000, 120000).astype(np.uint64))
    b = oracle.FMI.from_runs(small_b.symbols.astype(np.uint64), np.full(small_b.symbols.size, 2000, dtype=np.uint64))
    assert class_counts(a)[longest - 1] >= (1 << 32) and max(class_counts(b)) < (1 << 32)
    gpu.tune("frontier_epoch", 5)
    try:
        out = search_forms(gpu, oracle, a, b, 2, 0, dict(capacity=1 << 21, threads=8), knobs=(1,))
    finally:
        gpu.tune("frontier_epoch", 0)
    assert_forms(out, absolute=(1,), relative=())


def test_a_class_just_below_2_to_32(gpu, oracle):
    """The largest offsets the 32-bit entries must hold: the runs of symbol 1 four times as long give it 4.286 * 10^9 occurrences in a,
    0.2 % below 2^32, in an index of 7.6 * 10^9 positions whose other classes all begin beyond 2^32.  The default knob takes the
    relative form."""
    small_a = oracle.FMI.from_text(oracle.generate_reads(9301, 600, 60)); small_b = oracle.FMI.from_text(oracle.generate_reads(9302, 500, 70))
    sym = small_a.symbols
    a = oracle.FMI.from_runs(sym.astype(np.uint64), np.where(sym == 1, 480000, 120000).astype(np.uint64))
    b = oracle.FMI.from_runs(small_b.symbols.astype(np.uint64), np.full(small_b.symbols.size, 2000, dtype=np.uint64))
    assert (1 << 32) - (1 << 24) < max(class_counts(a)) == class_counts(a)[0] < (1 << 32) and int(a.C[2]) > (1 << 32)
    gpu.tune("frontier_epoch", 5)
    try:
        out = search_forms(gpu, oracle, a, b, 2, 0, dict(capacity=1 << 21, threads=8), knobs=(0, 1))
    finally:
        gpu.tune("frontier_epoch", 0)
    assert_forms(out, absolute=(0,), relative=(1,))


def test_step_kernel_inside_a_whole_merge(gpu, oracle):
    """The mixed-length inputs through merge_consume with the relative form: bytes and samples of the merged index against the oracle's."""
    a, b = mixed_inputs(oracle)
    A = gpu.Index.upload(a.data, a.sequences, a.bases); B = gpu.Index.upload(b.data, b.sequences, b.bases)
    gpu.tune("frontier_rel", 2); gpu.tune("search_algo", 2)
    gpu.profile_reset()
    try:
        M = gpu.merge_consume(A, B)
    finally:
        gpu.tune("frontier_rel", 1); gpu.tune("search_algo", 0)
    try:
        forms = gpu.frontier_step_forms()
        assert A.h is None and B.h is None
        assert forms[0] == 0 and forms[1] == 1 and forms[2] > 0, forms
        m, _ = oracle.merge(a, b, threads=2)
        assert np.array_equal(M.data(), m.data)
        be, cum = M.samples(); obe, ocum = m.samples
        assert np.array_equal(be, obe) and np.array_equal(cum, ocum)
    finally:
        M.free()
        gpu.trim()
