"""The recipes of tests/boundary_inputs.py have exactly the sizes they are named after: positions, sequences, native bytes, blocks and, for
pairs, a.bases + b.bases -- checked against the CPU oracle alone (no GPU), so that a recipe that drifts off its boundary by one position
fails here and cannot silently empty tests/test_gpu_exact_sizes.py."""
import numpy as np
import pytest

import boundary_inputs as bi
from locate_inputs import suffix_order


def test_the_size_lists_hold_the_units_and_their_neighbours():
    assert set(bi.SMALL_SIZES) >= {u + d for u in (64, 128, 3968, 8192, 65536) for d in (-1, 0, 1)} | {7936}
    assert bi.SUPER_SIZES == (2**25 - 1, 2**25, 2**25 + 1, 2**26) and bi.GROUP_BYTES == 3968
    assert len(bi.SMALL_STREAMS) == 2 * len(bi.SMALL_SIZES) + 1 and ("pure", 65536) in bi.SMALL_STREAMS


@pytest.mark.parametrize("n", bi.SMALL_SIZES)
def test_alternating_streams_have_one_byte_per_position(oracle, n):
    sym = bi.alternating(n)
    assert sym.size == n and np.all(sym[1:] != sym[:-1])
    f = oracle.FMI.from_symbols(sym)
    assert (f.bases, f.nbytes, f.blocks) == (n, n, (n + 63) // 64)
    assert f.sequences == (n + 5) // 6 and np.array_equal(f.symbols, sym)
    if n == 3968:
        assert (n // 128, f.blocks // 62, f.blocks % 62, f.nbytes % bi.GROUP_BYTES) == (31, 1, 0, 0)      # 31 records, exactly one group
    if n == 7936:
        assert (n // 128, f.blocks // 62, f.blocks % 62, f.nbytes % bi.GROUP_BYTES) == (62, 2, 0, 0)      # 62 records, two groups


@pytest.mark.parametrize("n", bi.SMALL_SIZES)
def test_run_streams_are_cut_to_their_size_and_keep_long_runs(oracle, n):
    sym = bi.run_stream(n)
    f = oracle.FMI.from_symbols(sym)
    assert sym.size == n and f.bases == n and np.array_equal(f.symbols, sym)
    assert f.nbytes < n // 3                                                # long runs, few bytes
    assert f.sequences == int(np.count_nonzero(sym == 0))


def test_the_pure_stream_is_one_run_of_a_segment(oracle):
    sym = bi.small_stream("pure", 65536)
    f = oracle.FMI.from_symbols(sym)
    assert (f.bases, f.sequences, f.blocks) == (65536, 0, 1) and np.unique(sym).tolist() == [3] and f.nbytes <= 4


@pytest.mark.parametrize("n", bi.SUPER_SIZES)
def test_super_sized_streams(oracle, n):
    sym = bi.super_stream(n)
    f = oracle.FMI.from_symbols(sym)
    assert sym.size == n and f.bases == n and f.sequences == int(np.count_nonzero(sym == 0))
    assert (n >> 25) + 1 == {2**25 - 1: 1, 2**25: 2, 2**25 + 1: 2, 2**26: 3}[n]                            # num_supers: the last row describes nothing
    assert f.nbytes < n // 100 and np.unique(sym[-100000:]).size == 6                                      # long runs of every symbol up to the end


@pytest.mark.parametrize("name", sorted(bi.READ_PAIRS))
def test_read_pairs_have_their_exact_n_out(oracle, name):
    (ra, la), (rb, lb) = bi.read_pair(oracle, name)
    a = oracle.FMI.from_text(bi.text_of(ra, la)); b = oracle.FMI.from_text(bi.text_of(rb, lb))
    n_out = bi.N_OUT[name]
    assert a.bases + b.bases == n_out and (a.sequences, b.sequences) == (ra.shape[0], rb.shape[0])
    assert a.bases == int(la.sum()) + la.size and b.bases == int(lb.sum()) + lb.size
    if name.isdigit():
        assert n_out == int(name) and 0.55 < a.bases / n_out < 0.65                                        # about 60 / 40
    if name == "a_65536":
        assert a.bases == 65536 and b.bases % 8192 != 0
    if name == "b_65536":
        assert b.bases == 65536 and a.bases % 8192 != 0
    m, _ = oracle.merge(a, b, threads=2)
    assert (m.bases, m.sequences) == (n_out, la.size + lb.size)
    assert (n_out >> 7) + 1 == {8191: 64, 8192: 65, 8193: 65, 65535: 512, 65536: 513, 65537: 513, 131072: 1025}.get(n_out, (n_out >> 7) + 1)


def test_every_wanted_n_out_has_a_pair():
    assert {bi.N_OUT[k] for k in bi.READ_PAIRS if k.isdigit()} == {8191, 8192, 8193, 65535, 65536, 65537, 131072}
    assert {"a_65536", "b_65536"} <= set(bi.READ_PAIRS)


@pytest.fixture(scope="module")
def chain(oracle):
    a, b = bi.chain_base(oracle)
    sizes = (a.bases, a.sequences, b.bases, b.sequences)
    m, _ = oracle.merge(a, b, threads=2)
    return sizes, m


def test_the_chain_base_is_512_positions_short_of_a_super_block(chain):
    sizes, m = chain
    assert sizes == (25_165_824, 1_572_864, 8_388_096, 524_256)
    assert m.bases == bi.CHAIN_BASE == 2**25 - 512 == 33_553_920 and m.sequences == 2_097_120


@pytest.mark.parametrize("name,positions,sequences,nbytes", [("511", 511, 16, 3534), ("512", 512, 17, 3534), ("513", 513, 17, 3514)])
def test_the_chain_tails_land_on_the_super_block(oracle, chain, name, positions, sequences, nbytes):
    _, base = chain
    rows, lengths = bi.chain_tail(oracle, name)
    tail = oracle.FMI.from_text(bi.text_of(rows, lengths))
    assert (tail.bases, tail.sequences) == (positions, sequences) and tail.bases == int(lengths.sum()) + lengths.size
    m, _ = oracle.merge(base.clone(), tail, threads=2)
    assert m.bases == 2**25 - 512 + positions == {"511": 2**25 - 1, "512": 2**25, "513": 2**25 + 1}[name]
    assert (m.sequences, m.nbytes, m.blocks) == (2_097_120 + sequences, nbytes, (nbytes + 63) // 64)


@pytest.mark.parametrize("name", sorted(bi.INGEST_SHAPES))
def test_ingest_shapes_have_their_suffix_totals(oracle, name):
    rows, lengths, total = bi.ingest_shape(oracle, name)
    assert total == bi.INGEST_SHAPES[name]
    if lengths is None:
        assert rows.shape[0] * (rows.shape[1] + 1) == total and np.all(rows > 0)
        lengths = np.full(rows.shape[0], rows.shape[1], dtype=np.uint32)
    else:
        assert int(lengths.sum()) + lengths.size == total
        assert all(np.all(rows[k, : int(lengths[k])] > 0) and np.all(rows[k, int(lengths[k]):] == 0) for k in range(rows.shape[0]))
    f = oracle.FMI.from_text(bi.text_of(rows, lengths))
    assert (f.bases, f.sequences) == (total, rows.shape[0])


def test_ingest_totals_cover_the_tile_and_grid_edges():
    assert set(bi.INGEST_SHAPES.values()) == {256, 512, 4095, 4096, 4097, 8192, 12288}


def test_the_walks_give_the_sequences_and_the_suffix_order(oracle):
    """sequence_by_walk and locate_by_walk (what the 2^25 cases expect) against the reads and the sorted suffixes of a small pair."""
    (ra, la), (rb, lb) = bi.read_pair(oracle, "8191")
    rows, lengths = np.concatenate([ra, rb]), np.concatenate([la, lb])
    m = oracle.FMI.from_text(bi.text_of(rows, lengths))
    for j in (0, 1, 152, 153, rows.shape[0] - 1):
        assert np.array_equal(bi.sequence_by_walk(m, j), rows[j, : int(lengths[j])]), j
    ids, offs = suffix_order(rows, lengths)
    C = m.C
    for p in list(range(0, m.bases, 97)) + [rows.shape[0] - 1, rows.shape[0], m.bases - 1]:
        assert bi.locate_by_walk(m, p, C) == (int(ids[p]), int(offs[p])), p
