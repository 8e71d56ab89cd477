"""The chunked upload (bwtm_index_upload_streamed): the inputs and checks tests/test_gpu_upload_streamed.py runs, and the child process it
starts for the cases on poisoned device memory (not a test module).
Usage: python upload_streamed_child.py     (one run-length mix at three chunk sizes, then the chunk-edge shapes at one group per chunk)

The library reads BWTM_POOL_POISON once per process, so the parent sets the environment and starts the child.  Every case is compared bit
for bit with the CPU oracle; the last lines on stdout are "POISON fills=<n> bytes=<n>" (bwtm_pool_poison_stats) and "OK"."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

BLOCK = 64
GROUP_BYTES = 62 * BLOCK                                  # 3968: the smallest upload_chunk, one 62-block group per chunk
DEFAULT_CHUNK = 0                                         # bwtm_tune("upload_chunk", 0) restores the default (256 MiB)
CHUNKS = (GROUP_BYTES, 2 * GROUP_BYTES, 5 * GROUP_BYTES, DEFAULT_CHUNK)

# The eight run-length mixes of upload_cases (test_gpu_parity.py) with the number of runs: enough for several groups at every mix (the dense
# ones: one byte per run) or at least two (the mixes of giant runs, whose position count grows 10^4 times faster than their bytes).
MIXES = (([1, 1, 1, 2, 3], 20000), ([2, 3, 4], 20000), ([1, 2, 41, 42, 43, 169, 170, 5000], 9000), ([16425, 16426, 100000, 1, 7], 1600),
         ([9, 12, 17, 23, 31, 32, 33, 41], 20000), ([5, 20, 42, 60, 83, 90, 168, 169, 170, 400], 14000), ([3, 8, 40000, 14, 70000, 21], 2200),
         ([2, 3, 4, 5, 6, 8, 10], 20000))


def mix_symbols(k):
    from test_gpu_parity import run_symbols
    lengths, nruns = MIXES[k]
    return run_symbols(np.random.default_rng(100 + k), nruns, lengths)


def singles(n, first=1):
    """n runs of one position each (one byte each): symbols first, first + 1, ... cycling through 1..5."""
    return ((np.arange(n) + first - 1) % 5 + 1).astype(np.uint8)


EDGE_NAMES = ("empty", "one_byte", "less_than_a_block", "one_group", "one_group_and_a_byte", "one_group_and_a_block", "three_groups",
              "partial_last_block", "giant_group")


def edge_shapes():
    """(name, symbols, native bytes the oracle must give or None): the streams whose ends fall on, before and behind the edges of a chunk of
    one group, of its lookahead blocks and of a block."""
    big = np.concatenate([singles(GROUP_BYTES + 30), np.full(3_000_000, 4, np.uint8), singles(20, 2), np.full(70_000, 2, np.uint8),
                          singles(2 * GROUP_BYTES + 11, 3)])
    return [("empty", np.zeros(0, np.uint8), 0), ("one_byte", singles(1), 1), ("less_than_a_block", singles(37), 37),
            ("one_group", singles(GROUP_BYTES), GROUP_BYTES), ("one_group_and_a_byte", singles(GROUP_BYTES + 1), GROUP_BYTES + 1),
            ("one_group_and_a_block", singles(GROUP_BYTES + BLOCK), GROUP_BYTES + BLOCK), ("three_groups", singles(3 * GROUP_BYTES), 3 * GROUP_BYTES),
            ("partial_last_block", singles(2 * GROUP_BYTES + 5 * BLOCK + 17), 2 * GROUP_BYTES + 5 * BLOCK + 17), ("giant_group", big, None)]


def upload_streamed(pkg, f, chunk, uniform=0, C_array=None, header=None):
    """bwtm_index_upload_streamed under the two knobs, both restored afterwards."""
    sequences, bases = (f.sequences, f.bases) if header is None else header
    pkg.tune("upload_chunk", chunk); pkg.tune("recs_uniform", uniform)
    try:
        return pkg.Index.upload_streamed(f.data, sequences, bases, C_array)
    finally:
        pkg.tune("upload_chunk", DEFAULT_CHUNK); pkg.tune("recs_uniform", 0)


def expected_chunks(nbytes, chunk):
    blocks = (nbytes + BLOCK - 1) // BLOCK
    groups = max(1, (blocks + 61) // 62)
    per_chunk = max(1, (chunk if chunk else 256 << 20) // GROUP_BYTES)
    return -(-groups // per_chunk), min(per_chunk, groups) * GROUP_BYTES


def check_upload(pkg, f, sym, rng, chunk, uniform=0, nq=4000):
    """The streamed upload of f (the oracle's FMI of sym) against the plain symbols -- extract, rank for all six symbols, inverse_select --
    and, encoded again, against the oracle's bytes and samples.  Returns the call's statistics."""
    from test_gpu_parity import check_index
    ix, stats = upload_streamed(pkg, f, chunk, uniform)
    try:
        assert (ix.sequences, ix.bases, ix.nbytes, ix.blocks) == (f.sequences, f.bases, 0, 0)       # records and super table only
        assert np.array_equal(ix.C, f.C)
        chunks, chunk_bytes = expected_chunks(f.nbytes, chunk)
        assert (stats.chunks, stats.chunk_bytes) == (chunks, chunk_bytes), (stats.chunks, stats.chunk_bytes, chunks, chunk_bytes)
        print("nbytes %d chunk %d: %d chunks of %d bytes, staging peak %d" % (f.nbytes, chunk, stats.chunks, stats.chunk_bytes, stats.staging_bytes_peak))
        assert 0 < stats.staging_bytes_peak <= 4 * stats.chunk_bytes + 65536
        check_index(ix, sym, rng, nq=nq)
        ix.encode()
        assert (ix.nbytes, ix.blocks) == (f.nbytes, f.blocks) and np.array_equal(ix.data(), f.data)
        be, cum = ix.samples()
        obe, ocum = f.samples
        assert np.array_equal(be, obe) and np.array_equal(cum, ocum)
    finally:
        ix.free()
    return stats


def check_edge_shape(pkg, orc, name, sym, nbytes, rng):
    f = orc.FMI.from_symbols(sym)
    assert nbytes is None or f.nbytes == nbytes, (name, f.nbytes, nbytes)
    if name == "giant_group":
        # the long runs lie in the second group: its records outnumber its neighbours' a thousandfold, and the stream goes on for groups
        assert f.nbytes > 3 * GROUP_BYTES and int(f.samples[0][61]) < GROUP_BYTES + 30 < 3_000_000 < int(f.samples[0][2 * 62 - 1])
    for uniform in (0, 1, -1):
        check_upload(pkg, f, sym, rng, GROUP_BYTES, uniform, nq=1000)


def main():
    import _pkg
    from oracle import oracle as orc
    pkg = _pkg.load()
    pkg.init(0)
    rng = np.random.default_rng(7)
    sym = mix_symbols(2)
    f = orc.FMI.from_symbols(sym)
    for chunk in (GROUP_BYTES, 2 * GROUP_BYTES, DEFAULT_CHUNK):
        check_upload(pkg, f, sym, rng, chunk, nq=1000)
    for name, sym, nbytes in edge_shapes():
        check_edge_shape(pkg, orc, name, sym, nbytes, rng)
    pkg.synchronize()
    print("POISON fills=%d bytes=%d" % pkg.pool_poison_stats())
    print("OK")


if __name__ == "__main__":
    main()
