"""The streamed host-to-host merge (bwtm_merge_host_streamed): the checks tests/test_gpu_streamed_merge.py runs, and the child process it
starts for the cases on poisoned device memory (not a test module).
Usage: python streamed_child.py            (the read sets at 1024 records per slice, then `long_runs` at 512)

The library reads BWTM_POOL_POISON once per process, so the parent sets the environment and starts one child per word.  Every case is
compared bit for bit with the CPU oracle here; the child also prints "DIGEST <sha256 of every array it got>", which the parent compares
across the words, then "POISON fills=<n> bytes=<n>" (bwtm_pool_poison_stats) and "OK"."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

READ_SETS = ((9001, 5000, 100), (9002, 4000, 100))       # as in test_gpu_slices.py: 0.9 Mbase = 14 encoder segments
NONE, FULL, COMPACT = 0, 1, 2
MIB = 1 << 20


def inp(f):
    return (f.data, f.sequences, f.bases)


def read_sets(orc):
    a = orc.FMI.from_text(orc.generate_reads(*READ_SETS[0])); b = orc.FMI.from_text(orc.generate_reads(*READ_SETS[1]))
    m, _ = orc.merge(a.clone(), b.clone(), threads=2)
    return a, b, m


def long_run_symbols(case):
    """The strings of test_slices_across_long_runs (same generator, same seed)."""
    from test_gpu_parity import run_symbols
    rng = np.random.default_rng(17)
    if case == "long_runs":
        return run_symbols(rng, 3000, [1, 2, 3, 41, 42, 43, 170, 3000, 16426, 100000, 400000])
    if case == "one_run":
        return np.concatenate([np.full(7, 2, np.uint8), np.full(3_000_000, 4, np.uint8), np.full(5, 1, np.uint8)])
    if case == "runs_on_cuts":
        sym = np.concatenate([np.full(65536, 1 + (k % 5), np.uint8) if k % 3 else run_symbols(rng, 1, [65536]) for k in range(40)])
        return np.concatenate([sym, run_symbols(rng, 50000, [1, 2, 3])])
    assert case == "tiny"
    return run_symbols(rng, 30, [1, 2, 50])


def collect(pkg, a, b, slice_records, samples, chained=None):
    """The pieces as the sink saw them, the call's header and statistics."""
    pieces = []
    out, stats = pkg.capi.merge_host_streamed(a, b, slice_records, samples, chained=chained, sink=lambda p: pieces.append(p) and False)
    return pieces, out, stats


def check_pieces(pieces, out, stats, want):
    """What holds for the pieces of every streamed merge: byte ranges and sample ranges are contiguous, exactly one piece is the last
    one (the final one), every piece but that one carries something, and the counts of the header agree."""
    assert stats.pieces == len(pieces) >= 1
    assert [p.last for p in pieces] == [False] * (len(pieces) - 1) + [True]
    at_byte = at_block = 0
    for p in pieces:
        assert p.byte_first == at_byte and p.data.size == p.nbytes
        assert p.nbytes > 0 or p.sample_blocks > 0 or p.last
        if want == NONE:
            assert p.sample_width == 0 and p.sample_blocks == 0
        if p.sample_blocks > 0:
            assert p.sample_block_first == at_block
            assert p.sample_width == 8 if want == FULL else p.sample_width in (1, 2, 4, 8)
        at_byte += p.nbytes; at_block += p.sample_blocks
    assert at_byte == out.nbytes and out.blocks == (out.nbytes + 63) // 64
    assert at_block == (out.blocks if want != NONE else 0)
    assert not out.data and not out.block_end and not out.cum and not out.fields and not out.anchors        # the pointers stay NULL


def narrowest(pieces):
    """The compact rule per piece: the narrowest width that holds the longest block of the piece's sample range."""
    for p in pieces:
        if p.sample_blocks > 0 and p.sample_width != 8:
            mx = int(p.fields[0].max())
            assert p.sample_width == (1 if mx < 0xFF else 2 if mx < 0xFFFF else 4), (p.sample_block_first, mx, p.sample_width)


def check_streamed(pkg, a, b, m, slice_records, oneshot=None, chained=None, bound=False):
    """One streamed merge of a and b in every form of the samples against the oracle FMI m: bytes, header, the full samples, the compact
    samples under both settings of the stream_samples_query knob (equal to each other, to the one-shot call's compact arrays when given,
    and, expanded, to the oracle's).  chained: a callable that returns the device index to pass in place of a.  Returns the arrays."""
    capi = pkg.capi
    obe, ocum = m.samples
    first = (lambda: None) if chained is None else chained
    got = []
    pieces, out, stats = collect(pkg, a, b, slice_records, NONE, chained=first())
    check_pieces(pieces, out, stats, NONE)
    data, width, x, y = capi.assemble_pieces(pieces, list(out.C))
    assert width == 0 and np.array_equal(data, m.data)
    assert (out.sequences, out.bases, out.nbytes, out.blocks) == (m.sequences, m.bases, m.nbytes, m.blocks)
    assert np.array_equal(np.array(list(out.C), dtype=np.uint64), m.C)
    got.append(data)

    pieces, out, stats = collect(pkg, a, b, slice_records, FULL, chained=first())
    check_pieces(pieces, out, stats, FULL)
    data, width, be, cum = capi.assemble_pieces(pieces, list(out.C))
    assert width == 8 and np.array_equal(data, m.data)
    assert np.array_equal(be, obe) and np.array_equal(cum, ocum)
    got += [be, cum]

    compact = []
    for knob in (0, 1):
        pkg.tune("stream_samples_query", knob)
        try:
            pieces, out, stats = collect(pkg, a, b, slice_records, COMPACT, chained=first())
        finally:
            pkg.tune("stream_samples_query", 0)
        check_pieces(pieces, out, stats, COMPACT)
        narrowest(pieces)
        data, width, fields, anchors = capi.assemble_pieces(pieces, list(out.C))
        assert np.array_equal(data, m.data), knob
        if width == 8:
            assert np.array_equal(fields, obe) and np.array_equal(anchors, ocum), knob
        else:
            xbe, xcum = capi.expand_samples(width, fields, anchors, m.blocks, m.bases)
            assert np.array_equal(xbe, obe) and np.array_equal(xcum, ocum), knob
        compact.append((width, fields, anchors))
        if bound:
            # records 64 B + native bytes <= 128 B + block starts and cum32 <= 56 B + size tables 0.5 B per record, two live slices;
            # 4 MiB for the super tables and the scratch at these sizes
            print("slice_records %d: slice_bytes_peak %d" % (slice_records, stats.slice_bytes_peak))
            assert stats.slice_records == slice_records
            assert 0 < stats.slice_bytes_peak <= 2 * 256 * slice_records + 4 * MIB, (slice_records, stats.slice_bytes_peak)
    assert compact[0][0] == compact[1][0] and np.array_equal(compact[0][1], compact[1][1]) and np.array_equal(compact[0][2], compact[1][2])
    if oneshot is not None:
        w, f, an = oneshot
        assert compact[0][0] == w and compact[0][1].dtype == f.dtype and np.array_equal(compact[0][1], f) and np.array_equal(compact[0][2], an)
    got += [compact[0][1], compact[0][2]]
    return got


def main():
    import _pkg
    from oracle import oracle as orc
    pkg = _pkg.load()
    pkg.init(0)
    digest = hashlib.sha256()
    a, b, m = read_sets(orc)
    for x in check_streamed(pkg, inp(a), inp(b), m, 1024):
        digest.update(np.ascontiguousarray(x).tobytes())
    f = orc.FMI.from_symbols(long_run_symbols("long_runs"))
    e = orc.FMI.from_symbols(np.zeros(0, dtype=np.uint8))
    for x in check_streamed(pkg, inp(f), inp(e), f, 512):
        digest.update(np.ascontiguousarray(x).tobytes())
    pkg.synchronize()
    print("DIGEST %s" % digest.hexdigest())
    print("POISON fills=%d bytes=%d" % pkg.pool_poison_stats())
    print("OK")


if __name__ == "__main__":
    main()
