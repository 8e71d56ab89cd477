"""An exact certificate for a multi-string BWT: invert it and compare with the reads it was built from.

Theorem.  Let M be a string over {0..5} with m zeros and T_0 .. T_{m-1} an ordered collection over {1..5}.  M is the BWT of
the collection (endmarkers smallest, equal suffixes ordered by sequence index: the order bwt_merge produces, SURVEY.md
section 4) IF AND ONLY IF, for every k < m, walking LF over M from row k spells T_k backwards and stops on a 0, and the m
walks together visit all |M| rows.

  LF(i) = #{j : M[j] < M[i]} + #{j < i : M[j] = M[i]}: the place of row i in a stable counting sort of M.  Row LF(i) is the
  row of the suffix M[i] . S(i), where S(i) is the suffix of row i.
  (=>) is the definition of the BWT.  (<=) The first m rows are the suffixes "$_k" in sequence order by the convention
  row k <-> sequence k.  The rows of the block of a symbol c > 0 are c . S(p) in the order of their sources p, because LF is
  stable per symbol; so if the sources are sorted (first symbol by the blocks, then the rest by induction on the suffix
  length, ties between ended suffixes by sequence index), the block is.  Every row that a walk reaches therefore holds the
  suffix the walk has spelled, in sorted order; full coverage excludes rows on cycles that no endmarker row reaches.
  LF is a bijection and no walk steps through a 0, so the walks are simple and pairwise disjoint: counting their steps counts
  the rows visited.

Nothing here knows a rank structure, a suffix sort, the product package or the oracle: LF is a stable partition of the rows by
symbol in numpy, and all m walks advance together with one gather per step (slices of the rows and of the walks on a few
threads).  certify_native() adds the two linear codec checks that extend the verdict from the symbols to every byte of a native
stream and its samples; the codec is the caller's (the oracle's, which the suite pins to the reference's vectors).

Not covered: the SDSL framing of files on disk (headers, int_vector layout), and anything about speed.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

SIGMA = 6
THREADS = max(1, min(16, os.cpu_count() or 1))


def _pool_map(fn, jobs, threads):
    """fn over jobs on `threads` threads (numpy releases the interpreter lock inside its loops); results in order."""
    if threads <= 1 or len(jobs) <= 1:
        return [fn(*j) for j in jobs]
    with ThreadPoolExecutor(threads) as pool:
        return list(pool.map(lambda j: fn(*j), jobs))


def _ranges(n, pieces):
    bounds = [n * k // pieces for k in range(pieces + 1)]
    return [(bounds[k], bounds[k + 1]) for k in range(pieces) if bounds[k + 1] > bounds[k]]


def lf_mapping(symbols, threads=THREADS):
    """LF as an int64 array: a stable counting sort of the rows by symbol (slices of the rows are counted, then placed, side by side)."""
    n = symbols.size
    lf = np.empty(n, dtype=np.int64)
    slices = _ranges(n, max(1, min(4 * threads, n >> 16)))
    counts = np.array(_pool_map(lambda lo, hi: np.bincount(symbols[lo:hi], minlength=256), slices, threads), dtype=np.int64).reshape(len(slices), 256)
    total = counts.sum(axis=0)
    first = np.concatenate([[0], np.cumsum(total)[:-1]])                     # first row of each symbol's block
    before = first[None, :] + np.cumsum(counts, axis=0) - counts             # ... and where each slice's rows of that symbol begin in it

    def place(k, lo, hi):
        part, out = symbols[lo:hi], lf[lo:hi]
        for c in np.flatnonzero(counts[k]):
            rows = np.flatnonzero(part == c)
            out[rows] = np.arange(before[k, c], before[k, c] + rows.size, dtype=np.int64)

    _pool_map(place, [(k, lo, hi) for k, (lo, hi) in enumerate(slices)], threads)
    return lf


def _walk(symbols, lf, lo, hi, max_len):
    """The walks from rows lo .. hi-1, all advancing together: -> (forward matrix [hi - lo, width], lengths, rows visited)."""
    m = hi - lo
    lengths = np.zeros(m, dtype=np.int64)
    cap = max_len if max_len is not None else 128
    back = np.zeros((cap, m), dtype=np.uint8)                  # back[t, k] = the symbol t places before the end of sequence lo + k
    ids = np.arange(m, dtype=np.int64)                         # walks still going, ascending
    pos = ids + lo
    visited = 0
    t = 0
    while ids.size:
        c = symbols[pos]
        visited += ids.size
        go = c != 0
        if not go.all():
            ids, pos, c = ids[go], pos[go], c[go]
        if ids.size == 0:
            break
        if t == cap:
            if max_len is not None:
                lengths[ids] = max_len + 1
                break
            back = np.concatenate([back, np.zeros_like(back)]); cap *= 2
        if ids.size == m:
            back[t] = c
        else:
            back[t, ids] = c
        lengths[ids] = t + 1
        pos = lf[pos]
        t += 1
    shown = np.minimum(lengths, cap)
    out = np.zeros((m, int(shown.max()) if m else 0), dtype=np.uint8)
    for L in np.unique(shown):
        L = int(L)
        if L == 0:
            continue
        rows = np.flatnonzero(shown == L)
        if rows.size == m:
            out[:, :L] = back[L - 1::-1].T
        else:
            out[rows, :L] = back[L - 1::-1][:, rows].T
    return out, lengths, visited


def invert(symbols, sequences, max_len=None, threads=THREADS):
    """Walks LF from rows 0 .. sequences-1 until each walk reads a 0.
    -> (matrix [sequences, width] uint8: sequence k in forward order, zero after its end; lengths int64 [sequences]; rows visited).
    max_len: walks that have not read a 0 after max_len symbols are cut there and get the length max_len + 1 (their row of the
    matrix holds the LAST max_len symbols); by default the walks run to their ends, which a walk always reaches (see the module
    docstring) -- after at most len(symbols) steps."""
    symbols = np.ascontiguousarray(symbols, dtype=np.uint8).reshape(-1)
    m, n = int(sequences), symbols.size
    if m > n:
        raise ValueError("invert: %d sequences in %d symbols" % (m, n))
    lf = lf_mapping(symbols, threads)
    chunks = _ranges(m, max(1, min(4 * threads, m >> 12)))
    parts = _pool_map(lambda lo, hi: _walk(symbols, lf, lo, hi, max_len), chunks, threads)
    del lf
    out = np.zeros((m, max([1] + [p[0].shape[1] for p in parts])), dtype=np.uint8)
    lengths = np.zeros(m, dtype=np.int64)
    for (lo, hi), (rows, lens, _) in zip(chunks, parts):
        out[lo:hi, :rows.shape[1]] = rows
        lengths[lo:hi] = lens
    return out, lengths, sum(p[2] for p in parts)


def _text(row):
    return "".join("$ACGTN"[v] if v < SIGMA else "?" for v in row.tolist())


def _row_lengths(reads):
    """Length of each zero-padded row: the index of its first zero."""
    if reads.shape[1] == 0:
        return np.zeros(reads.shape[0], dtype=np.int64)
    zero = reads == 0
    return np.where(zero.any(axis=1), zero.argmax(axis=1), reads.shape[1]).astype(np.int64)


def certify(symbols, reads, lengths=None):
    """None when `symbols` is the BWT of the ordered collection `reads` ([m, width] uint8, row k = sequence k, zero after its end;
    lengths: int [m], by default the index of each row's first zero), else a short diagnosis."""
    symbols = np.ascontiguousarray(symbols, dtype=np.uint8).reshape(-1)
    reads = np.asarray(reads, dtype=np.uint8)
    if reads.ndim != 2:
        raise ValueError("certify: reads must be an [m, width] matrix")
    m, width = reads.shape
    lengths = _row_lengths(reads) if lengths is None else np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lengths.size != m or (m and (int(lengths.min()) < 0 or int(lengths.max()) > width)):
        raise ValueError("certify: lengths do not fit the reads matrix")
    inside = np.arange(width, dtype=np.int64)[None, :] < lengths[:, None]
    if ((reads != 0) != inside).any() or (reads >= SIGMA).any():
        raise ValueError("certify: reads must hold 1..5 inside each sequence and 0 behind it")
    del inside
    expect_size = m + int(lengths.sum())
    if symbols.size != expect_size:
        return "wrong size: %d symbols, the collection has %d (%d sequences)" % (symbols.size, expect_size, m)
    counts = np.bincount(symbols, minlength=SIGMA)
    if counts.size > SIGMA:
        return "symbol %d is outside the alphabet" % int(np.flatnonzero(counts)[-1])
    if int(counts[0]) != m:
        return "wrong count of zeros: %d endmarkers for %d sequences" % (int(counts[0]), m)
    expect_counts = np.bincount(reads.reshape(-1), minlength=SIGMA)[:SIGMA]
    found, found_len, visited = invert(symbols, m, max_len=width)
    wrong = found_len != lengths
    if found.shape[1] == width or m == 0:
        wrong |= (found != reads).any(axis=1)
    else:
        wrong |= (found != reads[:, :found.shape[1]]).any(axis=1)
    notes = []
    if wrong.any():
        k = int(np.flatnonzero(wrong)[0])
        fl = int(found_len[k])
        shown = _text(found[k, :min(fl, found.shape[1])]) + ("" if fl <= width else " (cut: the walk did not end after %d symbols)" % width)
        notes.append("%d of %d sequences differ; first: sequence %d (walk from row %d): expected %s (%d), found %s (%d)"
                     % (int(wrong.sum()), m, k, k, _text(reads[k, :int(lengths[k])]), int(lengths[k]), shown, min(fl, width)))
    if visited != symbols.size:
        notes.append("rows not all visited: %d of %d rows lie on no walk" % (symbols.size - visited, symbols.size))
    if not notes and not np.array_equal(counts[1:], expect_counts[1:]):
        notes.append("symbol counts differ from the reads'")                 # cannot happen once every walk agrees; kept as a cross-check
    return "; ".join(notes) if notes else None


def certify_native(oracle, data, sequences, bases, block_end, cum, C, reads, lengths=None):
    """The same for a native byte stream with its samples (block_end [blocks], cum [6, blocks + 1]) and C array: the stream decodes (in
    `oracle`'s codec) to symbols whose canonical encoding -- Run::write's block rule -- is the same bytes, samples and C, and the symbols
    pass certify().  -> None or a diagnosis."""
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    f = oracle.FMI.from_native(data, int(sequences), int(bases))
    symbols = f.symbols
    del f
    if symbols.size != int(bases):
        return "the stream decodes to %d symbols, the header says %d" % (symbols.size, int(bases))
    g = oracle.FMI.from_symbols(symbols)
    if g.sequences != int(sequences):
        return "the stream holds %d endmarkers, the header says %d sequences" % (g.sequences, int(sequences))
    canonical = g.data
    if canonical.size != data.size or not np.array_equal(canonical, data):
        k = min(canonical.size, data.size)
        d = np.flatnonzero(canonical[:k] != data[:k])
        k = int(d[0]) if d.size else k
        return "the stream is not the canonical encoding of its symbols (%d bytes against %d; first difference at byte %d)" % (data.size, canonical.size, k)
    del canonical
    obe, ocum = g.samples
    block_end = np.asarray(block_end); cum = np.asarray(cum)
    if block_end.shape != obe.shape or not np.array_equal(block_end.astype(np.uint64), obe):
        return "block_end differs from the samples of the stream"
    if cum.shape != ocum.shape or not np.array_equal(cum.astype(np.uint64), ocum):
        return "cum differs from the samples of the stream"
    if not np.array_equal(np.asarray(C).astype(np.uint64).reshape(-1), g.C):
        return "C differs from the symbol counts of the stream: %s against %s" % (np.asarray(C).tolist(), g.C.tolist())
    del g
    return certify(symbols, reads, lengths)
