"""The host side of the streamed merge, without a GPU: the binding's piece assembly (a pure function) on synthetic pieces, and the
layouts of bwtm_piece / bwtm_stream_stats in the binding against the compiler's."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def whole_samples(rng, lengths):
    """A result of len(lengths) blocks: fields[6][blocks] (positions of the block, occurrences of 1..5 in it) as u64, the anchors, C."""
    blocks = lengths.size
    f = np.zeros((6, blocks), dtype=np.uint64)
    f[0] = lengths
    left = lengths.copy()
    for c in range(1, 6):                                        # split every block's positions over the six symbols (0 takes the rest)
        take = (left * rng.random(blocks) * 0.5).astype(np.uint64)
        f[c] = take; left -= take
    excl = np.cumsum(f, axis=1, dtype=np.uint64) - f
    anchors = excl[:, ::64].copy()
    counts = f[1:].sum(axis=1, dtype=np.uint64)
    bases = int(lengths.sum())
    counts0 = np.uint64(bases) - counts.sum(dtype=np.uint64)
    C = np.concatenate([[0], np.cumsum(np.concatenate([[counts0], counts]))]).astype(np.uint64)
    return f, anchors, bases, C


def width_of(mx):
    return 1 if mx < 0xFF else 2 if mx < 0xFFFF else 4 if mx < 0xFFFFFFFF else 8


def cut_into_pieces(capi, f, anchors, cuts, nbytes, full=False):
    """Pieces with the sample ranges [cuts[k], cuts[k + 1]) -- empty ranges allowed -- in the form the library delivers them."""
    blocks = f.shape[1]
    excl = np.cumsum(f, axis=1, dtype=np.uint64) - f
    pieces, at_byte = [], 0
    for k in range(len(cuts) - 1):
        lo, hi = cuts[k], cuts[k + 1]
        ns = hi - lo
        share = nbytes // (len(cuts) - 1) if k + 2 < len(cuts) else nbytes - at_byte
        p = SimpleNamespace(byte_first=at_byte, nbytes=share, data=np.full(share, k & 0xFF, dtype=np.uint8), sample_block_first=lo, sample_blocks=ns,
                            last=(k + 2 == len(cuts)), fields=None, anchors=None, block_end=None, cum=None, anchor_first=0, nanchors=0)
        at_byte += share
        w = width_of(int(f[0, lo:hi].max())) if ns > 0 else 1
        if full or w == 8:
            p.sample_width = 8
            if ns > 0:
                at = excl[:, lo:hi]
                p.block_end = at[0] + f[0, lo:hi] - np.uint64(1)
                p.cum = at.copy(); p.cum[0] = at[0] - at[1:].sum(axis=0, dtype=np.uint64)
        else:
            p.sample_width = w
            if ns > 0:
                p.fields = f[:, lo:hi].astype(capi.FIELD_DTYPES[w])
                p.anchor_first = (lo + 63) // 64
                p.nanchors = (hi + 63) // 64 - p.anchor_first
                p.anchors = anchors[:, p.anchor_first: p.anchor_first + p.nanchors].copy()
        pieces.append(p)
    return pieces


def test_piece_assembly_widens_and_concatenates(bwtm):
    capi = bwtm.capi
    rng = np.random.default_rng(5)
    blocks = 1000
    lengths = rng.integers(64, 200, blocks).astype(np.uint64)                  # width 1 ...
    lengths[300:340] = rng.integers(300, 60000, 40)                            # ... a stretch of width 2 ...
    lengths[641] = 3_000_000                                                   # ... and one block of width 4
    f, anchors, bases, C = whole_samples(rng, lengths)
    # cuts: an anchor on a piece's first sample block (64, 640), a piece without any anchor (65 .. 100), empty sample ranges (a slice with
    # bytes but no block start), a piece of one block
    cuts = [0, 64, 65, 100, 100, 320, 640, 641, 642, 642, 999, 1000]
    pieces = cut_into_pieces(capi, f, anchors, cuts, nbytes=64 * blocks - 17)
    assert sorted({p.sample_width for p in pieces if p.sample_blocks}) == [1, 2, 4]
    assert any(p.sample_blocks and p.sample_block_first % 64 == 0 and p.nanchors for p in pieces) and any(p.sample_blocks and not p.nanchors for p in pieces)
    data, width, fields, anch = capi.assemble_pieces(pieces, C)
    assert width == 4 and fields.dtype == np.uint32 and fields.shape == (6, blocks)
    assert np.array_equal(fields, f.astype(np.uint32)) and np.array_equal(anch, anchors)
    assert data.size == 64 * blocks - 17 and np.array_equal(data, np.concatenate([p.data for p in pieces]))
    whole = capi.expand_samples(4, f.astype(np.uint32), anchors, blocks, bases)
    got = capi.expand_samples(width, fields, anch, blocks, bases)
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    # the same pieces in the full form give the same arrays; the column behind the last block comes from C
    data8, width8, be, cum = capi.assemble_pieces(cut_into_pieces(capi, f, anchors, cuts, nbytes=64 * blocks - 17, full=True), C)
    assert width8 == 8 and np.array_equal(be, whole[0]) and np.array_equal(cum, whole[1])
    # a compact-mode merge in which one piece needs the full form: the compact pieces are expanded with it
    lengths[10] = (1 << 32) + 5
    f, anchors, bases, C = whole_samples(rng, lengths)
    pieces = cut_into_pieces(capi, f, anchors, [0, 5, 20, 64, 700, 1000], nbytes=64000)
    assert [p.sample_width for p in pieces] == [1, 8, 1, 4, 1]
    data, width, be, cum = capi.assemble_pieces(pieces, C)
    excl = np.cumsum(f, axis=1, dtype=np.uint64) - f
    assert width == 8 and np.array_equal(be, excl[0] + f[0] - np.uint64(1))
    assert np.array_equal(cum[1:, :-1], excl[1:]) and np.array_equal(cum[:, -1], C[1:] - C[:-1])


def test_piece_assembly_refuses_pieces_that_do_not_fit(bwtm):
    capi = bwtm.capi
    rng = np.random.default_rng(6)
    f, anchors, bases, C = whole_samples(rng, rng.integers(64, 200, 200).astype(np.uint64))
    good = lambda: cut_into_pieces(capi, f, anchors, [0, 70, 130, 200], nbytes=12800)
    assert capi.assemble_pieces(good(), C)[1] == 1
    for spoil in ("gap", "no_last", "two_last", "blocks"):
        pieces = good()
        if spoil == "gap":
            pieces[1].byte_first += 1
        elif spoil == "no_last":
            pieces[-1].last = False
        elif spoil == "two_last":
            pieces[0].last = True
        else:
            pieces[2].sample_block_first -= 1
        with pytest.raises(capi.BwtmError):
            capi.assemble_pieces(pieces, C)
    # without samples, and nothing at all
    empty = SimpleNamespace(byte_first=0, nbytes=0, data=np.zeros(0, np.uint8), sample_block_first=0, sample_blocks=0, sample_width=0, last=True,
                            fields=None, anchors=None, block_end=None, cum=None, anchor_first=0, nanchors=0)
    data, width, x, y = capi.assemble_pieces([empty], np.zeros(7, np.uint64))
    assert data.size == 0 and width == 0 and x is None and y is None
    empty.sample_width = 1
    data, width, fields, anch = capi.assemble_pieces([empty], np.zeros(7, np.uint64))
    assert width == 1 and fields.shape == (6, 0) and anch.shape == (6, 0)


def test_layouts_of_the_piece_and_the_statistics_match_the_header(bwtm, tmp_path):
    """The method of test_struct_layouts_of_the_binding_match_the_headers: the compiler's own sizes and offsets."""
    capi = bwtm.capi
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bwtm.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(bwtm_piece), offsetof(bwtm_piece, data), offsetof(bwtm_piece, sample_width),\n'
                   '  offsetof(bwtm_piece, fields), offsetof(bwtm_piece, anchor_first), offsetof(bwtm_piece, block_end), offsetof(bwtm_piece, cum), offsetof(bwtm_piece, last),\n'
                   '  sizeof(bwtm_stream_stats), offsetof(bwtm_stream_stats, slice_bytes_peak), offsetof(bwtm_stream_stats, ms_upload), offsetof(bwtm_stream_stats, ms_total)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    (size_piece, off_data, off_width, off_fields, off_anchor_first, off_block_end, off_cum, off_last,
     size_stats, off_peak, off_upload, off_total) = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    P, S = capi.Piece, capi.StreamStats
    assert ctypes.sizeof(P) == size_piece
    assert (P.data.offset, P.sample_width.offset, P.fields.offset, P.anchor_first.offset, P.block_end.offset, P.cum.offset, P.last.offset) == \
        (off_data, off_width, off_fields, off_anchor_first, off_block_end, off_cum, off_last)
    assert ctypes.sizeof(S) == size_stats
    assert (S.slice_bytes_peak.offset, S.ms_upload.offset, S.ms_total.offset) == (off_peak, off_upload, off_total)
    assert any(n == "bwtm_merge_host_streamed" for n, _, _ in capi.SYMBOLS)
