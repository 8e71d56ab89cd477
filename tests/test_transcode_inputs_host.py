"""The recipes of tests/transcode_inputs.py do what they claim: proved with the CPU oracle, no GPU.

The class of a stream -- the kernel the upload launches for it -- is restated here from build_records (api/index.hip.h; ChunkedUpload::queue
in api/upload_stream.hip.h repeats it): per_group = positions / groups of 62 blocks, <= 6500 gives the window of 8192 positions, <= 14000
gives 16384, anything else 32768; the cooperative fill only with the 32768 window and positions / blocks > 400; the straight-line deposit
only with the 32768 window.  Everything else is computed from the oracle's bytes, symbols and samples (block_end): the start of every block,
of every group, and the kernel's window edges (S_g & ~127) + k W."""
import numpy as np
import pytest

import transcode_inputs as ti

_streams = {}


def stream(oracle, name):
    if name not in _streams:
        _streams[name] = ti.Stream(oracle, name)
    return _streams[name]


def stated_class(bases, nbytes):
    """build_records, word for word."""
    nblocks = (nbytes + 63) // 64
    ngroups = max(1, (nblocks + 61) // 62)
    per_group = bases // ngroups
    long_runs = nblocks > 0 and bases // nblocks > 400
    window = 8192 if per_group <= 6500 else (16384 if per_group <= 14000 else 32768)
    uniform = window == 32768
    return window, (window == 32768 and long_runs), uniform


def test_the_restated_dispatcher_agrees_with_the_recipes_helper():
    for bases, nbytes in ((0, 0), (1, 1), (6500 * 3, 3 * 3968), (6500 * 3 + 3, 3 * 3968), (14000 * 2, 2 * 3968), (14001 * 2, 2 * 3968), (401 * 62, 3968), (400 * 62, 3968)):
        assert ti.dispatch(bases, nbytes) == stated_class(bases, nbytes)
    assert ti.dispatch(10, 10, 16384, 1) == (16384, False, True) and ti.dispatch(10 ** 6, 100, 32768, -1) == (32768, True, False)
    assert ti.dispatch(10 ** 6, 100, 8192, 0) == (8192, False, False) and ti.dispatch(10, 10, 32768, 0) == (32768, False, True)
    assert sorted(ti.form_index(c, w, f, u) for c in (0, 1) for w, f in ((8192, False), (16384, False), (32768, False), (32768, True)) for u in (0, 1)) == list(range(16))
    assert ti.form_index(1, 32768, True, False) == 8 + 6 and ti.form_index(0, 16384, False, True) == 3


@pytest.mark.parametrize("name", ti.STREAMS)
def test_size_class_and_symbols(oracle, name):
    s = stream(oracle, name)
    assert 0 < s.bases <= ti.MAX_POSITIONS and 0 < s.nbytes <= ti.MAX_BYTES
    assert stated_class(s.bases, s.nbytes) == ti.DEFAULT_CLASS[name], (s.bases, s.nbytes)
    if s.canonical is None:
        # the oracle did not coalesce anything: the runs are the recipe's
        assert np.array_equal(s.symbols, np.repeat(s.run_syms.astype(np.uint8), s.run_lens.astype(np.int64)))
        assert np.all(s.run_syms[1:] != s.run_syms[:-1])
    bs = s.block_starts()
    assert bs.size == s.blocks + 1 and bs[-1] == s.bases and np.all(np.diff(bs) > 0)
    assert s.sequences == int(np.count_nonzero(s.symbols == 0))


def test_model_of_the_writer_matches_the_oracle(oracle):
    """Writer (the model the steered recipes are written with) predicts the oracle's byte count and block starts."""
    w = ti.Writer()
    rng = np.random.default_rng(5)
    for length in rng.choice([1, 1, 1, 2, 41, 42, 43, 169, 170, 171, 16425, 16426, 16427, 100000, 2097193, 2097194], 3000):
        w.run(int(length))
    f = oracle.FMI.from_runs(*w.runs())
    assert f.nbytes == w.nbytes and f.bases == w.pos
    assert np.array_equal(np.concatenate([[0], f.samples[0].astype(np.int64) + 1])[:-1], np.array(w.block_start))


def test_groups_disagree_with_the_average(oracle):
    """What makes the three density mixes `mixed`: the smallest and the largest group of each against the window its class gives it."""
    s = stream(oracle, "dense_with_giants")
    gp = s.group_positions()
    giant = int(np.argmax(gp))
    assert ti.DEFAULT_CLASS[s.name][0] == 8192 and gp.max() > 100_000 and gp.max() > 12 * 8192      # a dozen windows of the smallest kernel
    assert 0 < giant < gp.size - 1 and np.median(gp) < 6500
    syms, lens = ti.runs_of(s.symbols)
    k = int(np.flatnonzero(lens == 40001)[0])
    assert syms[k] == 0 and lens[k - 1] == 70000 and lens[k + 1] == 33000 and syms[k - 1] != 0 and syms[k + 1] != 0
    assert np.count_nonzero(lens < 42) >= 390_000

    s = stream(oracle, "giants_with_dense")
    gp = s.group_positions()
    assert ti.DEFAULT_CLASS[s.name] == (32768, True, True) and s.bases // s.blocks > 400 and s.bases // gp.size > 14000
    assert gp.min() < 8192 and np.count_nonzero(gp < 8192) >= 10 and gp.max() > 3 * 32768            # dense groups in the kernel of the long runs

    s = stream(oracle, "mid_mixed")
    gp = s.group_positions()
    assert ti.DEFAULT_CLASS[s.name][0] == 16384 and 6500 < s.bases // gp.size <= 14000
    assert gp[:-1].min() < 8192 and gp.max() > 6 * 16384
    lens = ti.runs_of(s.symbols)[1]
    assert set(np.unique(lens).tolist()) >= {1, 2, 3, 9, 12, 17, 23, 31, 32, 33, 41, 42, 170}


class Layout:
    """Blocks, groups and maximal runs of a stream against the kernel's edges for windows of W positions."""

    def __init__(self, s, W):
        self.W = W
        self.bs = s.block_starts()
        self.blocks = self.bs.size - 1
        self.base_of_block = s.window_bases()[np.arange(self.blocks) // ti.GROUP]
        self.syms, self.lens = ti.runs_of(s.symbols)
        self.lens = self.lens.astype(np.int64)
        self.starts = np.concatenate([[0], np.cumsum(self.lens)[:-1]])
        self.ends = self.starts + self.lens
        self.run_block = np.searchsorted(self.bs, self.starts, side="right") - 1              # the block that holds the run's (first) head
        self.run_base = self.base_of_block[self.run_block]

    def on_edge(self, pos, base, shift=0):
        """pos - shift is an edge base + k W with k >= 1."""
        d = pos - shift - base
        return (d >= self.W) & (d % self.W == 0)


@pytest.mark.parametrize("W", ti.WINDOWS)
def test_edges_sit_on_the_kernels_window_edges(oracle, W):
    s = stream(oracle, "edges_%d" % W)
    L = Layout(s, W)
    b0, b1, base = L.bs[:-1], L.bs[1:], L.base_of_block
    assert np.any(L.on_edge(b0, base)), "a block that starts exactly on an edge"
    ends_on = L.on_edge(b1, base) & (b0 >= b1 - W) & (b0 >= base)
    assert np.any(ends_on[:-1]), "a block (not the last) that lies in one window and ends exactly on its edge"
    assert np.any(L.on_edge(b0, base, -1) & (b1 > b0 + 1)), "a block that starts one position before an edge"
    assert np.any(L.on_edge(b1, base, 1) & (b0 < b1 - 1)), "a block that ends one position behind an edge"
    long_run = L.lens >= ti.MAX_RUN
    for shift in (-1, 0, 1):
        assert np.any(long_run & L.on_edge(L.ends, L.run_base, shift)), "a long run that ends at edge %+d" % shift
    first_edge = L.run_base + ((L.starts - L.run_base + W - 1) // W) * W                      # the first edge at or behind the run's start
    assert np.any((L.syms != 0) & (L.ends >= first_edge + 3 * W)), "a non-zero run across three whole windows"
    inner = L.run_base + ((L.starts - L.run_base) // W + 1) * W                               # the first edge behind the run's start
    assert np.any((L.syms == 0) & (L.lens >= 128) & (inner >= L.run_base + W) & (L.starts < inner) & (inner < L.ends)), "endmarkers across an edge"
    assert L.on_edge(np.int64(s.bases), base[-1]) and s.nbytes % 64 != 0 and b0[-1] < s.bases, "the stream ends on an edge, inside a 64-byte block"


def test_fill_thresholds(oracle):
    s = stream(oracle, "fill_thresholds")
    assert s.bases // s.blocks > 400
    L = Layout(s, 32768)
    seen = {}
    for sym, start, length in zip(L.syms.tolist(), L.starts.tolist(), L.lens.tolist()):
        if sym != 0 and length in ti.THRESHOLD_RUNS:
            seen.setdefault((length, start % 32), set()).add(int(np.searchsorted(L.bs, start, side="right")) - 1)
    for length in ti.THRESHOLD_RUNS:
        for offset in ti.THRESHOLD_OFFSETS:
            assert len(seen.get((length, offset), ())) >= 2, (length, offset)                 # in more than one block
    # whole plane words inside a run of `length` that starts at bit `offset`: 3, 4 and 5 at offset 0; the branching body's `l >= 128` behind
    # the first word's completion is met exactly by 128 at offset 0 and by 159 at offset 1
    whole = {(length, offset): (offset + length) // 32 - (offset + 31) // 32 for length in ti.THRESHOLD_RUNS for offset in ti.THRESHOLD_OFFSETS}
    assert [whole[(length, 0)] for length in (96, 127, 128, 159, 160)] == [3, 3, 4, 4, 5]
    assert whole[(128, 1)] == 3 and whole[(129, 31)] == 4 and whole[(159, 1)] == 4 and whole[(161, 31)] == 5
    rest = {(length, offset): length - ((32 - offset) % 32) for length in ti.THRESHOLD_RUNS for offset in ti.THRESHOLD_OFFSETS}
    assert rest[(128, 0)] == 128 and rest[(127, 0)] == 127 and rest[(159, 1)] == 128 and rest[(129, 31)] == 128 and rest[(128, 31)] == 127


def test_tails(oracle):
    s = stream(oracle, "tail_no_record_in_last_group")
    bs = s.block_starts()
    assert s.blocks == ti.GROUP + 1 and s.bases - bs[ti.GROUP] < 128 and bs[ti.GROUP] % 128 != 0
    assert (bs[ti.GROUP] + 127) // 128 == (s.bases + 127) // 128                                # no record starts at or behind the group's start
    assert stream(oracle, "tail_two_blocks_in_last_group").blocks == ti.GROUP + 2
    assert stream(oracle, "tail_three_blocks_in_last_group").blocks == ti.GROUP + 3
    s = stream(oracle, "tail_one_whole_group")
    assert s.nbytes == ti.GROUP_BYTES and s.blocks == ti.GROUP


@pytest.mark.parametrize("name", [n for n in ti.STREAMS if n.startswith("rewritten")])
def test_rewritten_streams_are_valid_and_not_canonical(oracle, name):
    s = stream(oracle, name)
    c = s.canonical
    assert np.array_equal(s.symbols, c.symbols) and (s.sequences, s.bases) == (c.sequences, c.bases) and np.array_equal(s.f.C, c.C)
    assert s.nbytes != c.nbytes or not np.array_equal(s.data, c.data)
    runs = ti.decode(s.data)
    assert sum(r[1] for r in runs) == s.bases
    assert all(head // 64 == (end - 1) // 64 for _, _, head, end in runs), "a run's bytes cross a block"
    assert max(end - head for _, _, head, end in runs) <= 10
    # block starts by the plain decode == the oracle's; every full block holds at least 64 positions
    starts, pos = [], 0
    for _, length, head, _ in runs:
        if head % 64 == 0:
            starts.append(pos)
        pos += length
    bs = s.block_starts()
    assert np.array_equal(np.array(starts), bs[:-1])
    full = np.diff(bs)[: s.nbytes // 64]
    assert full.size == 0 or full.min() >= 64
    print("%s: %d bytes (canonical %d), sparsest full block %s positions" % (name, s.nbytes, c.nbytes, full.min() if full.size else None))
    # both kinds of rewriting occur: a maximal run cut into same-symbol runs, and a varint longer than it needs to be
    cut = sum(1 for k in range(1, len(runs)) if runs[k][0] == runs[k - 1][0])
    data = s.data.tolist()
    padded = sum(1 for _, length, head, end in runs if end - head >= 3 and data[end - 1] == 0)
    assert cut >= 20 and padded >= (5 if name == "rewritten_reads" else 20), (cut, padded)      # (a read set's BWT has few runs of 42 and more)
