"""Run-length streams for the transcode kernels (k_build_recs / k_build_recs_chunk, kernels/transcode.hip.h): recipes only, no GPU code.

The upload picks the kernel's LDS window (8192 / 16384 / 32768 positions), the cooperative fill and the deposit body from the stream's AVERAGE
density; the streams here are the ones whose groups disagree with their average, whose blocks and runs sit on the kernel's window edges on
purpose, whose runs meet the fill thresholds exactly, whose last group is degenerate, and -- rewritten() -- native bytes that Run::read decodes
but Run::write never writes.  tests/test_transcode_inputs_host.py proves each recipe's conditions with the CPU oracle;
tests/test_gpu_transcode_forms.py uploads them under every forced form.

A recipe returns (symbols, lengths) of MAXIMAL runs (adjacent runs differ), for oracle.FMI.from_runs.  The window edges of the kernel are
group-relative: (S_g & ~127) + k W for the start position S_g of the group's first block, so the steered recipes are written with a model of
Run::write (Writer) that knows at every moment the byte offset, the position and the start of every block.  Every stream holds at most
MAX_POSITIONS positions and MAX_BYTES bytes."""
import numpy as np

BLOCK = 64
GROUP = 62
GROUP_BYTES = GROUP * BLOCK
MAX_RUN = 42
REC_POS = 128
WINDOWS = (8192, 16384, 32768)
MAX_POSITIONS = 2_000_000
MAX_BYTES = 500_000


# ------------------------------------------------------------------------------------------------------------------------------------
# The dispatcher, restated (build_records in api/index.hip.h, ChunkedUpload::queue in api/upload_stream.hip.h)

def dispatch(bases, nbytes, recs_window=0, recs_uniform=0):
    """(window, fill, uniform) of the kernel an upload of `bases` positions in `nbytes` bytes launches under the two knobs."""
    nblocks = -(-nbytes // BLOCK)
    ngroups = max(1, -(-nblocks // GROUP))
    per_group = bases // ngroups
    long_runs = nblocks > 0 and bases // nblocks > 400
    window = recs_window if recs_window in WINDOWS else (8192 if per_group <= 6500 else (16384 if per_group <= 14000 else 32768))
    uniform = (recs_uniform > 0) if recs_uniform != 0 else (window == 32768)
    return window, (window == 32768 and long_runs), uniform


def form_index(chunk, window, fill, uniform):
    """The entry of bwtm_transcode_forms: 8 chunk + 2 w + uniform."""
    return 8 * int(chunk) + 2 * (0 if window == 8192 else (1 if window == 16384 else (3 if fill else 2))) + int(uniform)


# ------------------------------------------------------------------------------------------------------------------------------------
# Random mixes

def random_runs(rng, nruns, lengths, after=None):
    """nruns runs with lengths drawn from `lengths`; adjacent symbols differ, and the first one differs from `after`."""
    steps = rng.integers(1, 6, nruns)
    first = 0 if after is None else int(after)
    syms = (first + np.cumsum(steps)) % 6
    return syms.astype(np.uint64), rng.choice(np.asarray(lengths, dtype=np.uint64), nruns)


def joined(parts):
    syms = np.concatenate([p[0] for p in parts]).astype(np.uint64)
    lens = np.concatenate([p[1] for p in parts]).astype(np.uint64)
    assert np.all(syms[1:] != syms[:-1]) and np.all(lens > 0)
    return syms, lens


def nonzero_unlike(*avoid):
    return next(c for c in (1, 2, 3, 4, 5) if c not in [int(a) for a in avoid])


def dense_with_giants():
    """A read-like stream (the 8192-position branching kernel) with three giant runs in the middle: one group of more than 10^5 positions is
    walked as a dozen windows through the straddle body.  Of the one-byte runs, the share drawn from [1, 1, 1, 2, 3] is what the average
    allows: the rest are single positions."""
    rng = np.random.default_rng(4101)
    half = 200_000
    mix = [1] * 12 + [2, 3]                                           # (five runs in fourteen from [1, 1, 1, 2, 3], the others single positions)
    left = random_runs(rng, half, mix)
    a = nonzero_unlike(left[0][-1])
    right_first = random_runs(rng, half, mix)
    b = nonzero_unlike(right_first[0][0])
    giants = (np.array([a, 0, b], dtype=np.uint64), np.array([70000, 40001, 33000], dtype=np.uint64))
    return joined([left, giants, right_first])


def giants_with_dense():
    """Giant runs (32768 + FILL + UNIFORM by the average) around 6 x 10^4 read-like runs: dense groups in the kernel of the long runs."""
    rng = np.random.default_rng(4102)
    lengths = [100000, 65536, 32768, 4096, 131, 129, 128, 127]
    head = random_runs(rng, 20, lengths)
    dense = random_runs(rng, 60_000, [1, 1, 2, 3], after=head[0][-1])
    tail = random_runs(rng, 20, lengths, after=dense[0][-1])
    return joined([head, dense, tail])


def mid_mixed():
    """The 16384 window by the average: stretches of [1, 2, 3] (groups of under 8192 positions) around one stretch of runs about the
    one-byte limit and beyond (groups of more than 10^5)."""
    rng = np.random.default_rng(4103)
    first = random_runs(rng, 70_000, [1, 2, 3])
    rich = random_runs(rng, 3_600, [9, 12, 17, 23, 31, 32, 33, 41, 42, 170], after=first[0][-1])
    last = random_runs(rng, 60_000, [1, 2, 3], after=rich[0][-1])
    return joined([first, rich, last])


# ------------------------------------------------------------------------------------------------------------------------------------
# Steered streams

def run_cost(offset, length):
    """Bytes Run::write appends for a run of `length` at byte offset `offset` (support.h:256-282), and the positions at which it opens a new
    block (relative to the run's start): a run whose extension does not fit the block goes on behind a new head in the next one."""
    nbytes, left, opened = 0, length, []
    while left > 0:
        if (offset + nbytes) % BLOCK == 0:
            opened.append(length - left)
        if left < MAX_RUN:
            nbytes += 1
            break
        remaining = BLOCK - (offset + nbytes) % BLOCK
        basic = MAX_RUN if remaining > 1 else MAX_RUN - 1
        nbytes += 1; left -= basic; remaining -= 1
        if remaining > 0:
            ext = left
            if ext.bit_length() > 7 * remaining:
                ext = (1 << (7 * remaining)) - 1
            nbytes += max(1, -(-ext.bit_length() // 7)); left -= ext
    return nbytes, opened


class Writer:
    """The runs of a stream, with Run::write's byte offset, the position and the start position of every block as they grow."""

    def __init__(self):
        self.syms, self.lens, self.block_start = [], [], []
        self.nbytes = self.pos = 0

    def run(self, length, sym=None):
        """A run of `length`; without a symbol: the next of 1..5 that differs from the last run's."""
        length = int(length)
        last = self.syms[-1] if self.syms else 0
        sym = last % 5 + 1 if sym is None else sym
        assert length >= 1 and (not self.syms or sym != last)
        cost, opened = run_cost(self.nbytes, length)
        self.block_start += [self.pos + at for at in opened]
        self.syms.append(sym); self.lens.append(length)
        self.nbytes += cost; self.pos += length

    def singles(self, n):
        for _ in range(int(n)):
            self.run(1)

    def fresh_group(self):
        """Single positions up to the start of the next 62-block group; returns its start position S_g."""
        self.singles((-self.nbytes) % GROUP_BYTES)
        return self.pos

    def steer(self, target, byte_mod=None):
        """One long run and then k single positions, so that the position is `target`; k = 0 without byte_mod, otherwise the smallest k
        that leaves the byte offset at byte_mod modulo 64.  (A long run moves the position, single positions move the byte offset.)"""
        for k in range(0, 3 * BLOCK):
            length = target - self.pos - k
            assert length >= MAX_RUN
            if byte_mod is None or (self.nbytes + run_cost(self.nbytes, length)[0] + k) % BLOCK == byte_mod:
                self.run(length); self.singles(k)
                assert self.pos == target
                return
        raise AssertionError("steer: no k")

    def runs(self):
        return np.array(self.syms, dtype=np.uint64), np.array(self.lens, dtype=np.uint64)


def edges(W):
    """Blocks and runs on the edges (S_g & ~127) + k W of the kernel's windows of W positions; one scenario per group, each from the
    group's first byte:
      block_on_edge      a block that ends exactly on the first edge, the next one starts on it
      starts_one_before  a block that starts at edge - 1        ends_one_behind   a block that ends at edge + 1
      run_to_before / run_to_edge / run_to_behind   a long run that ends at edge - 1, at an edge (the second one), at edge + 1
      three_windows      a non-zero run across more than three whole windows
      endmarkers         300 endmarkers from edge - 100 on
      last               the stream ends exactly on an edge, in the middle of a 64-byte block."""
    w = Writer()

    def edge(k=1):
        return (w.fresh_group() & ~(REC_POS - 1)) + k * W

    w.steer(edge(), 0); w.singles(5)
    w.steer(edge() - 1, 0); w.singles(5)
    w.steer(edge() + 1, 0); w.singles(5)
    e = edge(); w.singles(20); w.steer(e - 1); w.singles(3)
    e = edge(2); w.singles(7); w.steer(e); w.singles(3)
    e = edge(); w.singles(41); w.steer(e + 1); w.singles(3)
    w.fresh_group(); w.singles(30); w.run(4 * W + 77); w.singles(3)
    e = edge(); w.steer(e - 100); w.run(300, sym=0); w.singles(3)
    w.steer(edge(), 37)
    return w.runs()


THRESHOLD_RUNS = (96, 127, 128, 129, 159, 160, 161)
THRESHOLD_OFFSETS = (0, 1, 31)


def fill_thresholds():
    """A stream of long runs (FILL by the average).  Non-zero runs of 96 .. 161 positions, each starting at bit 0, 1 and 31 of a plane word: 3,
    4 and 5 whole words in the straight-line deposit (4 and more go to the cooperative fill), `l >= 128` met or missed by one in the
    branching one.  The runs between them keep the class and set the next start's offset; their lengths vary from round to round, so that
    the runs under test fall into different blocks and records."""
    w = Writer()
    w.singles(3)
    for rnd in range(6):
        for length in THRESHOLD_RUNS:
            for offset in THRESHOLD_OFFSETS:
                between = 1500 + 97 * rnd
                between += (offset - (w.pos + between)) % 32
                w.run(between)
                assert w.pos % 32 == offset
                w.run(length)
    w.run(2000); w.singles(9)
    return w.runs()


TAILS = ("no_record_in_last_group", "two_blocks_in_last_group", "three_blocks_in_last_group", "one_whole_group")


def tail(name):
    """Four short streams by the shape of their last group."""
    w = Writer()
    if name == "no_record_in_last_group":
        # the second group is one block of 50 positions inside record 31, which the first group's wave owns
        w.run(10); w.singles(GROUP_BYTES - 1)
        assert w.nbytes == GROUP_BYTES and w.pos % REC_POS != 0
        w.singles(50)
        assert (w.pos - 1) // REC_POS == (w.pos - 50) // REC_POS
    elif name == "two_blocks_in_last_group":
        w.singles(GROUP_BYTES - 1); w.run(3); w.singles(BLOCK + 20)
    elif name == "three_blocks_in_last_group":
        w.singles(GROUP_BYTES - 1); w.run(3); w.singles(2 * BLOCK); w.run(300); w.singles(5)
    else:
        assert name == "one_whole_group"
        w.singles(GROUP_BYTES - 2); w.run(41); w.run(7)
        assert w.nbytes == GROUP_BYTES
    return w.runs()


# ------------------------------------------------------------------------------------------------------------------------------------
# The non-canonical writer

def rewritten(syms, lens, seed):
    """Native bytes of the runs that Run::read decodes to the same symbols and Run::write never writes: runs are cut into same-symbol pieces at
    random; a piece of fewer than 42 positions is one byte, any other is the head of 42 and a varint with 0 to 3 redundant continuation
    bytes (0x80 ... 0x00, zero payload) behind its last significant byte.  No piece's bytes cross a 64-byte boundary (a piece is cut to what
    the block still takes), at most 9 extension bytes (every shift stays below 64), and since every byte is a head of at least one position
    or one of at most 9 extension bytes behind a head of 42, every full block encodes at least 64 positions."""
    rng = np.random.default_rng(seed)
    syms = np.asarray(syms, dtype=np.int64).tolist(); lens = np.asarray(lens, dtype=np.int64).tolist()
    draws = rng.random(4096).tolist()
    at = 0
    out = bytearray()
    for s, left in zip(syms, lens):
        while left > 0:
            u, v = draws[at & 4095], draws[(at + 1) & 4095]
            at += 2
            piece = left
            if left > 1 and u < 0.35:
                piece = 1 + int(v * (left - 1))                      # 1 .. left - 1: the rest follows as a run of the same symbol
            room = BLOCK - len(out) % BLOCK
            if room == 1:
                piece = min(piece, MAX_RUN - 1)
            if piece < MAX_RUN:
                out.append(s + 6 * (piece - 1))
            else:
                most = min(room - 1, 9)
                value = piece - MAX_RUN
                nb = max(1, -(-value.bit_length() // 7))
                if nb > most:
                    nb = most; value = (1 << (7 * most)) - 1; piece = MAX_RUN + value
                extra = min(int(4 * draws[(at + 7) & 4095]), most - nb)
                out.append(s + 6 * (MAX_RUN - 1))
                for k in range(nb):
                    out.append(((value >> (7 * k)) & 0x7F) | (0x80 if (k + 1 < nb or extra > 0) else 0))
                for k in range(extra):
                    out.append(0x80 if k + 1 < extra else 0x00)
            left -= piece
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def decode(data):
    """Run::read over the bytes, in plain Python: (symbol, length, byte offset of the head) of every run."""
    data = np.asarray(data, dtype=np.uint8).tolist()
    runs, i = [], 0
    while i < len(data):
        head = i
        code = data[i]; i += 1
        sym, length = code % 6, code // 6 + 1
        if length >= MAX_RUN:
            shift = 0
            while True:
                b = data[i]; i += 1
                length += (b & 0x7F) << shift; shift += 7
                if not b & 0x80:
                    break
            assert shift <= 63
        runs.append((sym, length, head, i))
    return runs


def rewritten_dense():
    rng = np.random.default_rng(4201)
    return random_runs(rng, 60_000, [1] * 60 + [2] * 10 + [3] * 10 + [42, 43, 100])


def rewritten_long():
    rng = np.random.default_rng(4202)
    return random_runs(rng, 250, [41, 42, 43, 100, 130, 5000, 40000])


REWRITTEN = {"rewritten_dense": (rewritten_dense, 4301), "rewritten_long": (rewritten_long, 4302)}
READS_A = ((4401, 2500, 100), ((1, 60), (5, 40)))         # oracle.generate_reads(seed, reads, length) and (symbol, copies) of the reads of
READS_B = ((4402, 2000, 100), ((1, 30), (3, 7)))           # one symbol that follow them: the pair of the merge test
READS_SEED = 4303


def read_set(orc, spec):
    """Random reads and a few low-complexity ones (a poly-A or N stretch): their BWT is read-like with some long runs."""
    (seed, reads, length), poly = spec
    one = [np.concatenate([np.full(length, c, np.uint8), np.zeros(1, np.uint8)]) for c, copies in poly for _ in range(copies)]
    return np.concatenate([orc.generate_reads(seed, reads, length)] + one)


def runs_of(symbols):
    """Maximal runs of a symbol array."""
    symbols = np.asarray(symbols, dtype=np.uint8)
    starts = np.concatenate([[0], np.flatnonzero(symbols[1:] != symbols[:-1]) + 1]) if symbols.size else np.zeros(0, dtype=np.int64)
    lens = np.diff(np.concatenate([starts, [symbols.size]]))
    return symbols[starts].astype(np.uint64), lens.astype(np.uint64)


CANONICAL = {"dense_with_giants": dense_with_giants, "giants_with_dense": giants_with_dense, "mid_mixed": mid_mixed,
             "edges_8192": lambda: edges(8192), "edges_16384": lambda: edges(16384), "edges_32768": lambda: edges(32768),
             "fill_thresholds": fill_thresholds}
CANONICAL.update({"tail_" + name: (lambda name=name: tail(name)) for name in TAILS})

# the kernel the upload picks by the average density, (window, FILL, UNIFORM): proved by tests/test_transcode_inputs_host.py
DEFAULT_CLASS = {"dense_with_giants": (8192, False, False), "giants_with_dense": (32768, True, True), "mid_mixed": (16384, False, False),
                 "edges_8192": (32768, False, True), "edges_16384": (32768, True, True), "edges_32768": (32768, True, True),
                 "fill_thresholds": (32768, True, True), "tail_no_record_in_last_group": (8192, False, False),
                 "tail_two_blocks_in_last_group": (8192, False, False), "tail_three_blocks_in_last_group": (8192, False, False),
                 "tail_one_whole_group": (8192, False, False), "rewritten_dense": (16384, False, False), "rewritten_long": (32768, True, True),
                 "rewritten_reads": (8192, False, False)}
STREAMS = tuple(CANONICAL) + tuple(REWRITTEN) + ("rewritten_reads",)


class Stream:
    """One input: .f the oracle's FMI of the bytes an upload is given (.data, .sequences, .bases), .symbols; for a rewritten stream .canonical,
    the oracle's FMI of the same runs as Run::write writes them."""

    def __init__(self, orc, name):
        self.name = name
        self.canonical = None
        if name in CANONICAL:
            syms, lens = CANONICAL[name]()
            self.f = orc.FMI.from_runs(syms, lens)
        else:
            if name == "rewritten_reads":
                self.canonical = orc.FMI.from_text(read_set(orc, READS_A))
                syms, lens = runs_of(self.canonical.symbols)
                seed = READS_SEED
            else:
                recipe, seed = REWRITTEN[name]
                syms, lens = recipe()
                self.canonical = orc.FMI.from_runs(syms, lens)
            data = rewritten(syms, lens, seed)
            self.f = orc.FMI.from_native(data, self.canonical.sequences, self.canonical.bases)
        self.run_syms, self.run_lens = syms, lens
        self.data = self.f.data
        self.sequences, self.bases, self.nbytes, self.blocks = self.f.sequences, self.f.bases, self.f.nbytes, self.f.blocks
        self.symbols = self.f.symbols

    def block_starts(self):
        """Start position of every block and, last, the number of positions: from the oracle's samples."""
        return np.concatenate([[0], self.f.samples[0].astype(np.int64) + 1]) if self.blocks else np.zeros(1, dtype=np.int64)

    def group_positions(self):
        bs = self.block_starts()
        cuts = np.concatenate([bs[:-1][::GROUP], [bs[-1]]])
        return np.diff(cuts)

    def window_bases(self):
        """(S_g & ~127) of every group."""
        return self.block_starts()[:-1][::GROUP] & ~np.int64(REC_POS - 1)
