"""Inputs whose SIZE lands exactly on a unit of the device structure, shared by tests/test_boundary_inputs_host.py (every recipe has exactly
the size it is named after: conditions on the oracle's results alone) and tests/test_gpu_exact_sizes.py (every builder of records and super
table, every form of the merge and the consumers on these inputs).  Not a test module.  Texts are the oracle's: symbols 1..5, each sequence
followed by a 0 ("$"); everything comes from oracle.generate_reads, oracle.FMI.*, tests/test_gpu_parity.run_symbols and seeded numpy
generators, so the inputs are deterministic.

The units: 32 positions (a plane word), 64 bytes (a native block), 128 positions (a record: num_records(n) = (n >> 7) + 1, so a multiple of
128 leaves a last record without a position), 3968 bytes (a transcode group of 62 blocks), 8192 positions (a bitvector chunk, 64 records),
65 536 positions (an encoder segment and emit tile, 512 records), 2^25 positions (a super row: num_supers(n) = (n >> 25) + 1), and for the
ingest sort 4096 suffixes (a tile) and 256 (a grid block of k_ingest_init).

alternating(n)    symbols 0, 1, .., 5, 0, .. : every run is one position and one byte, so the native stream has exactly n bytes.  3968 is at
                  once 31 records and one group, 7936 is 62 records and two groups.
run_stream(n)     run_symbols of mixed run lengths (long runs, few bytes) cut to n; pure(65 536): one run that fills a segment.
super_stream(n)   run lengths 1 .. 1500 cut to 2^25 - 1, 2^25, 2^25 + 1 and 2^26.
read_pair(name)   reads of 31 bases (32 positions each) split about 60 / 40, plus one read of 30 or 32 bases in b where +-1 is wanted: n_out
                  8191 .. 131 072; "a_65536" and "b_65536": one input alone ends on a segment boundary.
chain             a (25 165 824 positions) + b (8 388 096) = 2^25 - 512; tails of 511, 512 and 513 positions bring the merge to 2^25 - 1,
                  2^25 and 2^25 + 1.
INGEST_SHAPES     suffix totals (the sum of length + 1) of exactly 256, 512, 4095, 4096, 4097, 8192 and 12 288."""
import numpy as np

SMALL_SIZES = (63, 64, 65, 127, 128, 129, 3967, 3968, 3969, 7936, 8191, 8192, 8193, 65535, 65536, 65537)
SUPER = 1 << 25
SUPER_SIZES = (SUPER - 1, SUPER, SUPER + 1, 1 << 26)
GROUP_BYTES = 62 * 64
READ_BASES = 31                                                            # 32 positions with the endmarker

# (kind, n) of every small single stream
SMALL_STREAMS = [("alternating", n) for n in SMALL_SIZES] + [("runs", n) for n in SMALL_SIZES] + [("pure", 65536)]


def alternating(n):
    return (np.arange(n) % 6).astype(np.uint8)


def run_stream(n):
    """Mixed run lengths cut to n positions: short mixes for the sizes below a group, runs of up to 5000 above."""
    from test_gpu_parity import run_symbols
    lengths = [1, 2, 3, 7, 20, 41, 42] if n < 3000 else [1, 2, 3, 41, 42, 43, 170, 5000]
    sym = run_symbols(np.random.default_rng(7000 + n), max(64, n // 16), lengths)
    assert sym.size >= n
    return sym[:n].copy()


def pure(n):
    return np.full(n, 3, dtype=np.uint8)


def small_stream(kind, n):
    return {"alternating": alternating, "runs": run_stream, "pure": pure}[kind](n)


_super_symbols = []


def super_stream(n):
    """The run lengths of test_rank_structure_across_super_blocks, enough runs for 2^26 positions, cut to n (a view: read only)."""
    from test_gpu_parity import run_symbols
    if not _super_symbols:
        _super_symbols.append(run_symbols(np.random.default_rng(2), 420000, [1, 2, 3, 50, 400, 1500]))
    assert _super_symbols[0].size >= n
    return _super_symbols[0][:n]


# ------------------------------------------------------------------------------------------------------------------------------------
# Read pairs with an exact n_out

# name -> (reads of 31 bases in a, reads of 31 bases in b, bases of one more read in b or None): positions = 32 * reads (+ extra + 1)
READ_PAIRS = {
    "8191": (153, 102, 30), "8192": (154, 102, None), "8193": (154, 101, 32),
    "65535": (1228, 819, 30), "65536": (1229, 819, None), "65537": (1229, 818, 32),
    "131072": (2458, 1638, None),
    "a_65536": (2048, 1365, None),                                         # a alone ends on a segment (and chunk) boundary: a_off clamps there
    "b_65536": (1365, 2048, None),                                         # b alone does
}
N_OUT = {"8191": 8191, "8192": 8192, "8193": 8193, "65535": 65535, "65536": 65536, "65537": 65537, "131072": 131072,
         "a_65536": 65536 + 32 * 1365, "b_65536": 65536 + 32 * 1365}


def rows_of(oracle, seed, nreads, bases, width=READ_BASES + 1):
    """(rows, lengths): nreads generated reads of `bases` bases in rows of `width` symbols, zero behind each read's end."""
    rows = np.zeros((nreads, width), dtype=np.uint8)
    rows[:, :bases] = oracle.generate_reads(seed, nreads, bases).reshape(nreads, bases + 1)[:, :bases]
    return rows, np.full(nreads, bases, dtype=np.uint32)


def text_of(rows, lengths):
    """Rows -> the oracle's text: every read followed by an endmarker."""
    parts = []
    for k in range(rows.shape[0]):
        parts.append(rows[k, : int(lengths[k])]); parts.append(np.zeros(1, dtype=np.uint8))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def read_pair(oracle, name):
    """-> ((rows_a, lengths_a), (rows_b, lengths_b)): the reads of the pair `name`, rows of 32 symbols."""
    na, nb, extra = READ_PAIRS[name]
    seed = 8000 + 10 * sorted(READ_PAIRS).index(name)
    a = rows_of(oracle, seed, na, READ_BASES)
    b = rows_of(oracle, seed + 1, nb, READ_BASES)
    if extra is not None:
        x = rows_of(oracle, seed + 2, 1, extra)
        b = (np.concatenate([b[0], x[0]]), np.concatenate([b[1], x[1]]))
    return a, b


# ------------------------------------------------------------------------------------------------------------------------------------
# The 2^25 chain

CHAIN_A = (501, 32, 15, 49152)                                             # 25 165 824 positions, 1 572 864 sequences
CHAIN_B = (502, 32, 15, 16383)                                             # 8 388 096 positions, 524 256 sequences
CHAIN_BASE = SUPER - 512
# tail name -> (reads of 31 bases, bases of the further reads): 511 = 15 x 32 + 31; 512 = 15 x 32 + 31 + 1; 513 = 16 x 32 + 1
CHAIN_TAILS = {"511": (15, (30,)), "512": (15, (30, 0)), "513": (16, (0,))}


def chain_base(oracle):
    from second_half_inputs import repeated_collection
    return repeated_collection(oracle, *CHAIN_A), repeated_collection(oracle, *CHAIN_B)


def chain_tail(oracle, name):
    """-> (rows, lengths) of the tail collection `name`."""
    n31, more = CHAIN_TAILS[name]
    rows, lengths = rows_of(oracle, 503, n31, READ_BASES)
    for k, bases in enumerate(more):
        x = rows_of(oracle, 504 + k, 1, bases)
        rows, lengths = np.concatenate([rows, x[0]]), np.concatenate([lengths, x[1]])
    return rows, lengths


# ------------------------------------------------------------------------------------------------------------------------------------
# Ingest shapes

def ragged_to(oracle, seed, nreads, width, total):
    """nreads reads of random lengths 0 .. width whose suffix total (the sum of length + 1) is exactly `total`."""
    rng = np.random.default_rng(seed)
    rows, _ = rows_of(oracle, seed, nreads, width, width)
    lengths = rng.integers(0, width + 1, nreads).astype(np.int64)
    k = 0
    while int(lengths.sum()) + nreads != total:                           # move single bases until the total fits
        step = 1 if int(lengths.sum()) + nreads < total else -1
        if 0 <= lengths[k % nreads] + step <= width:
            lengths[k % nreads] += step
        k += 1
    lengths = lengths.astype(np.uint32)
    for j in range(nreads):
        rows[j, lengths[j]:] = 0
    return rows, lengths


def ingest_shape(oracle, name):
    """-> (rows, lengths or None, suffix total)."""
    uniform = {"8x31": (8, 31), "4x63": (4, 63), "16x31": (16, 31), "128x31": (128, 31), "64x63": (64, 63), "256x31": (256, 31), "384x31": (384, 31),
               "192x63": (192, 63)}
    if name in uniform:
        n, w = uniform[name]
        return rows_of(oracle, 8500 + n + w, n, w, w)[0], None, n * (w + 1)
    if name == "4095":                                                      # 127 reads of 31 bases and one of 30
        rows, lengths = rows_of(oracle, 8601, 128, 31, 31)
        lengths[77] = 30; rows[77, 30:] = 0
        return rows, lengths, 4095
    if name == "4097":                                                      # 128 reads of 31 bases and one empty read
        rows, lengths = rows_of(oracle, 8602, 129, 31, 31)
        lengths[128] = 0; rows[128] = 0
        return rows, lengths, 4097
    if name == "ragged_4096":
        rows, lengths = ragged_to(oracle, 8603, 150, 50, 4096)
        return rows, lengths, 4096
    raise ValueError(name)


# name -> the suffix total the shape is named after
INGEST_SHAPES = {"8x31": 256, "4x63": 256, "16x31": 512, "4095": 4095, "128x31": 4096, "64x63": 4096, "ragged_4096": 4096, "4097": 4097,
                 "256x31": 8192, "384x31": 12288, "192x63": 12288}


# ------------------------------------------------------------------------------------------------------------------------------------
# Expected sequences and locations of an index too large for the naive tables, from the oracle's LF / select alone

def sequence_by_walk(m, j):
    """Sequence j of the oracle FMI m: the LF walk from position j (the endmarker suffix of sequence j) back to the sequence's start."""
    out, p = [], int(j)
    while True:
        p, c = m.LF(p)
        if c == 0:
            return np.array(out[::-1], dtype=np.uint8)
        out.append(c)


def locate_by_walk(m, p, C=None):
    """(sequence id, offset) of position p of the oracle FMI m: the offset is the number of LF steps to the sequence's start, the id is
    where the forward walk (the suffix's first symbol c by C, then select of the (p - C[c] + 1)-th c) reaches an endmarker suffix."""
    C = m.C if C is None else C
    q, offset = int(p), 0
    while True:
        nxt, c = m.LF(q)
        if c == 0:
            break
        q, offset = nxt, offset + 1
    q, sequences = int(p), m.sequences
    while q >= sequences:
        c = int(np.searchsorted(C, q, side="right")) - 1
        q = m.select(q - int(C[c]) + 1, c)
    return q, offset
