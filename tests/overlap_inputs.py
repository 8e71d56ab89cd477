"""What the overlap tests expect, from the reads alone (not a test module): reads cut from one small genome, so that they do overlap, the
suffix-prefix overlaps of queries with them by plain string comparison of the rows -- never the library's own search or extraction --
and the two calls of bwtm_overlap_sequences / bwtm_overlap_batch on prefilled outputs with spare slots behind the end."""
import numpy as np

from locate_inputs import FILL, SPARE

WIDTH = 40
LENGTH_CYCLE = (0, 1, 5, 12, 17, 23, 33, 40)
GENOME = 600


def overlap_reads(m, seed):
    """m rows of WIDTH comp values (zero behind each read's end), windows of one genome of 600 symbols 1..4 in which positions 100..139 are
    the tandem repeat (1, 2) x 20 and positions 300..329 the homopolymer of 3: read k is the window of LENGTH_CYCLE[k % 8] symbols at a
    uniformly drawn start.  Rows 24..31 repeat rows 16..23 (exact duplicates: the cycle gives them the same lengths)."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(1, 5, size=GENOME).astype(np.uint8)
    genome[100:140] = np.tile(np.array([1, 2], dtype=np.uint8), 20)
    genome[300:330] = 3
    lengths = np.array([LENGTH_CYCLE[k % len(LENGTH_CYCLE)] for k in range(m)], dtype=np.uint32)
    reads = np.zeros((m, WIDTH), dtype=np.uint8)
    for k in range(m):
        start = int(rng.integers(0, GENOME - int(lengths[k]) + 1))
        reads[k, : lengths[k]] = genome[start: start + int(lengths[k])]
    if m >= 32:
        reads[24:32] = reads[16:24]
    return reads, lengths


def rows_of(reads, lengths):
    return [tuple(int(v) for v in reads[j, : int(lengths[j])]) for j in range(reads.shape[0])]


def all_pairs_hits(rows, query, tau):
    """The hits (t, l) of one query by comparing it with every row at every length, in the order of the contract: longest first, then the
    targets ascending as strings (a prefix before its extensions), equal ones by id."""
    L = len(query)
    found = [(l, rows[t], t) for t in range(len(rows)) for l in range(max(tau, 1), min(L, len(rows[t])) + 1) if rows[t][:l] == query[L - l:]]
    found.sort(key=lambda h: (-h[0], h[1], h[2]))
    return [(t, l) for l, _, t in found]


def prefix_table(rows):
    """tuple of symbols -> ids of the rows that start with it, ascending by (row, id): the all-pairs comparison, hashed."""
    order = sorted(range(len(rows)), key=lambda t: (rows[t], t))
    table = {}
    for t in order:
        for l in range(1, len(rows[t]) + 1):
            table.setdefault(rows[t][:l], []).append(t)
    return table


def table_hits(table, query, tau):
    """all_pairs_hits through prefix_table(rows)."""
    L = len(query)
    out = []
    for l in range(L, max(tau, 1) - 1, -1):
        out.extend((t, l) for t in table.get(tuple(query[L - l:]), ()))
    return out


def expected(table, queries, tau, max_hits=0):
    """(hit_offsets, ids, lengths) of a list of queries (tuples), each query's hits cut to its first max_hits when max_hits > 0."""
    hit_offsets, ids, lens = [0], [], []
    for q in queries:
        hits = table_hits(table, tuple(int(v) for v in q), tau)
        if max_hits > 0:
            hits = hits[:max_hits]
        ids.extend(t for t, _ in hits); lens.extend(l for _, l in hits)
        hit_offsets.append(len(ids))
    return np.array(hit_offsets, dtype=np.uint64), np.array(ids, dtype=np.uint64), np.array(lens, dtype=np.uint64)


def _two_calls(gpu, count, call):
    """The sizing call and the real call, outputs prefilled with 0xEE.. and SPARE slots longer than needed."""
    p_u64 = gpu.capi.p_u64
    hit_offsets = np.full(count + 1, FILL, dtype=np.uint64)
    gpu.capi.check(call(hit_offsets.ctypes.data_as(p_u64), None, None, 0))
    sized = hit_offsets.copy()
    total = int(hit_offsets[-1])
    ids = np.full(total + SPARE, FILL, dtype=np.uint64)
    lens = np.full(total + SPARE, FILL, dtype=np.uint64)
    hit_offsets[:] = FILL
    gpu.capi.check(call(hit_offsets.ctypes.data_as(p_u64), ids.ctypes.data_as(p_u64), lens.ctypes.data_as(p_u64), ids.size))
    assert np.array_equal(hit_offsets, sized), "the sizing call and the real call disagree about the hit offsets"
    assert np.all(ids[total:] == FILL) and np.all(lens[total:] == FILL), "slots behind hit_offsets[count] were written"
    return hit_offsets, ids[:total], lens[:total]


def sequences_raw(gpu, loc, tau, ids=None, first=0, count=None, max_hits=0):
    """bwtm_overlap_sequences, both calls."""
    lib, ip = gpu.capi.lib(), None
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        ip, count = ids.ctypes.data_as(gpu.capi.p_u64), ids.size
    return _two_calls(gpu, int(count), lambda ho, oi, ol, cap: lib.bwtm_overlap_sequences(loc.h, ip, int(first), int(count), int(tau), int(max_hits), ho, oi, ol, cap))


def patterns_raw(gpu, loc, tau, patterns, max_hits=0):
    """bwtm_overlap_batch, both calls."""
    lib = gpu.capi.lib()
    offsets = np.zeros(len(patterns) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(p) for p in patterns])
    text = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.uint8) for p in patterns] + [np.zeros(0, dtype=np.uint8)]))
    tp, op = text.ctypes.data_as(gpu.capi.p_u8), offsets.ctypes.data_as(gpu.capi.p_u64)
    return _two_calls(gpu, len(patterns), lambda ho, oi, ol, cap: lib.bwtm_overlap_batch(loc.h, tp, op, len(patterns), int(tau), int(max_hits), ho, oi, ol, cap))


def same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == len(want)
