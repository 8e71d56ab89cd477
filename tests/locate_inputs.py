"""What the locate tests expect, from the reads alone (not a test module): the suffixes of a read collection in BWT order and the
occurrences of every short substring -- plain Python over the rows the test made, never the library's own find or extraction -- and
the two calls of bwtm_locate_ranges / the call of bwtm_locate_batch on prefilled outputs with spare slots behind the end."""
import numpy as np

SPARE = 16
FILL = 0xEEEEEEEEEEEEEEEE


def suffix_order(reads, lengths):
    """(ids, offsets) of BWT positions 0 .. n - 1: the suffixes of every read followed by its endmarker, sorted; the endmarker is below every
    symbol and the endmarker of read j below that of read j + 1, so a suffix that is a prefix of another comes first and equal suffixes come
    in the order of their reads.  Position p < m is the endmarker suffix of read p: (p, length of p)."""
    rows = [tuple(int(v) for v in reads[j, : int(lengths[j])]) for j in range(reads.shape[0])]
    keys = [(rows[j][o:], j, o) for j in range(len(rows)) for o in range(len(rows[j]) + 1)]
    keys.sort(key=lambda k: (k[0], k[1]))
    return np.array([k[1] for k in keys], dtype=np.uint64), np.array([k[2] for k in keys], dtype=np.uint64)


def all_suffixes(lengths):
    """The set {(j, o) : 0 <= o <= length of j}."""
    return {(j, o) for j in range(len(lengths)) for o in range(int(lengths[j]) + 1)}


def substring_table(reads, lengths, longest):
    """tuple of symbols -> sorted list of (read, offset), for every substring of 1 .. longest symbols of every read followed by its
    endmarker 0 (a 0 can only be a pattern's last symbol)."""
    table = {}
    for j in range(reads.shape[0]):
        row = tuple(int(v) for v in reads[j, : int(lengths[j])]) + (0,)
        for o in range(len(row)):
            for k in range(1, min(longest, len(row) - o) + 1):
                table.setdefault(row[o: o + k], []).append((j, o))
    return table


def naive_hits(table, lengths, pattern):
    """Sorted (read, offset) occurrences of a pattern; the empty pattern occurs at every suffix."""
    if len(pattern) == 0:
        return sorted(all_suffixes(lengths))
    return sorted(table.get(tuple(int(v) for v in pattern), []))


def pairs(ids, offs):
    return list(zip((int(v) for v in ids), (int(v) for v in offs)))


def locate_raw(gpu, loc, positions):
    """bwtm_locate_batch on outputs prefilled with 0xEE.. and SPARE slots longer than needed: the spare slots must keep the fill."""
    p_u64 = gpu.capi.p_u64
    positions = np.ascontiguousarray(positions, dtype=np.uint64)
    ids = np.full(positions.size + SPARE, FILL, dtype=np.uint64)
    offs = np.full(positions.size + SPARE, FILL, dtype=np.uint64)
    gpu.capi.check(gpu.capi.lib().bwtm_locate_batch(loc.h, positions.ctypes.data_as(p_u64), positions.size, ids.ctypes.data_as(p_u64), offs.ctypes.data_as(p_u64)))
    assert np.all(ids[positions.size:] == FILL) and np.all(offs[positions.size:] == FILL), "slots behind the last position were written"
    return ids[: positions.size], offs[: positions.size]


def ranges_raw(gpu, loc, sp, ep, max_hits=0):
    """The sizing call and the locating call of bwtm_locate_ranges, outputs prefilled with 0xEE.. and SPARE slots longer than needed."""
    p_u64, lib = gpu.capi.p_u64, gpu.capi.lib()
    sp = np.ascontiguousarray(sp, dtype=np.uint64)
    ep = np.ascontiguousarray(ep, dtype=np.uint64)
    hit_offsets = np.full(sp.size + 1, FILL, dtype=np.uint64)
    gpu.capi.check(lib.bwtm_locate_ranges(loc.h, sp.ctypes.data_as(p_u64), ep.ctypes.data_as(p_u64), sp.size, max_hits, hit_offsets.ctypes.data_as(p_u64), None, None, 0))
    sized = hit_offsets.copy()
    total = int(hit_offsets[-1])
    ids = np.full(total + SPARE, FILL, dtype=np.uint64)
    offs = np.full(total + SPARE, FILL, dtype=np.uint64)
    hit_offsets[:] = FILL
    gpu.capi.check(lib.bwtm_locate_ranges(loc.h, sp.ctypes.data_as(p_u64), ep.ctypes.data_as(p_u64), sp.size, max_hits, hit_offsets.ctypes.data_as(p_u64),
                                          ids.ctypes.data_as(p_u64), offs.ctypes.data_as(p_u64), ids.size))
    assert np.array_equal(hit_offsets, sized), "the sizing call and the locating call disagree about the hit offsets"
    assert np.all(ids[total:] == FILL) and np.all(offs[total:] == FILL), "slots behind hit_offsets[count] were written"
    return hit_offsets, ids[:total], offs[:total]
