"""What the walk tests expect (not a test module): a collection with sequences around the default bound of 2^16 symbols, its suffix array
by prefix doubling, suffix-prefix overlaps by the prefix function -- and streams that are the BWT of nothing, with a plain numpy model of
what LF walks and the backward search do on them.  Expected values come from the rows the test made or from these models, never from
the library.  tests/test_walk_inputs_host.py pins every recipe, against the oracle where one exists."""
import numpy as np

LONG_LENGTHS = (0, 65535, 3, 65536, 1, 65537, 129, 128, 127, 40)
PLANT_35 = 4000                 # the last 4000 symbols of sequence 3 are the first 4000 of sequence 5
PLANT_16 = 129                  # the last 129 symbols of sequence 1 are sequence 6
LONG_SEED = 1

# The scrambled streams in use, (seed, n, m) -> what lf_model says about them (printed when they were chosen, asserted in
# tests/test_walk_inputs_host.py): the longest walk and the id that takes it, the number of positions on cycles and the smallest of them.
SCRAMBLED = {
    "small": dict(seed=1, n=6000, m=100, longest=376, longest_id=90, cycle=44, first_cycle=310),
    "large": dict(seed=2, n=20000, m=300, longest=340, longest_id=73, cycle=155, first_cycle=504),
}


def long_collection(seed):
    """(rows, text): ten iid sequences over 1..5 of LONG_LENGTHS symbols, in this id order, with the two planted suffix-prefix overlaps;
    text is the oracle's input, every row followed by an endmarker 0.  197 046 positions."""
    rng = np.random.default_rng(seed)
    rows = [rng.integers(1, 6, size=length).astype(np.uint8) for length in LONG_LENGTHS]
    rows[3][LONG_LENGTHS[3] - PLANT_35:] = rows[5][:PLANT_35]
    rows[1][LONG_LENGTHS[1] - PLANT_16:] = rows[6]
    return rows, text_of_rows(rows)


def text_of_rows(rows):
    parts = []
    for row in rows:
        parts.append(np.asarray(row, dtype=np.uint8)); parts.append(np.zeros(1, dtype=np.uint8))
    return np.concatenate(parts)


def expected_text(rows, ids):
    """(offsets, text) of the rows with the given ids, as bwtm_sequences_extract returns them."""
    offsets = np.zeros(len(ids) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(rows[int(j)]) for j in ids])
    return offsets, np.concatenate([np.asarray(rows[int(j)], dtype=np.uint8) for j in ids] + [np.zeros(0, dtype=np.uint8)])


def suffix_array(text):
    """(sa, ids, offsets, bwt) of a text of rows that each end in 0.  sa[p] = the text position of the p-th smallest suffix, by prefix
    doubling; the endmarker of read j has the key j and a symbol c the key m - 1 + c, so every endmarker is distinct and below every symbol,
    two suffixes differ at the first endmarker of either at the latest, and the order is the one locate_inputs.suffix_order states.
    (ids[p], offsets[p]) is the read and the offset of that suffix, bwt[p] the symbol before it (0 before a read's first symbol)."""
    text = np.asarray(text, dtype=np.uint8)
    n = text.size
    ends = np.nonzero(text == 0)[0]
    m = ends.size
    assert n > 0 and text[-1] == 0
    rank = text.astype(np.int64) + (m - 1)
    rank[ends] = np.arange(m)
    k = 1
    while True:
        second = np.full(n, -1, dtype=np.int64)
        second[: n - k] = rank[k:]
        sa = np.lexsort((second, rank))
        differs = (rank[sa][1:] != rank[sa][:-1]) | (second[sa][1:] != second[sa][:-1])
        new = np.zeros(n, dtype=np.int64)
        new[sa[1:]] = np.cumsum(differs)
        rank = new
        if int(rank.max()) == n - 1:
            break
        k *= 2
        assert k < 2 * n
    sa = np.argsort(rank, kind="stable")
    starts = np.concatenate([[0], ends[:-1] + 1])
    ids = np.searchsorted(ends, sa, side="left")                           # the first endmarker at or behind the suffix is its read's
    offsets = sa - starts[ids]
    bwt = np.where(offsets > 0, text[sa - 1], 0).astype(np.uint8)
    return sa, ids.astype(np.uint64), offsets.astype(np.uint64), bwt


def borders(target, query):
    """The overlap lengths l >= 1 with target[:l] == query[-l:], longest first: the borders of target + (6,) + query, by its prefix function
    (6 is no symbol, so no border is longer than either part)."""
    s = [int(v) for v in target] + [6] + [int(v) for v in query]
    pi = [0] * len(s)
    k = 0
    for i in range(1, len(s)):
        c = s[i]
        while k > 0 and s[k] != c:
            k = pi[k - 1]
        if s[k] == c:
            k += 1
        pi[i] = k
    out = []
    k = pi[-1] if len(query) > 0 else 0
    while k > 0:
        out.append(k)
        k = pi[k - 1]
    return out


def border_hits(rows, query, tau):
    """The hits (t, l) of one query against every row in the order of the contract: longest first, then the targets ascending as strings
    (a prefix before its extensions), equal ones by id -- overlap_inputs.all_pairs_hits for rows too long to compare at every length."""
    keys = [np.asarray(r, dtype=np.uint8).tobytes() for r in rows]          # bytes compare as strings do, a prefix first
    found = [(l, keys[t], t) for t in range(len(rows)) for l in borders(rows[t], query) if l >= max(tau, 1)]
    found.sort(key=lambda h: (-h[0], h[1], h[2]))
    return [(t, l) for l, _, t in found]


def hits_arrays(per_query, max_hits=0):
    """(hit_offsets, ids, lengths) of a list of hit lists, each cut to its first max_hits when max_hits > 0."""
    hit_offsets, ids, lens = [0], [], []
    for hits in per_query:
        if max_hits > 0:
            hits = hits[:max_hits]
        ids.extend(t for t, _ in hits); lens.extend(l for _, l in hits)
        hit_offsets.append(len(ids))
    return np.array(hit_offsets, dtype=np.uint64), np.array(ids, dtype=np.uint64), np.array(lens, dtype=np.uint64)


def scrambled_stream(seed, n, m):
    """n symbols, iid 1..5, with m zeros at positions drawn without replacement: a stream with consistent counts that is no BWT."""
    rng = np.random.default_rng(seed)
    symbols = rng.integers(1, 6, size=n).astype(np.uint8)
    symbols[rng.choice(n, size=m, replace=False)] = 0
    return symbols


class LFModel:
    """What lf_model returns.  n, m, C (7 entries), rank (6 x (n + 1) cumulative counts), lf (LF of every position that holds 1..5, -1 at a
    zero); per walk j < m: lengths[j] steps, sequences[j] (its symbols reversed), ends[j] (the position of the zero it meets), ks[j] =
    rank(ends[j], 0); table[k] = j; per position ids / offs (-1 on a cycle), cycle = the positions on pure cycles, ascending;
    visited_max / table_max = the largest position loaded and the largest table index used by any walk."""

    def fails(self, ids, max_len):
        """The index in `ids` that the kernels name: the first walk that meets a symbol other than 0 after max_len steps (exactly max_len
        symbols pass), or None."""
        for k, j in enumerate(ids):
            if self.lengths[int(j)] > max_len:
                return k
        return None

    def pair(self, p):
        return (int(self.ids[p]), int(self.offs[p])) if self.ids[p] >= 0 else None


def lf_model(symbols):
    """Plain LF over any symbols 0..5 whose counts are taken from the stream itself.  LF maps the positions that hold c >= 1 one to one into
    [C[c], C[c + 1]), all of it at or beyond C[1] = m: positions 0 .. m - 1 have no predecessor, so the walk from each ends at a zero of its
    own, and every position that is on none of these m walks lies on a cycle without a zero."""
    symbols = np.asarray(symbols, dtype=np.uint8)
    n = symbols.size
    M = LFModel()
    M.n = n
    M.C = np.zeros(7, dtype=np.int64)
    M.C[1:] = np.cumsum(np.bincount(symbols, minlength=6))[:6]
    M.m = m = int(M.C[1])
    M.rank = np.zeros((6, n + 1), dtype=np.int64)
    for c in range(6):
        M.rank[c, 1:] = np.cumsum(symbols == c)
    at = np.arange(n)
    M.lf = np.where(symbols > 0, M.C[symbols] + M.rank[symbols, at], -1)
    lf, sym = M.lf.tolist(), symbols.tolist()
    M.lengths = np.zeros(m, dtype=np.int64); M.ends = np.zeros(m, dtype=np.int64); M.ks = np.zeros(m, dtype=np.int64)
    M.sequences = []
    M.table = np.full(m, -1, dtype=np.int64)
    M.ids = np.full(n, -1, dtype=np.int64); M.offs = np.full(n, -1, dtype=np.int64)
    M.visited_max = M.table_max = -1
    for j in range(m):
        path, p = [], j
        while sym[p] != 0:
            path.append(p); p = lf[p]
            assert len(path) <= n, "a walk from an endmarker suffix entered a cycle"
        path.append(p)
        d = len(path) - 1
        k = int(M.rank[0, p])
        M.lengths[j] = d; M.ends[j] = p; M.ks[j] = k
        M.sequences.append(symbols[path[:d]][::-1].copy())
        assert M.table[k] == -1, "two walks end at the same zero"
        M.table[k] = j
        assert np.all(M.ids[path] == -1), "two walks share a position"
        M.ids[path] = j
        M.offs[path] = d - np.arange(d + 1)
        M.visited_max = max(M.visited_max, max(path)); M.table_max = max(M.table_max, k)
    M.cycle = np.nonzero(M.ids < 0)[0]
    return M


def cycle_walk_stays_inside(M, p, steps):
    """The positions a walk of `steps` steps from the cycle position p loads are all cycle positions below n."""
    for _ in range(steps):
        if not (0 <= p < M.n and M.ids[p] < 0 and M.lf[p] >= 0):
            return False
        p = int(M.lf[p])
    return True


def overlap_model(symbols, table, query, tau, max_hits):
    """The backward search of kernels/overlap.hip.h in numpy, on any stream: after l symbols of the query, taken from its end, the range is
    [sp, e1); while it is not empty and l >= tau the hits of length l are table[z] for z in [rank(sp, 0), rank(e1, 0)).  The hits come longest
    first, within a length by ascending z, cut to the first max_hits when max_hits > 0.  Returns [(id, l), ...]."""
    symbols = np.asarray(symbols, dtype=np.uint8)
    n = symbols.size
    C = np.zeros(7, dtype=np.int64)
    C[1:] = np.cumsum(np.bincount(symbols, minlength=6))[:6]
    rank = np.zeros((6, n + 1), dtype=np.int64)
    for c in range(6):
        rank[c, 1:] = np.cumsum(symbols == c)
    found, sp, e1 = [], 0, n
    for l in range(1, len(query) + 1):
        c = int(query[len(query) - l])
        assert 1 <= c <= 5
        sp, e1 = int(C[c] + rank[c, sp]), int(C[c] + rank[c, e1])
        if sp >= e1:
            break
        assert e1 <= n
        z0, z1 = int(rank[0, sp]), int(rank[0, e1])
        if l >= max(tau, 1) and z1 > z0:
            assert z1 <= len(table)
            found.append([(int(table[z]), l) for z in range(z0, z1)])
    hits = [h for group in reversed(found) for h in group]
    return hits[:max_hits] if max_hits > 0 else hits
