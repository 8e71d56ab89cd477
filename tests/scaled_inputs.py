"""How every query result changes when each read of a collection is held c times in a row (not a test module; pure numpy, never the library).

R is a small collection given as rows; R x c holds read 0 c times, then read 1 c times, and so on: copy t of read j has id c j + t.  Equal
suffixes are ordered by sequence index, so the BWT of R x c is the BWT of R with every symbol repeated c times, and position p' of R x c
is (p, t) = (p' // c, p' % c) with p a position of R.  Every function below states one rule: it takes what a brute force of tests/*_inputs.py
gives on R and returns what the same brute force gives on R x c.  tests/test_scaled_inputs_host.py pins every rule against the brute force
on the explicitly expanded rows; tests/test_gpu_beyond_32_bits.py uses the rules with a c that puts n' = c n beyond 2^25 and beyond 2^32,
where the expanded rows themselves could not be held."""
import numpy as np

import kmer_inputs
import kmer_join_inputs

U64 = np.uint64
EMPTY = (1, 0)                          # the canonical empty range


def small_collection(m, seed, n_at=((3, 4), (5, 20), (13, 0), (37, 11), (46, 16), (47, 39))):
    """(reads, lengths, clean): overlap_inputs.overlap_reads(m, seed) -- ragged lengths 0 .. 40, empty reads, exact duplicates, a tandem
    repeat and a homopolymer -- with the symbols at n_at (row, column) set to 5, so that skip matters, and the reads before that (the
    patterns of mem_inputs.special_patterns are made from reads of symbols 1..4)."""
    from overlap_inputs import overlap_reads
    clean, lengths = overlap_reads(m, seed)
    reads = clean.copy()
    for j, o in n_at:
        assert o < int(lengths[j])
        reads[j, o] = 5
    return reads, lengths, clean


def expand(rows, c):
    """The rows of R x c, explicitly: row j c times in a row."""
    return [rows[j] for j in range(len(rows)) for _ in range(int(c))]


def expand_reads(reads, lengths, c):
    """(reads, lengths) of R x c for a padded matrix of rows (tests/overlap_inputs.py, tests/locate_inputs.py)."""
    return np.repeat(reads, int(c), axis=0), np.repeat(lengths, int(c))


def split(position, c):
    """p' -> (p, t)."""
    return int(position) // int(c), int(position) % int(c)


def scaled(values, c):
    """An array of positions, counts or prefix sums of R, multiplied by c, as uint64 (n' may lie beyond 2^32: no 32-bit product anywhere)."""
    return np.asarray(values, dtype=U64) * U64(int(c))


# ---------------------------------------------------------------------------------------------------------------------------- rank, find

def rank(bwt, position, symbol, c):
    """rank'(p', s) = c rank(p, s) + (t if BWT[p] == s else 0); bwt = the BWT of R as an array of symbols, p' in [0, n']."""
    p, t = split(position, c)
    below = int(np.count_nonzero(bwt[:p] == symbol))
    return int(c) * below + (t if p < len(bwt) and int(bwt[p]) == int(symbol) else 0)


def find_range(sp, ep, c):
    """[sp, ep] -> [c sp, c ep + c - 1]; an empty range (sp > ep) stays empty.  The empty pattern's [0, n - 1] becomes [0, n' - 1] by the same rule."""
    sp, ep, c = int(sp), int(ep), int(c)
    return (c * sp, c * ep + c - 1) if sp <= ep else EMPTY


# ---------------------------------------------------------------------------------------------------------------------------- hits

def approx_hits(want, c):
    """approx_inputs.expected's (hit_offsets, sp, count, mismatches): hit_offsets, the order and the mismatches stay, sp and count are
    multiplied.  The empty pattern's hit (0, n, 0) becomes (0, n', 0) by the same rule."""
    hit_offsets, sp, count, mismatches = want
    return hit_offsets.copy(), scaled(sp, c), scaled(count, c), mismatches.copy()


def edit_hits(want, c):
    """edit_inputs.expected's (hit_offsets, sp, count, edits, lengths), likewise."""
    hit_offsets, sp, count, edits, lengths = want
    return hit_offsets.copy(), scaled(sp, c), scaled(count, c), edits.copy(), lengths.copy()


def stats(want, c):
    """mem_inputs.expected_stats's (lengths, sp, count): the lengths stay, sp and count are multiplied ((0, 0, 0) stays)."""
    lengths, sp, count = want
    return lengths.copy(), scaled(sp, c), scaled(count, c)


def mems(want, c):
    """mem_inputs.expected_mems's (hit_offsets, begin, length, sp, count): hit_offsets, begins and lengths stay, sp and count are multiplied."""
    hit_offsets, begin, length, sp, count = want
    return hit_offsets.copy(), begin.copy(), length.copy(), scaled(sp, c), scaled(count, c)


# ---------------------------------------------------------------------------------------------------------------------------- locate

def locate(ids, offs, positions, c):
    """p' -> (c id(p) + t, offset(p)); (ids, offs) = locate_inputs.suffix_order of R, positions = an array of p'."""
    positions = np.asarray(positions, dtype=U64)
    p = (positions // U64(int(c))).astype(np.int64)
    t = positions % U64(int(c))
    return np.asarray(ids, dtype=U64)[p] * U64(int(c)) + t, np.asarray(offs, dtype=U64)[p]


def locate_ranges(ids, offs, sp, ep, c, max_hits=0):
    """(hit_offsets, ids, offsets) of closed ranges [sp', ep'] of R x c (sp' > ep': empty): a range's hits come in ascending p', its first
    max_hits when max_hits > 0."""
    kept = []
    for s, e in zip((int(v) for v in sp), (int(v) for v in ep)):
        size = max(e - s + 1, 0)
        kept.append(min(size, int(max_hits)) if max_hits > 0 else size)
    hit_offsets = np.zeros(len(kept) + 1, dtype=U64)
    hit_offsets[1:] = np.cumsum(np.array(kept, dtype=U64), dtype=U64)
    positions = np.concatenate([np.arange(int(s), int(s) + k, dtype=U64) for s, k in zip(sp, kept)] + [np.zeros(0, dtype=U64)])
    return (hit_offsets,) + locate(ids, offs, positions, c)


def range_sizes(sp, ep, max_hits=0):
    """hit_offsets of locate_ranges alone, in Python integers: the sizing call's answer, whose last entry may lie beyond 2^32."""
    out = [0]
    for s, e in zip((int(v) for v in sp), (int(v) for v in ep)):
        size = max(e - s + 1, 0)
        out.append(out[-1] + (min(size, int(max_hits)) if max_hits > 0 else size))
    return np.array(out, dtype=U64)


# ---------------------------------------------------------------------------------------------------------------------------- sequences

def sequence_row(seq_id, c):
    """Sequence i' of R x c is row i' // c of R."""
    return int(seq_id) // int(c)


# ---------------------------------------------------------------------------------------------------------------------------- overlaps

def overlap_offsets(want, c, max_hits=0):
    """hit_offsets of overlap_inputs.expected(..., max_hits=0) on R -> those on R x c: multiplied by c without max_hits, min(h, c hits)
    per query with max_hits = h."""
    per_query = scaled(np.diff(want[0].astype(np.int64)), c)
    if max_hits > 0:
        per_query = np.minimum(per_query, U64(int(max_hits)))
    hit_offsets = np.zeros(per_query.size + 1, dtype=U64)
    hit_offsets[1:] = np.cumsum(per_query, dtype=U64)
    return hit_offsets


def overlaps(want, c, max_hits=0):
    """overlap_inputs.expected(..., max_hits=0) on R, (hit_offsets, ids, lengths) -> the same on R x c with max_hits: if a query's hits on R
    are (t_0, l_0), (t_1, l_1), ..., its hit number r on R x c is (c t_{r // c} + r % c, l_{r // c}).  (Without max_hits the result holds c
    times the hits of R: only for a small c.)"""
    hit_offsets = overlap_offsets(want, c, max_hits)
    ids, lens = [], []
    for q in range(hit_offsets.size - 1):
        r = np.arange(int(hit_offsets[q + 1] - hit_offsets[q]), dtype=np.int64)
        at = int(want[0][q]) + r // int(c)
        ids.append(want[1][at].astype(U64) * U64(int(c)) + (r % int(c)).astype(U64))
        lens.append(want[2][at].astype(U64))
    return hit_offsets, np.concatenate(ids + [np.zeros(0, dtype=U64)]), np.concatenate(lens + [np.zeros(0, dtype=U64)])


def overlap_queries(rows, seq_ids, c):
    """The queries of an overlap call by id: sequence i' uses row i' // c.  (A hit (q, L) of R stands for all c copies of q: overlaps().)"""
    return [tuple(int(v) for v in rows[sequence_row(i, c)]) for i in seq_ids]


# ---------------------------------------------------------------------------------------------------------------------------- k-mers

def kmers(want, c, min_count=1):
    """kmer_inputs.brute(R, k, skip, 1)'s (codes, counts, sp) -> that of R x c at a min_count stated on the scaled counts: codes stay,
    counts and sp are multiplied, and what stays below min_count leaves."""
    codes, counts, sp = want
    counts = scaled(counts, c)
    keep = counts >= U64(max(int(min_count), 1))
    return codes[keep], counts[keep], scaled(sp, c)[keep]


def kmer_levels(rows, k, skip, c, min_count=1, brute=kmer_inputs.brute):
    """nodes[t] = the (t + 1)-mers of R x c with count >= min_count, every level.  brute: kmer_inputs.brute, or a caller's function of the
    same arguments that remembers its results."""
    return np.array([kmers(brute(rows, t + 1, skip, 1), c, min_count)[0].size for t in range(k)], dtype=U64)


def kmer_total(want, c):
    """bwtm_kmers_total: the sum of the kept counts."""
    return int(c) * int(np.asarray(want[1], dtype=U64).sum(dtype=U64))


def histogram(hist, c, bins):
    """The unfolded histogram of R's kept counts (hist[j] = k-mers of count j, long enough to hold every count) -> the histogram of
    R x c folded at `bins`: hist'[c j] = hist[j] while c j lies below the folding bin bins - 1, everything else is folded into it."""
    out = np.zeros(bins, dtype=U64)
    for j, v in enumerate(int(v) for v in hist):
        if v:
            out[min(int(c) * j, bins - 1)] += U64(v)
    return out


# ---------------------------------------------------------------------------------------------------------------------------- k-mer join

def join(want, ca, cb, min_a=0, max_a=None, min_b=0, max_b=None, min_sum=1):
    """kmer_join_inputs.brute_pair(A, B, k, skip) without bounds, (codes, cnt_a, cnt_b, sp_a, sp_b) -> that of (A x ca, B x cb) with
    the bounds stated on the scaled counts: cnt_a ca, cnt_b cb, sp_a ca and sp_b cb, insertion points included."""
    codes, cnt_a, cnt_b, sp_a, sp_b = want
    cnt_a, cnt_b = scaled(cnt_a, ca), scaled(cnt_b, cb)
    none = kmer_join_inputs.NO_BOUND
    keep = (cnt_a >= U64(int(min_a))) & (cnt_b >= U64(int(min_b))) & (cnt_a + cnt_b >= U64(max(int(min_sum), 1)))
    keep &= (cnt_a <= U64(none if max_a is None else int(max_a))) & (cnt_b <= U64(none if max_b is None else int(max_b)))
    return codes[keep], cnt_a[keep], cnt_b[keep], scaled(sp_a, ca)[keep], scaled(sp_b, cb)[keep]


def join_levels(rows_a, rows_b, k, skip, ca, cb, min_a=0, max_a=None, min_b=0, max_b=None, min_sum=1, brute_pair=kmer_join_inputs.brute_pair):
    """nodes[t] for t < k - 1 = the (t + 1)-mers the lower bounds keep; nodes[k - 1] = the k-mers all bounds keep (kmer_join_inputs.brute_pair_levels).
    brute_pair: kmer_join_inputs.brute_pair, or a caller's function of the same arguments that remembers its results."""
    inner = [join(brute_pair(rows_a, rows_b, t + 1, skip), ca, cb, min_a, None, min_b, None, min_sum)[0].size for t in range(k - 1)]
    return np.array(inner + [join(brute_pair(rows_a, rows_b, k, skip), ca, cb, min_a, max_a, min_b, max_b, min_sum)[0].size], dtype=U64)


def join_summary(scaled_want):
    """The seven numbers of bwtm_kmer_join_summary: kmer_join_inputs.classes on the scaled result, so every side is scaled by its own c."""
    return kmer_join_inputs.classes(scaled_want)


# ---------------------------------------------------------------------------------------------------------------------------- corrector, unitigs

def small_threshold(threshold, c):
    """A threshold on the counts of R x c -> the threshold on R with the same solid set: c count >= T iff count >= ceil(T / c).  So c t,
    c t - 1 (for c > 1) and c (t - 1) + 1 all give t: the last two are the edges of the thresholds that do."""
    return -(-max(int(threshold), 1) // int(c))


def unitig_arrays(arrays, c):
    """unitig_inputs.Graph(R's table, k, t).arrays() -> those of the graph over the k-mers of R x c at a threshold T with
    small_threshold(T, c) == t: the same graph with every occurrences value multiplied by c."""
    offsets, text, nodes, occurrences, flags, links = arrays
    return offsets.copy(), text.copy(), nodes.copy(), scaled(occurrences, c), flags.copy(), links.copy()
