"""What the unitig tests expect (not a test module): the compacted de Bruijn graph of a dict of k-mer codes, by the rule of include/bwtm.h
restated over Python sets -- never the library.  The codes and counts come from kmer_inputs.brute; tests/test_unitigs_host.py checks this
file on its own.  It also holds the hand-made collections (A C G T = comp values 1..4)."""
import functools

import numpy as np

from kmer_inputs import brute, genome_reads, iid_reads, kept_comps

NONE = (1 << 64) - 1
CIRCULAR = 1


def comps_of(s):
    """'ACGTN' -> comp values 1..5."""
    return np.array(["$ACGTN".index(c) for c in s], dtype=np.uint8)


def table_of(rows, k, skip=5, min_count=1):
    """{code: count} of the k-mers of the rows."""
    codes, counts, _ = brute(rows, k, skip, min_count)
    return dict(zip((int(c) for c in codes), (int(c) for c in counts)))


def successors(x, k):
    mask = (1 << (2 * k)) - 1
    return [((x << 2) | r) & mask for r in range(4)]


def predecessors(x, k):
    return [(r << (2 * (k - 1))) | (x >> 2) for r in range(4)]


class Graph:
    """nodes: the codes of count >= t, ascending.  unitigs: a list of (text uint8, nodes, occurrences, flags, links [4]) in the rule's order;
    where: {code: (unitig, offset)}; members[u]: the codes of unitig u in order."""

    def __init__(self, table, k, t, skip=5):
        t = max(int(t), 1)
        self.k, self.skip = k, skip
        self.nodes = sorted(c for c, n in table.items() if n >= t)
        solid = set(self.nodes)
        out = {x: [y for y in successors(x, k) if y in solid] for x in self.nodes}
        inn = {x: [y for y in predecessors(x, k) if y in solid] for x in self.nodes}
        self.out, self.inn = out, inn
        nxt, prv = {}, {}
        for x in self.nodes:
            if len(out[x]) == 1 and len(inn[out[x][0]]) == 1:
                nxt[x] = out[x][0]; prv[out[x][0]] = x
        paths, seen = [], set()
        for x in self.nodes:                                      # the paths, from their first nodes
            if x in prv:
                continue
            path = [x]
            while path[-1] in nxt:
                path.append(nxt[path[-1]])
            paths.append((path, 0)); seen.update(path)
        for x in self.nodes:                                      # what is left lies on cycles: ascending, so x is its cycle's smallest code
            if x in seen:
                continue
            path = [x]
            while nxt[path[-1]] != x:
                path.append(nxt[path[-1]])
            paths.append((path, CIRCULAR)); seen.update(path)
        paths.sort(key=lambda p: p[0][0])
        assert len(seen) == len(self.nodes) == sum(len(p) for p, _ in paths)
        self.members = [p for p, _ in paths]
        first_of = {p[0]: u for u, (p, _) in enumerate(paths)}
        self.where = {x: (u, j) for u, (p, _) in enumerate(paths) for j, x in enumerate(p)}
        kept = kept_comps(skip)
        self.unitigs = []
        for path, flags in paths:
            ranks = [(path[0] >> (2 * (k - 1 - j))) & 3 for j in range(k)] + [x & 3 for x in path[1:]]
            links = [NONE] * 4
            if not flags:
                for r, y in enumerate(successors(path[-1], k)):
                    if y in solid:
                        links[r] = first_of[y]                    # a KeyError here would break the rule: y is first in its unitig
            self.unitigs.append((kept[ranks], len(path), sum(table[x] for x in path), flags, links))

    S = property(lambda s: len(s.nodes))
    U = property(lambda s: len(s.unitigs))
    symbols = property(lambda s: sum(u[1] + s.k - 1 for u in s.unitigs))
    longest = property(lambda s: max([u[1] for u in s.unitigs] + [0]))
    circular_nodes = property(lambda s: sum(u[1] for u in s.unitigs if u[3] & CIRCULAR))

    def arrays(self, first=0, count=None):
        """(offsets, text, nodes, occurrences, flags, links) of the unitigs [first, first + count) as bwtm_unitigs_download lays them out."""
        part = self.unitigs[first: None if count is None else first + count]
        offsets = np.zeros(len(part) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([u[0].size for u in part])
        text = np.concatenate([u[0] for u in part] + [np.zeros(0, dtype=np.uint8)])
        return (offsets, text, np.array([u[1] for u in part], dtype=np.uint64), np.array([u[2] for u in part], dtype=np.uint64),
                np.array([u[3] for u in part], dtype=np.uint8), np.array([v for u in part for v in u[4]], dtype=np.uint64))

    def place(self, codes):
        got = [self.where.get(int(c), (NONE, NONE)) for c in codes]
        return np.array([g[0] for g in got], dtype=np.uint64), np.array([g[1] for g in got], dtype=np.uint64)

    def gfa(self):
        """The lines bwt_unitigs writes."""
        lines = ["H\tVN:Z:1.0"]
        for u, (text, _, occ, flags, _) in enumerate(self.unitigs):
            lines.append("S\t%d\t%s\tKC:i:%d%s" % (u, "".join("$ACGTN"[v] for v in text), occ, "\tTP:Z:circular" if flags & CIRCULAR else ""))
        for u, unitig in enumerate(self.unitigs):
            lines += ["L\t%d\t+\t%d\t+\t%dM" % (u, v, self.k - 1) for v in unitig[4] if v != NONE]
        return lines


def rand_row(seed, n):
    return np.random.default_rng(seed).integers(1, 5, size=n).astype(np.uint8)


def bubble_rows():
    left, right = rand_row(31, 30), rand_row(32, 30)
    return [np.concatenate([left, comps_of(mid), right]) for mid in "AC"]


def long_cycle_rows():
    s = rand_row(33, 3000)
    return [np.concatenate([s, s[:11]])]


# name -> (rows, k)
HAND = {
    "short_cycle": (lambda: [comps_of("ACGTACGTACGT")], 5),
    "homopolymer": (lambda: [comps_of("AAAAAAAA")], 4),
    "bubble": (bubble_rows, 8),
    "tailed_cycle": (lambda: [comps_of("TTGCA" + "ACGTACGTACGT")], 5),
    "long_cycle": (long_cycle_rows, 12),
    "k1": (lambda: [comps_of("ACGTTGCA")], 1),
}

def reads_with_n():
    rows = rand_row(36, 60).reshape(3, 20)
    rows[0, 9] = 5; rows[2, 0] = 5; rows[2, 19] = 5
    return list(rows) + [rows[1].copy()]


# name -> (rows, k, t, skip): the collections of the GPU test beyond the hand-made ones
COLLECTIONS = {
    "genome_k12_t3": (lambda: list(genome_reads()), 12, 3, 5),
    "genome_k12_t1": (lambda: list(genome_reads()), 12, 1, 5),
    "iid_k12_t1": (lambda: list(iid_reads()), 12, 1, 5),
    "iid_k6_t1": (lambda: list(iid_reads()), 6, 1, 5),
    "genome_k31_t2": (lambda: list(genome_reads()), 31, 2, 5),
    "genome_k8_t3": (lambda: list(genome_reads()), 8, 3, 5),
    "read200_k32": (lambda: [rand_row(34, 200)], 32, 1, 5),
    "read5000_k16": (lambda: [rand_row(35, 5000)], 16, 1, 5),
    "sorted_alphabet_k12_t3": (lambda: [sorted_alphabet(r) for r in genome_reads()], 12, 3, 4),
    "iid_sorted_alphabet_k9_t1": (lambda: [sorted_alphabet(r) for r in iid_reads()[:300]], 9, 1, 4),
    "reads_with_n_k5": (reads_with_n, 5, 1, 5),
}


def sorted_alphabet(row):
    """$ A C G N T: T is comp 5 and N comp 4."""
    return np.array([0, 1, 2, 3, 5, 4], dtype=np.uint8)[row]


@functools.lru_cache(maxsize=None)
def case(name):
    """(rows, k, t, skip, Graph) of a hand-made case or a collection: computed once, shared, not to be changed."""
    if name in HAND:
        make, k = HAND[name]
        rows, t, skip = make(), 1, 5
    else:
        make, k, t, skip = COLLECTIONS[name]
        rows = make()
    return rows, k, t, skip, Graph(table_of(rows, k, skip), k, t, skip)
