"""The bounded-mismatch search, the parts that need no GPU: the brute force the GPU tests expect (tests/approx_inputs.py) is pinned to the
oracle -- at d = 0 it is the oracle's backward search, at d = 1 and 2 the oracle's search of every Hamming neighbour -- and the entry points
are bound."""
import functools

import numpy as np

from approx_inputs import Collection, batch_peaks, cut_patterns, genome_reads, iid_reads, neighbours, text_of


@functools.lru_cache(maxsize=None)
def collection(name):
    return Collection(list({"iid": iid_reads, "genome": genome_reads}[name]()))


def oracle_range(f, pattern):
    s, e = f.find(np.ascontiguousarray(pattern, dtype=np.uint8))
    return int(s), int(e)


def by_enumeration(f, pattern, d):
    """The hits of a pattern through the oracle: every neighbour searched on its own, the non-empty ranges kept, in the documented order."""
    found = []
    for key, dist in neighbours(pattern, d).items():
        w = np.frombuffer(key, dtype=np.uint8)
        s, e = oracle_range(f, w)
        if (e + 1 - s) % (1 << 64) != 0 and e >= s:
            found.append((tuple(w[::-1].tolist()), s, e - s + 1, dist))
    found.sort()
    return [row[1:] for row in found]


def test_the_calls_are_bound(bwtm):
    bound = {name: args for name, _, args in bwtm.capi.SYMBOLS}
    for name, nargs in (("bwtm_find_approx_batch", 11), ("bwtm_find_approx_stats", 1)):
        assert name in bound and len(bound[name]) == nargs and hasattr(bwtm.capi.lib(), name), name
    assert callable(bwtm.Index.find_approx) and callable(bwtm.Locator.locate_approx) and callable(bwtm.find_approx_stats)


def test_d0_is_the_oracles_find(oracle):
    for name, seed in (("iid", 1), ("genome", 2)):
        coll = collection(name)
        f = oracle.FMI.from_text(text_of(coll.rows))
        patterns = cut_patterns(coll.rows, (0, 1, 2, 3, 12, 31, 40, 41), 6, seed, substitutions=0) + cut_patterns(coll.rows, (3, 12, 40), 6, seed + 10)
        hits = 0
        for p in patterns:
            sp, count, mm, strings = coll.hits(p, 0)
            s, e = oracle_range(f, p)
            if p.size == 0:
                assert (s, e) == (0, coll.n - 1) and (sp.tolist(), count.tolist(), mm.tolist()) == ([0], [coll.n], [0])
            elif (e + 1 - s) % (1 << 64) == 0 or e < s:
                assert sp.size == 0, (name, p)
            else:
                assert (sp.tolist(), count.tolist(), mm.tolist()) == ([s], [e - s + 1], [0]) and np.array_equal(strings[0], p), (name, p)
                hits += 1
        assert 40 <= hits < len(patterns)                                          # both outcomes are among the patterns


def test_d1_and_d2_are_the_oracles_find_over_every_neighbour(oracle):
    for name, seed in (("iid", 3), ("genome", 4)):
        coll = collection(name)
        f = oracle.FMI.from_text(text_of(coll.rows))
        several = 0
        for d, lengths, per in ((1, (1, 2, 3, 6, 12), 4), (2, (1, 2, 4, 7), 3)):
            for p in cut_patterns(coll.rows, lengths, per, seed + d):
                sp, count, mm, strings = coll.hits(p, d)
                want = by_enumeration(f, p, d)
                assert list(zip(sp.tolist(), count.tolist(), mm.tolist())) == want, (name, d, p)
                several += (sp.size > 1)
                assert np.all((strings != p).sum(axis=1) == mm) and int(mm.max(initial=0)) <= d
        assert several >= 10


def test_the_collections_are_as_hard_as_the_gpu_tests_need(oracle):
    """One pattern's frontier at d = 3 spans several workgroups of 256 nodes, and the levels at which patterns of mixed lengths finish differ."""
    for name in ("iid", "genome"):
        coll = collection(name)
        p = cut_patterns(coll.rows, (12,), 1, 5)[0]
        nodes = coll.frontier(p, 3)
        assert nodes[0] == 1 and max(nodes) > 512, (name, nodes)
        P, H, T = batch_peaks(coll, [p, p[:3], p[:0]], 3)
        assert P >= max(nodes) and H >= 2 and T == 15
