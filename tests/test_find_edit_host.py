"""The edit-distance search, the parts that need no GPU: the brute force the GPU tests expect (tests/edit_inputs.py) is pinned to the oracle
-- at e = 0 it is the oracle's backward search, at e = 1 the oracle's search of every string within one edit -- and to the Hamming brute
force of tests/approx_inputs.py, whose hits are among its own; the inputs of the GPU tests are as hard as those tests need; the entry
points are bound."""
import numpy as np

from approx_inputs import cut_patterns
from edit_inputs import MIXED_LENGTHS, batch_peaks, collection, edited_patterns, memory_patterns, mixed_budget, mixed_expected, mixed_patterns, text_of, within_one_edit


def oracle_range(f, pattern):
    s, e = f.find(np.ascontiguousarray(pattern, dtype=np.uint8))
    return int(s), int(e)


def test_the_calls_are_bound(bwtm):
    bound = {name: args for name, _, args in bwtm.capi.SYMBOLS}
    for name, nargs in (("bwtm_find_edit_batch", 12), ("bwtm_find_edit_stats", 1)):
        assert name in bound and len(bound[name]) == nargs and hasattr(bwtm.capi.lib(), name), name
    assert callable(bwtm.Index.find_edit) and callable(bwtm.Locator.locate_edit) and callable(bwtm.find_edit_stats)


def test_e0_is_the_oracles_find(oracle):
    for name, seed in (("iid", 1), ("genome", 2)):
        coll = collection(name)
        f = oracle.FMI.from_text(text_of(coll.rows))
        patterns = cut_patterns(coll.rows, (0, 1, 2, 3, 12, 31, 40, 41), 6, seed, substitutions=0) + cut_patterns(coll.rows, (3, 12, 40), 6, seed + 10)
        hits = 0
        for p in patterns:
            sp, count, edits, lengths, strings = coll.edit_hits(p, 0)
            s, e = oracle_range(f, p)
            if p.size == 0:
                assert (s, e) == (0, coll.n - 1) and (sp.tolist(), count.tolist(), edits.tolist(), lengths.tolist()) == ([0], [coll.n], [0], [0])
            elif (e + 1 - s) % (1 << 64) == 0 or e < s:
                assert sp.size == 0, (name, p)
            else:
                assert (sp.tolist(), count.tolist(), edits.tolist(), lengths.tolist()) == ([s], [e - s + 1], [0], [p.size]) and np.array_equal(strings[0], p), (name, p)
                hits += 1
        assert 40 <= hits < len(patterns)                                          # both outcomes are among the patterns


def test_e1_is_the_oracles_find_over_every_string_within_one_edit(oracle):
    for name, seed in (("iid", 3), ("genome", 4)):
        coll = collection(name)
        f = oracle.FMI.from_text(text_of(coll.rows))
        several = 0
        for p in edited_patterns(coll.rows, (0, 1, 2, 3, 6, 12), 4, seed):
            found = []
            for key, dist in within_one_edit(p).items():
                w = np.frombuffer(key, dtype=np.uint8)
                s, e = oracle_range(f, w)
                if w.size == 0:
                    found.append((0, (), 0, coll.n, dist))
                elif (e + 1 - s) % (1 << 64) != 0 and e >= s:
                    found.append((w.size, tuple(w[::-1].tolist()), s, e - s + 1, dist))
            found.sort()                                                           # shortest first, then from the last symbol backwards
            sp, count, edits, lengths, strings = coll.edit_hits(p, 1)
            assert list(zip(lengths.tolist(), sp.tolist(), count.tolist(), edits.tolist())) == [(row[0],) + row[2:] for row in found], (name, p)
            several += (sp.size > 1)
        assert several >= 10


def test_the_hamming_hits_are_among_the_edit_hits():
    for name, seed in (("iid", 5), ("genome", 6)):
        coll = collection(name)
        for e in (1, 2):
            for p in cut_patterns(coll.rows, (1, 2, 3, 7, 12), 3, seed + e, substitutions=e):
                hsp, hcount, hmm, _ = coll.hits(p, e)
                sp, count, edits, lengths, _ = coll.edit_hits(p, e)
                mine = {(int(a), int(b)): int(c) for a, b, c, l in zip(sp, count, edits, lengths) if int(l) == p.size}
                assert hsp.size >= 1
                for a, b, c in zip(hsp.tolist(), hcount.tolist(), hmm.tolist()):
                    assert (a, b) in mine and mine[(a, b)] <= c, (name, e, p)          # an indel pair can be cheaper than the substitutions
                assert len(mine) >= hsp.size


def test_the_inputs_are_as_hard_as_the_gpu_tests_need():
    for name in ("iid", "genome"):
        patterns = mixed_patterns(name)
        assert sorted(set(len(p) for p in patterns)) == list(MIXED_LENGTHS)
        for e in (1, 2, 3):
            hit_offsets, sp, count, edits, lengths = mixed_expected(name, e)
            run = mixed_budget(patterns, e)
            per = np.diff(hit_offsets)
            relative = set()
            nested = 0
            for j, p in enumerate(run):
                a, b = int(hit_offsets[j]), int(hit_offsets[j + 1])
                relative |= set((lengths[a:b].astype(np.int64) - len(p)).tolist())
                lo, hi = sp[a:b].astype(np.int64), (sp[a:b] + count[a:b]).astype(np.int64)
                inside = (lo[:, None] >= lo[None, :]) & (hi[:, None] <= hi[None, :])
                nested += int(inside.sum()) > b - a                                # some range lies within another one: W and xW are both hits
                crossing = (lo[:, None] < lo[None, :]) & (lo[None, :] < hi[:, None]) & (hi[:, None] < hi[None, :])
                assert not crossing.any()                                          # disjoint or nested, never overlapping
            assert relative == set(range(-e, e + 1)), (name, e, relative)          # every length m - e .. m + e carries a hit
            assert int(edits.max()) == e and nested >= 1 and int(per.max()) > 1
            assert e == 3 or int((per == 0).sum()) >= 1                            # some pattern has no hit at all
    # one 12-mer's frontier at e = 3 spans several workgroups of 256 nodes; six or more of them clear 20 workgroups by the reference alone
    for name in ("iid", "genome"):
        coll = collection(name)
        p = cut_patterns(coll.rows, (12,), 1, 5)[0]
        assert [max(coll.edit_frontier(p, e)) for e in (1, 2, 3)] == {"iid": [42, 688, 5140], "genome": [34, 420, 1962]}[name]
        hits = coll.edit_hits(p, 3)
        assert name != "iid" or np.bincount(hits[3], minlength=16)[9:16].tolist() == [21, 51, 58, 41, 23, 9, 3]
    coll = collection("iid")
    P, H, T = batch_peaks(coll, memory_patterns(), 3)
    assert P > 20 * 256 and H > 8 and T == 96

