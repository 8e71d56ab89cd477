"""The brute force of the unitig tests on its own (no GPU, no library): tests/unitig_inputs.py restates the rule of include/bwtm.h for
bwtm_unitigs_create; here its results on the hand-made collections are the ones worked out by hand, and on the two read collections of
the k-mer tests they have the properties the rule promises."""
import numpy as np
import pytest

from kmer_inputs import decode
from unitig_inputs import CIRCULAR, NONE, case, predecessors, successors


def text(g, u):
    return "".join("$ACGTN"[v] for v in g.unitigs[u][0])


def test_short_cycle():
    g = case("short_cycle")[4]
    assert g.S == 4 and g.U == 1
    assert text(g, 0) == "ACGTACGT" and g.unitigs[0][1:] == (4, 8, CIRCULAR, [NONE] * 4)


def test_homopolymer():
    g = case("homopolymer")[4]
    assert g.S == 1 and g.U == 1
    assert text(g, 0) == "AAAA" and g.unitigs[0][1:] == (1, 5, CIRCULAR, [NONE] * 4)


def test_bubble():
    rows, k, _, _, g = case("bubble")
    assert g.S == 62 and sorted(u[1] for u in g.unitigs) == [8, 8, 23, 23] and g.circular_nodes == 0
    left = [u for u in range(4) if g.unitigs[u][0].tolist() == rows[0][:30].tolist()]
    right = [u for u in range(4) if g.unitigs[u][0].tolist() == rows[0][31:].tolist()]
    assert len(left) == 1 and len(right) == 1
    arms = sorted(set(range(4)) - set(left + right))
    assert sorted(v for v in g.unitigs[left[0]][4] if v != NONE) == arms
    for a in arms:
        assert [v for v in g.unitigs[a][4] if v != NONE] == right and g.unitigs[a][1] == 8
    assert g.unitigs[right[0]][4] == [NONE] * 4


def test_tailed_cycle():
    g = case("tailed_cycle")[4]
    assert g.S == 9 and sorted(u[1] for u in g.unitigs) == [4, 5] and g.circular_nodes == 0
    cycle = [u for u in range(2) if g.unitigs[u][1] == 4][0]
    assert [v for v in g.unitigs[cycle][4] if v != NONE] == [cycle]                 # it links to itself
    assert [v for v in g.unitigs[1 - cycle][4] if v != NONE] == [cycle]             # and the tail leads into it
    assert text(g, 1 - cycle) == "TTGCAACGT" and sorted(text(g, cycle)) == sorted("ACGTACGT")


def test_long_cycle():
    rows, _, _, _, g = case("long_cycle")
    assert g.S == 3000 and g.U == 1 and g.unitigs[0][1] == 3000 and g.unitigs[0][3] == CIRCULAR
    t = g.unitigs[0][0]
    assert t.size == 3011 and np.array_equal(t[-11:], t[:11]) and g.members[0][0] == min(g.members[0])
    doubled = np.concatenate([rows[0][:3000]] * 2)                                  # the text is a rotation of the string
    at = [j for j in range(3000) if np.array_equal(doubled[j: j + 3011], t)]
    assert len(at) == 1


def test_k1():
    g = case("k1")[4]
    assert g.S == 4 and g.U == 4 and [u[1] for u in g.unitigs] == [1] * 4
    assert [u[4] for u in g.unitigs] == [[0, 1, 2, 3]] * 4 and [u[2] for u in g.unitigs] == [2] * 4


@pytest.mark.parametrize("name,nodes,unitigs,longest", [("genome_k12_t3", 2977, 4, 1470), ("genome_k12_t1", 9218, 1550, None),
                                                       ("iid_k12_t1", 51433, 2802, None), ("iid_k6_t1", 4096, 4096, None)])
def test_collections_have_the_rules_properties(name, nodes, unitigs, longest):
    _, k, _, skip, g = case(name)
    assert (g.S, g.U) == (nodes, unitigs) and g.circular_nodes == 0
    if longest is not None:
        assert g.longest == longest
    if name == "iid_k6_t1":
        assert all(len(g.out[x]) == 4 and len(g.inn[x]) == 4 for x in g.nodes)
    # every solid k-mer is in exactly one unitig at one offset
    seen = [x for p in g.members for x in p]
    assert sorted(seen) == g.nodes and len(set(seen)) == len(seen)
    assert all(g.members[u][j] == x for x, (u, j) in g.where.items())
    # unitigs are numbered by the code of their first node
    firsts = [p[0] for p in g.members]
    assert firsts == sorted(firsts)
    rank = np.zeros(6, dtype=np.uint64)
    rank[[c for c in range(1, 6) if c != skip]] = np.arange(4, dtype=np.uint64)
    inside, linked = set(), set()
    for u, (t, n, occ, flags, links) in enumerate(g.unitigs):
        # the k-mers read off the text are the unitig's nodes in order
        assert t.size == n + k - 1
        windows = np.lib.stride_tricks.sliding_window_view(t, k)
        codes = np.zeros(n, dtype=np.uint64)
        for j in range(k):
            codes |= rank[windows[:, j]] << np.uint64(2 * (k - 1 - j))
        assert codes.tolist() == g.members[u]
        assert np.array_equal(decode(codes[:1], k, skip)[0], t[:k])
        inside.update(zip(g.members[u][:-1], g.members[u][1:]))
        for r, v in enumerate(links):
            if v != NONE:
                assert g.members[v][0] == successors(g.members[u][-1], k)[r]
                linked.add((g.members[u][-1], g.members[v][0]))
    # the links are exactly the edges that are not inside a unitig
    edges = {(x, y) for x in g.nodes for y in g.out[x]}
    assert edges == {(y, x) for x in g.nodes for y in g.inn[x]} and all(x in predecessors(y, k) for x, y in edges)
    assert inside <= edges and linked == edges - inside and not (inside & linked)
    assert len(linked) == sum(v != NONE for u in g.unitigs for v in u[4])
