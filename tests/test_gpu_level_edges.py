"""The placement the four level-wise searches share (kernels/level.hip.h: ballots within a wave, wave totals through LDS, workgroup slots through
the scan) at exact wave and workgroup edges, which the ragged frontiers of the other tests may step over: frontiers that end one lane before,
on and one lane behind the last lane of a wave (64) and of a workgroup (256), and levels of exactly one and four full workgroups.  Every result
is compared exactly with the brute force of tests/approx_inputs.py, edit_inputs.py, kmer_inputs.py and kmer_join_inputs.py."""
import functools

import numpy as np
import pytest

import edit_inputs
from approx_inputs import Collection, cut_patterns, expected, iid_reads, text_of
from kmer_inputs import brute, brute_levels
from kmer_join_inputs import brute_pair, brute_pair_levels

pytestmark = pytest.mark.gpu
EDGES = (63, 64, 65, 255, 256, 257)


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    return bwtm


def uploaded(gpu, oracle, rows):
    f = oracle.FMI.from_text(text_of(list(rows)))
    assert f.sequences == len(rows)
    return gpu.Index.upload(f.data, f.sequences, f.bases)


@pytest.fixture(scope="module")
def iid(gpu, oracle):
    x = uploaded(gpu, oracle, iid_reads())
    yield x
    x.free()


@functools.lru_cache(maxsize=None)
def patterns():
    """258 patterns of 1, 2 and 3 symbols cut from the reads, in mixed order: a batch is a prefix of them, its root frontier has one node each."""
    cut = cut_patterns(list(iid_reads()), (1, 2, 3), 86, 21, substitutions=0)
    order = np.random.default_rng(22).permutation(len(cut))
    return [cut[j] for j in order.tolist()]


@functools.lru_cache(maxsize=None)
def whole(search):
    """The expected result of all 258 patterns, once; a pattern's hits do not depend on its batch."""
    if search == "approx":
        return expected(Collection(list(iid_reads())), patterns(), 1)
    return edit_inputs.expected(edit_inputs.collection("iid"), patterns(), 1)


def prefix(want, nb):
    """The expected result of the first nb patterns."""
    total = int(want[0][nb])
    return (want[0][: nb + 1],) + tuple(a[:total] for a in want[1:])


@pytest.mark.parametrize("nb", EDGES)
@pytest.mark.parametrize("search", ["approx", "edit"])
def test_root_frontiers_that_end_at_a_wave_or_workgroup_edge(gpu, iid, search, nb):
    batch = patterns()[:nb]
    assert sorted({len(p) for p in batch}) == [1, 2, 3]
    got = iid.find_approx(batch, 1) if search == "approx" else iid.find_edit(batch, 1)
    want = prefix(whole(search), nb)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    stats = gpu.find_approx_stats() if search == "approx" else gpu.find_edit_stats()
    assert stats["frontier_peak"] >= nb and stats["batch_hits"] == int(want[0][-1]) > nb      # the hit stream crosses the same edges, later


@pytest.mark.parametrize("k", [4, 5])
def test_kmer_levels_of_whole_workgroups(gpu, iid, k):
    rows = list(iid_reads())
    km = iid.kmers(k)
    levels = km.levels()
    assert int(levels[k - 1]) == 4 ** k and 4 ** k in (256, 1024)                             # one and four full workgroups, no lane idle
    assert np.array_equal(levels, brute_levels(rows, k, 5))
    want = brute(rows, k, 5)
    for g, w in zip(km.download(), want):
        assert np.array_equal(g, w)
    assert km.distinct == want[0].size == 4 ** k
    km.free()


@pytest.mark.parametrize("k", [4, 5])
def test_kmer_join_levels_of_whole_workgroups(gpu, oracle, iid, k):
    rows_a, rows_b = iid_reads(), iid_reads(17)
    other = uploaded(gpu, oracle, rows_b)
    kj = iid.kmer_join(other, k)
    levels = kj.levels()
    assert int(levels[k - 1]) == 4 ** k and 4 ** k in (256, 1024)
    assert np.array_equal(levels, brute_pair_levels(rows_a, rows_b, k, 5))
    want = brute_pair(rows_a, rows_b, k, 5)
    for g, w in zip(kj.download(), want):
        assert np.array_equal(g, w)
    assert kj.distinct == want[0].size == 4 ** k
    kj.free(); other.free()
