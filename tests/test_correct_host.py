"""The yardstick of the error-correction tests, checked before any kernel is measured against it (no GPU, no library): the brute force of
tests/correct_inputs.py on hand-made reads whose outcome is written down by hand, one for every branch of the rule in include/bwtm.h, and
on the two simulated collections, where it has to bring back the reads the errors were put into."""
import functools

import numpy as np
import pytest

import kmer_inputs
from correct_inputs import (CLEAN, CORRECTED, FAILED, HAND_K, HAND_T, SHORT, as_bytes, correct, correct_all, genome_truth, hand_made, long_reads,
                            solid_count, table_of)


def test_truth_is_the_collection_before_its_errors():
    rows, truth = kmer_inputs.genome_reads(), genome_truth()
    assert rows.shape == truth.shape
    differ = (rows != truth)
    assert 0.005 < differ.mean() < 0.015 and truth.min() >= 1 and truth.max() <= 4


def test_table_counts_windows_without_skip():
    rows = [np.array([1, 2, 3, 1, 2, 3], dtype=np.uint8), np.array([1, 2, 5, 1, 2], dtype=np.uint8), np.array([1], dtype=np.uint8)]
    table = table_of(rows, 2)
    assert dict(table) == {b"\x01\x02": 4, b"\x02\x03": 2, b"\x03\x01": 1}
    assert solid_count(table, 2) == 2 and solid_count(table, 0) == 3 and solid_count(table, 5) == 0
    assert dict(table_of(rows, 2, skip=3)) == {b"\x01\x02": 4, b"\x02\x05": 1, b"\x05\x01": 1}


@pytest.mark.parametrize("case", range(len(hand_made()[1])))
def test_hand_made_reads(case):
    collection, cases = hand_made()
    name, read, rounds, status, text, edits = cases[case]
    table = table_of(collection, HAND_K)
    got = correct(read, table, HAND_K, HAND_T, rounds)
    assert got == (text, status, edits), name
    if status == FAILED:
        assert got[0] == as_bytes(read), name


def test_hand_made_reads_cover_every_branch():
    names = [c[0] for c in hand_made()[1]]
    for want in ("shorter than k", "m == k, clean", "m == k, one error", "m == k + 1", "position 0", "k - 2", "m - 1", "two rounds", "R too small", "R = 0 on a clean",
                 "R = 0 on an error", "resolved by the second", "ambiguous in both", "N at the error", "N elsewhere"):
        assert any(want in n for n in names), want
    assert {c[3] for c in hand_made()[1]} == {CLEAN, CORRECTED, FAILED, SHORT}


@functools.lru_cache(maxsize=None)
def genome_corrected():
    return correct_all(list(kmer_inputs.genome_reads()), 12, 3, 10)


def test_genome_reads_are_restored():
    rows, truth = kmer_inputs.genome_reads(), genome_truth()
    text, status, edits = genome_corrected()
    with_errors = [j for j in range(len(rows)) if not np.array_equal(rows[j], truth[j])]
    restored = sum(1 for j in with_errors if text[j] == as_bytes(truth[j]))
    changed = sum(1 for j in range(len(rows)) if np.array_equal(rows[j], truth[j]) and text[j] != as_bytes(rows[j]))
    print("restored %d of %d, changed %d, statuses %s" % (restored, len(with_errors), changed, np.bincount(status, minlength=4).tolist()))
    assert restored >= 0.95 * len(with_errors) and changed == 0
    assert all(status[j] != CORRECTED or (edits[j] > 0 and text[j] != as_bytes(rows[j])) for j in range(len(rows)))
    assert all(status[j] == CORRECTED or (edits[j] == 0 and text[j] == as_bytes(rows[j])) for j in range(len(rows)))


@pytest.mark.parametrize("k", [21, 31, 32])
def test_long_reads_reach_every_status(k):
    rows, truth = long_reads()
    text, status, edits = correct_all(rows, k, 3, 10)
    counts = np.bincount(status, minlength=4).tolist()
    print("k = %d: statuses %s, most edits %d, reads over 256 windows %d" % (k, counts, int(edits.max()), sum(1 for r in rows if len(r) - k + 1 > 256)))
    assert all(c > 0 for c in counts), counts
    changed = sum(1 for j in range(len(rows)) if np.array_equal(rows[j], truth[j]) and text[j] != as_bytes(rows[j]))
    assert changed == 0
    assert status[[j for j in range(len(rows)) if len(rows[j]) < k]].tolist() == [SHORT] * sum(1 for r in rows if len(r) < k)
    if k == 21:
        assert int(edits.max()) >= 5
        assert sum(1 for r in rows if len(r) - k + 1 > 256) > 0
        restored = sum(1 for j in range(len(rows)) if status[j] == CORRECTED and text[j] == as_bytes(truth[j]))
        assert restored >= 0.95 * counts[CORRECTED]
