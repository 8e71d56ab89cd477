"""The contract of bwtm_matching_stats_batch / bwtm_mem_batch without a GPU: the brute force of tests/mem_inputs.py against the oracle's
backward search on every reported substring and its two one-symbol extensions, and the rule on matching statistics (which the kernels
apply) against the three-condition definition of a MEM (which the brute force applies)."""
import numpy as np
import pytest

from mem_inputs import Brute, rule_mems, special_patterns, varied_patterns
from overlap_inputs import overlap_reads, rows_of
from test_gpu_sequences import text_of


@pytest.fixture(scope="module")
def collection(oracle):
    reads, lengths = overlap_reads(300, 1)
    rows = rows_of(reads, lengths)
    return oracle.FMI.from_text(text_of(reads, lengths)), rows, Brute(rows)


def found(f, w):
    sp, ep = f.find(np.array(list(w), dtype=np.uint8))
    return (sp, ep - sp + 1) if sp <= ep else None


def test_brute_force_equals_the_oracles_search(collection):
    """Every entry of the matching statistics and every MEM: the oracle finds the substring at the same range, and does not find it extended
    by one symbol of the pattern on either side (for the statistics: on the left)."""
    f, rows, brute = collection
    patterns = special_patterns(rows, 5) + varied_patterns(rows, 6)[::7] + rows[::5]
    entries = mems = zero = 0
    for p in patterns:
        p = bytes(p)
        for e, (l, sp, cnt) in enumerate(brute.stats(p), start=1):
            if l == 0:
                assert found(f, p[e - 1:e]) is None and (sp, cnt) == (0, 0)
                zero += 1
                continue
            assert found(f, p[e - l:e]) == (sp, cnt), (p, e)
            assert e == l or found(f, p[e - l - 1:e]) is None, (p, e)
            entries += 1
        for b, l, sp, cnt in brute.mems(p):
            assert found(f, p[b:b + l]) == (sp, cnt), (p, b, l)
            assert b == 0 or found(f, p[b - 1:b + l]) is None
            assert b + l == len(p) or found(f, p[b:b + l + 1]) is None
            mems += 1
    assert entries > 3000 and mems > 300 and zero > 10


def test_rule_on_matching_statistics_equals_the_definition(collection):
    """Random patterns over the reads' alphabet and cut from the reads with substitutions: the ends the rule picks are the MEMs of the three
    conditions, in the same order, for every min_length; l(e + 1) <= l(e) + 1; begins and ends ascend strictly."""
    f, rows, brute = collection
    rng = np.random.default_rng(11)
    patterns = [tuple(int(v) for v in rng.integers(1, 5, size=int(rng.integers(0, 90)))) for _ in range(150)]
    patterns += varied_patterns(rows, 12)[::3] + special_patterns(rows, 13) + rows[::4]
    seen = 0
    for p in patterns:
        lengths = brute.lengths(p)
        assert all(lengths[e] <= lengths[e - 1] + 1 for e in range(1, len(p)))
        for min_length in (1, 2, 5, 12, 40, 41):
            want = [(b, l) for b, l, _, _ in brute.mems(p, min_length)]
            assert rule_mems(lengths, min_length) == want, (p, min_length)
            assert all(a[0] < b[0] and a[0] + a[1] < b[0] + b[1] for a, b in zip(want, want[1:]))
            assert len(want) <= len(p)
            seen += len(want)
    assert seen > 5000
    assert brute.mems((), 1) == [] and brute.lengths(()) == []


def test_every_read_is_one_mem(collection):
    f, rows, brute = collection
    for r in rows:
        assert [(b, l) for b, l, _, _ in brute.mems(r)] == ([(0, len(r))] if len(r) > 0 else [])
