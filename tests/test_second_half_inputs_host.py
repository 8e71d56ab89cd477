"""The pairs of tests/second_half_inputs.py reach what tests/test_gpu_second_half_forms.py needs them for: conditions on the inputs, checked
against the CPU oracle alone (no GPU), so that an edit of a generator cannot silently empty the GPU tests.  The measured values are in the
docstring of second_half_inputs.py; every floor here leaves room below them."""
import numpy as np
import pytest

import second_half_inputs as shi


@pytest.fixture(scope="module")
def measured(oracle):
    """{name: (a, b, properties)}, computed once (read only)."""
    out = {}
    for name in shi.PAIRS:
        a, b = shi.pair(oracle, name)
        out[name] = (a, b, shi.properties(oracle, a, b))
    return out


def test_properties_of_a_hand_made_pair(oracle):
    """properties() itself, on a merge small enough to count by hand: a = 3 x "CC", b = 2 x "CC" -- the merged BWT is C x 10, $ x 5, one
    two-source run of 10 and one of 5, no cut."""
    a = oracle.FMI.from_text(oracle.text_from_strings(["CC"] * 3)); b = oracle.FMI.from_text(oracle.text_from_strings(["CC"] * 2))
    p = shi.properties(oracle, a, b)
    assert (p["positions"], p["runs"], p["longest_run"], p["cuts"]) == (15, 2, 10, 0)
    assert p["two_source_runs_ge_42"] == 0 and p["cuts_inside_two_source_run"] == 0 and p["halo_from_a"] + p["halo_from_b"] == 0
    assert p["chunks_all_a"] == 0 and p["chunks_all_b"] == 0 and p["longest_block"] == 15


def test_genome60_cuts_every_slice_inside_a_two_source_run(measured):
    a, b, p = measured["genome60"]
    assert p["two_source_runs_ge_42"] >= 3000                            # the two-byte forms of the encoder, by the thousand
    assert p["cuts"] == 9 and p["cuts_inside_two_source_run"] == p["cuts"]


def test_repeated_super_opens_two_source_runs_at_cuts_and_behind_a_super_block(measured):
    a, b, p = measured["repeated_super"]
    assert a.bases + b.bases > 2**25
    assert p["two_source_runs_ge_65536"] >= 16                           # runs that can fill a whole slice
    assert p["cuts_inside_two_source_run"] >= 60
    assert p["beyond_2_25"] >= 3
    assert p["headless_slices_in_two_source_runs"] >= 8
    assert p["halo_from_b"] >= 100 and p["halo_from_a"] >= 100
    assert 65535 <= p["longest_block"] < 2**32 - 1                       # compact width 4: every narrower guess of a streamed piece is wrong
    assert p["chunks_all_a"] >= 500 and p["chunks_all_b"] >= 500


@pytest.mark.parametrize("name", ["homopolymer", "two_homopolymers"])
def test_homopolymer_collections_span_many_frontier_blocks(measured, name):
    a, b, p = measured[name]
    assert a.sequences > 2048 and b.sequences > 2048                     # more than 8 blocks of FR_BLOCK = 256 elements a side
    for x in (a, b):
        assert np.count_nonzero(x.character_counts[1:]) <= 2
    assert p["two_source_runs_ge_42"] >= 150


@pytest.mark.parametrize("name", ["tiny_into_runs", "runs_into_tiny"])
def test_tiny_pairs_set_a_single_record_against_long_runs(measured, name):
    a, b, p = measured[name]
    small, large = (b, a) if name == "tiny_into_runs" else (a, b)
    assert small.bases < 128 and small.sequences == 3
    assert large.bases > 2**24
    # at most one chunk per position of the tiny side holds both sources: chunks of one source, up to the last one
    chunks = (p["positions"] + shi.CHUNK - 1) // shi.CHUNK
    assert p["chunks_all_a" if name == "tiny_into_runs" else "chunks_all_b"] >= chunks - small.bases > 2000
