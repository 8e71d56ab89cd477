"""k-mers, the parts that need no GPU: the expected values of the GPU tests (tests/kmer_inputs.py) are checked here against the oracle -- the
backward search of a listed k-mer on the oracle's FMI gives exactly its count and the first position of its range, an absent k-mer gives an
empty range -- and the two collections are as hard as the GPU tests need them."""
import numpy as np

from kmer_inputs import brute, decode, folded_histogram, genome_reads, iid_reads, text_of

K = 12


def check_against_the_oracle(oracle, rows, skip, seed):
    f = oracle.FMI.from_text(text_of(list(rows)))
    codes, counts, sp = brute(list(rows), K, skip)
    assert np.all(codes[1:] > codes[:-1]) and np.all(sp[1:] > sp[:-1])
    assert int(counts.sum()) == sum(1 for row in rows for o in range(len(row) - K + 1) if skip not in row[o: o + K])
    rng = np.random.default_rng(seed)
    picks = rng.choice(codes.size, size=200, replace=False)
    for j, pattern in zip(picks.tolist(), decode(codes[picks], K, skip)):
        s, e = oracle_range(f, pattern)
        assert e - s + 1 == int(counts[j]) and s == int(sp[j]), (j, s, e)
    absent = []
    listed = set(codes.tolist())
    while len(absent) < 50:
        c = int(rng.integers(0, 1 << (2 * K)))
        if c not in listed:
            absent.append(c)
    for pattern in decode(np.array(absent, dtype=np.uint64), K, skip):
        s, e = oracle_range(f, pattern)
        assert (e + 1 - s) % (1 << 64) == 0                                       # ep - sp + 1 == 0 in the oracle's unsigned arithmetic
    return codes, counts


def oracle_range(f, pattern):
    s, e = f.find(np.ascontiguousarray(pattern, dtype=np.uint8))
    return int(s), int(e)


def test_bwt_kmers_builds_and_the_calls_are_bound(bwtm):
    import os
    import subprocess
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwt-merge_amd", "csrc", "host")
    bwtm.build()
    subprocess.check_call(["make", "-C", host, "-s"])
    out = subprocess.run([os.path.join(host, "bwt_kmers")], capture_output=True, text=True)
    assert out.returncode == 0 and "Usage: bwt_kmers [options] input output" in out.stderr
    for option in ("-g N", "-i format", "-k N", "-c N", "-H N"):
        assert option in out.stderr, option
    bound = {name: args for name, _, args in bwtm.capi.SYMBOLS}
    for name, nargs in (("bwtm_kmers_create", 5), ("bwtm_kmers_free", 1), ("bwtm_kmers_distinct", 1), ("bwtm_kmers_total", 1), ("bwtm_kmers_bytes", 1),
                        ("bwtm_kmers_levels", 2), ("bwtm_kmers_download", 6), ("bwtm_kmers_histogram", 3)):
        assert name in bound and len(bound[name]) == nargs and hasattr(bwtm.capi.lib(), name), name
    assert all(callable(getattr(bwtm.Kmers, f)) for f in ("levels", "download", "histogram", "free")) and callable(bwtm.Index.kmers)
    # the binding's decoder against the test's own: 2 bits per symbol, the first symbol highest, the skip symbol left out of the alphabet
    codes = np.array([0, 1, 0b111001, (1 << 64) - 1, 3 << 62], dtype=np.uint64)
    for k, skip in ((3, 5), (3, 4), (32, 5), (32, 1)):
        assert np.array_equal(bwtm.decode_kmers(codes, k, skip), decode(codes, k, skip))
    assert bwtm.decode_kmers(codes[2:3], 3, 5).tolist() == [[4, 3, 2]] and bwtm.decode_kmers(codes[2:3], 3, 4).tolist() == [[5, 3, 2]]


def test_iid_collection_against_the_oracle(oracle):
    rows = iid_reads()
    assert rows.shape == (2000, 40) and 400 < int((rows == 5).sum()) < 1200
    codes, counts = check_against_the_oracle(oracle, rows, 5, 1)
    assert codes.size >= 40000                                                   # expected about 51 000: most windows are k-mers of their own


def test_genome_collection_against_the_oracle(oracle):
    rows = genome_reads()
    assert rows.shape == (2000, 40) and rows.min() == 1 and rows.max() == 4
    codes, counts = check_against_the_oracle(oracle, rows, 5, 2)
    hist = folded_histogram(counts, 64)
    assert int(np.argmax(hist[2:])) + 2 > 5                                      # the coverage peak, beyond the error k-mers of count 1
    kept = brute(list(rows), K, 5, min_count=3)[0].size
    assert codes.size - kept >= 1000 and kept >= 2500
