"""The iid case of tests/test_gpu_kmers.py at k = 12 in a process of its own (not a test module): the child that test_on_a_poisoned_pool
starts with BWTM_POOL_POISON in its environment, which the library reads once per process.  Twice, with the genome collection and a threshold
in between, so that the later runs' blocks are recycled ones, and the spectrum.
The last lines on stdout are "POISON fills=<n> bytes=<n>" (bwtm_pool_poison_stats) and "OK"."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import numpy as np
    import _pkg
    from oracle import oracle as orc
    from kmer_inputs import brute, brute_levels, folded_histogram, genome_reads, iid_reads
    from test_gpu_kmers import same_kmers, uploaded
    pkg = _pkg.load()
    pkg.init(0)
    rows, grows = iid_reads(), genome_reads()
    x, g = uploaded(pkg, orc, rows), uploaded(pkg, orc, grows)
    want, want_levels = brute(list(rows), 12, 5), brute_levels(list(rows), 12, 5)
    gwant = brute(list(grows), 12, 5, 2)
    for again in range(2):                                                       # the second round's blocks are the first one's, given back
        km = x.kmers(12)
        same_kmers(km, want)
        assert np.array_equal(km.levels(), want_levels)
        assert np.array_equal(km.histogram(16), folded_histogram(want[1], 16))
        km.free()
        km = g.kmers(12, min_count=2)
        same_kmers(km, gwant)
        assert np.array_equal(km.histogram(4096), folded_histogram(gwant[1], 4096))
        km.free()
    pkg.synchronize()
    print("POISON fills=%d bytes=%d" % pkg.pool_poison_stats())
    print("OK")


if __name__ == "__main__":
    main()
