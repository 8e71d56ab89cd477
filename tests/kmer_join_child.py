"""The genome pair of tests/test_gpu_kmer_join.py at k = 12 in a process of its own (not a test module): the child that
test_on_a_poisoned_pool starts with BWTM_POOL_POISON in its environment, which the library reads once per process.  The union and a filtered
join, twice, so that the second round's blocks are recycled ones.
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
    from kmer_join_inputs import brute_pair, brute_pair_levels, pair_reads
    from test_gpu_kmer_join import same_join, uploaded
    pkg = _pkg.load()
    pkg.init(0)
    ra, rb = pair_reads()
    A, B = uploaded(pkg, orc, ra), uploaded(pkg, orc, rb)
    fresh = dict(max_a=0, min_b=2)
    want, want_levels = brute_pair(ra, rb, 12, 5), brute_pair_levels(ra, rb, 12, 5)
    fwant, fwant_levels = brute_pair(ra, rb, 12, 5, **fresh), brute_pair_levels(ra, rb, 12, 5, **fresh)
    for again in range(2):                                                       # the second round's blocks are the first one's, given back
        kj = A.kmer_join(B, 12)
        same_join(kj, want)
        assert np.array_equal(kj.levels(), want_levels)
        kj.free()
        kj = A.kmer_join(B, 12, **fresh)
        same_join(kj, fwant)
        assert np.array_equal(kj.levels(), fwant_levels)
        kj.free()
    pkg.synchronize()
    print("POISON fills=%d bytes=%d" % pkg.pool_poison_stats())
    print("OK")


if __name__ == "__main__":
    main()
