"""The long-sequence extraction and the scrambled refusals of tests/test_gpu_walks.py in a process of its own (not a test module): the
child that test_on_a_poisoned_pool starts with BWTM_POOL_POISON in its environment, which the library reads once per process.
The last lines on stdout are "POISON fills=<n> bytes=<n>" (bwtm_pool_poison_stats) and "OK"."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import _pkg
    from oracle import oracle as orc
    from test_gpu_walks import test_long_sequences_around_the_default_bound, test_scrambled_refusals
    pkg = _pkg.load()
    pkg.init(0)
    # the larger case first: the refusals' batches are cut from recycled blocks that hold the long sequences' bytes or the poison
    test_long_sequences_around_the_default_bound(pkg, orc, 4)
    test_long_sequences_around_the_default_bound(pkg, orc, 0)
    test_scrambled_refusals(pkg, orc, "small")
    pkg.synchronize()
    print("POISON fills=%d bytes=%d" % pkg.pool_poison_stats())
    print("OK")


if __name__ == "__main__":
    main()
