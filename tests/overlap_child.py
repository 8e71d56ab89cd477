"""The all-reads case and the batching case of tests/test_gpu_overlap.py in a process of its own (not a test module): the child that
test_on_a_poisoned_pool starts with BWTM_POOL_POISON in its environment, which the library reads once per process.
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
    from test_gpu_overlap import test_all_reads_as_queries, test_batches_give_the_same_result
    pkg = _pkg.load()
    pkg.init(0)
    # the larger case first: the second one's counts, records and outputs are cut from recycled blocks that hold the first one's bytes or the poison
    test_batches_give_the_same_result(pkg, orc)
    test_all_reads_as_queries(pkg, orc)
    pkg.synchronize()
    print("POISON fills=%d bytes=%d" % pkg.pool_poison_stats())
    print("OK")


if __name__ == "__main__":
    main()
