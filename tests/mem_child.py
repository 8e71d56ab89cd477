"""The all-reads case and the varied-reads case of tests/test_gpu_mem.py in a process of its own (not a test module): the child that
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
    from test_gpu_mem import check_all_reads, check_varied_reads, collection
    pkg = _pkg.load()
    pkg.init(0)
    # the larger case first: the second one's lengths, flags and outputs are cut from recycled blocks that hold the first one's bytes or the poison
    x, rows, brute = collection(pkg, orc, 1000, 2)
    check_all_reads(pkg, x, rows, brute)
    x.free()
    x, rows, brute = collection(pkg, orc, 300, 1)
    check_varied_reads(pkg, x, rows, brute, 21)
    check_all_reads(pkg, x, rows, brute)
    x.free()
    pkg.synchronize()
    print("POISON fills=%d bytes=%d" % pkg.pool_poison_stats())
    print("OK")


if __name__ == "__main__":
    main()
