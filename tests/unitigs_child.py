"""Cases of tests/test_gpu_unitigs.py in a process of its own (not a test module): the child that test_on_a_poisoned_pool starts with
BWTM_POOL_POISON in its environment, which the library reads once per process.  The larger graph runs first and smaller ones after it, so
that their blocks are recycled ones; then the same again with 700 nodes per launch.
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
    from test_gpu_unitigs import built, same
    pkg = _pkg.load()
    pkg.init(0)
    for launch in (0, 700):
        pkg.tune("unitig_launch", launch)
        for name in ("iid_k12_t1", "long_cycle", "genome_k12_t3", "tailed_cycle", "short_cycle", "k1", "read200_k32", "homopolymer"):
            u, g = built(pkg, orc, name)
            same(pkg, u, g)
            u.free()
        u, g = built(pkg, orc, "genome_k12_t3", t=10 ** 6)                       # no node at all: the directory is written all the same
        assert (u.count, u.nodes) == (0, 0) and u.download()[0].tolist() == [0]
        u.free()
    pkg.tune("unitig_launch", 0)
    pkg.synchronize()
    print("POISON fills=%d bytes=%d" % pkg.pool_poison_stats())
    print("OK")


if __name__ == "__main__":
    main()
