"""The mixed-length case of tests/test_gpu_find_edit.py in a process of its own (not a test module): the child that test_on_a_poisoned_pool
starts with BWTM_POOL_POISON in its environment, which the library reads once per process.  Twice, with the other collection in between, so
that the later runs' blocks are recycled ones; in batches of 7 as well, whose frontiers and hit streams shrink and grow from batch to batch.
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
    from edit_inputs import collection, mixed_budget, mixed_expected, mixed_patterns
    from test_gpu_find_edit import same, uploaded
    pkg = _pkg.load()
    pkg.init(0)
    x, g = uploaded(pkg, orc, collection("iid").rows), uploaded(pkg, orc, collection("genome").rows)
    for again in range(2):                                                       # the second round's blocks are the first one's, given back
        same(x.find_edit(mixed_budget(mixed_patterns("iid"), 3), 3), mixed_expected("iid", 3))
        same(g.find_edit(mixed_patterns("genome"), 2), mixed_expected("genome", 2))
        pkg.tune("approx_batch", 7)
        same(x.find_edit(mixed_patterns("iid"), 1), mixed_expected("iid", 1))
        pkg.tune("approx_batch", 0)
    pkg.synchronize()
    print("POISON fills=%d bytes=%d" % pkg.pool_poison_stats())
    print("OK")


if __name__ == "__main__":
    main()
