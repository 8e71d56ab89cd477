"""The long reads (k = 21 and 32) and the hand-made reads of tests/test_gpu_correct.py in a process of its own (not a test module): the child
that test_on_a_poisoned_pool starts with BWTM_POOL_POISON in its environment, which the library reads once per process.  Twice, in one
batch and in batches of 64 reads, so that the later runs' blocks are recycled ones.
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
    from correct_inputs import HAND_K, HAND_T, as_bytes, hand_made
    from test_gpu_correct import long_want, long_reads, same, uploaded
    pkg = _pkg.load()
    pkg.init(0)
    rows = long_reads()[0]
    x = uploaded(pkg, orc, rows)
    collection, cases = hand_made()
    h = uploaded(pkg, orc, collection)
    for batch in (0, 64):
        pkg.tune("correct_batch", batch)
        for k in (21, 32):
            km = x.kmers(k)
            cor = km.corrector(3)
            km.free()
            want, solid = long_want(k)
            assert cor.solid == solid
            same(cor.correct_sequences(x, max_len=300), want)
            same(cor.correct_sequences(x, max_len=300, text=False), want)
            texts, status, edits = cor.correct(rows)
            assert [as_bytes(t) for t in texts] == want[0] and np.array_equal(status, want[1]) and np.array_equal(edits, want[2])
            cor.free()
        cor = h.kmers(HAND_K).corrector(HAND_T)
        for name, read, rounds, wstatus, wtext, wedits in cases:
            texts, status, edits = cor.correct([read], max_rounds=rounds)
            assert (as_bytes(texts[0]), int(status[0]), int(edits[0])) == (wtext, wstatus, wedits), name
        cor.free()
        empty = x.kmers(21, min_count=10 ** 6).corrector(3)                      # no k-mer at all: the directory is written all the same
        assert empty.solid == 0 and set(empty.correct(rows[:40])[1].tolist()) <= {2, 3}
        empty.free()
    pkg.tune("correct_batch", 0)
    pkg.synchronize()
    print("POISON fills=%d bytes=%d" % pkg.pool_poison_stats())
    print("OK")


if __name__ == "__main__":
    main()
