#!/usr/bin/env python3
"""Reads out of a device-resident index, two ways over the same ids: Index.sequences (bwtm_sequences_extract: two kernels per batch, four
lanes per sequence) and synth.extract_sequences_matrix (one bwtm_inverse_select_batch call per base, driven from Python: the only way
there was before).  Both results are compared with the generator's reads before anything is timed.

    python tools/extract_reads_bench.py [--reads 30000000] [--readlen 100] [--repeats 7] [--loop-repeats 3] [--out profiles/NAME.json]

Times are host clocks around calls that end in a stream synchronise (both paths return host arrays), medians of `--repeats` runs after
one warm-up run of the same shape; the id sets are 10 000 random ids (bench.py's --verify-reads) and 2^20 contiguous ids.  The Python loop
takes seconds on the large set, so it gets `--loop-repeats` runs.  Needs a GPU; prints one JSON object and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats):
    fn()                                                     # warm-up: code objects, pool blocks of this shape
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=30_000_000)
    ap.add_argument("--readlen", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import _pkg
    pkg = _pkg.load()
    from bwt_merge_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("extract_reads_bench: no GPU (a CPU run cannot time this)")
    torch.cuda.set_device(0); pkg.init(0)
    n, L = args.reads, args.readlen
    t0 = time.perf_counter()
    ix = synth.build_index(pkg, args.seed, n, L, device=torch.device("cuda", 0))
    pkg.synchronize()
    build_s = time.perf_counter() - t0
    assert ix.sequences == n and ix.bases == n * (L + 1)
    id_sets = {"random_10000": np.sort(np.random.default_rng(5).integers(0, n, 10_000)).astype(np.uint64),
               "contiguous_2^20": np.arange(n // 3, n // 3 + min(1 << 20, n - n // 3), dtype=np.uint64)}
    result = {"reads": n, "readlen": L, "bases": ix.bases, "build_s": round(build_s, 2), "device": torch.cuda.get_device_name(0), "sets": {}}
    for name, ids in id_sets.items():
        contiguous = name.startswith("contiguous")
        want = synth.reads_matrix("iid", args.seed, ids, L, n, L)

        def new_way():
            if contiguous:
                return ix.sequences(first=int(ids[0]), count=ids.size, max_len=L)
            return ix.sequences(ids=ids, max_len=L)

        def old_way():
            return synth.extract_sequences_matrix(ix, ids, max_len=L + 2)

        offsets, text = new_way()
        assert np.array_equal(offsets, np.arange(ids.size + 1, dtype=np.uint64) * np.uint64(L)) and np.array_equal(text.reshape(ids.size, L), want), name
        assert np.array_equal(old_way()[:, :L], want), name
        new_t = timed(new_way, args.repeats)
        old_t = timed(old_way, args.loop_repeats)
        bases = int(ids.size) * L
        result["sets"][name] = {"ids": int(ids.size), "bases": bases, "sequences_call": new_t, "python_loop": old_t,
                                "sequences_call_gbases_per_s": bases / new_t["median_ms"] / 1e6, "python_loop_gbases_per_s": bases / old_t["median_ms"] / 1e6,
                                "speedup": old_t["median_ms"] / new_t["median_ms"]}
    # the kernels alone, from the library's own events, for the contiguous set
    ids = id_sets["contiguous_2^20"]
    pkg.profile_reset(); pkg.profile_enable(True)
    ix.sequences(first=int(ids[0]), count=ids.size, max_len=L)
    prof = pkg.profile_read()
    pkg.profile_enable(False)
    result["kernels_contiguous_2^20_ms"] = {k: {"total_ms": round(v[0], 3), "launches": v[1]} for k, v in prof.items() if k.startswith("seq_")}
    ix.free()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
