#!/usr/bin/env python3
"""The distinct k-mers of a device-resident index with their counts (Index.kmers, bwtm_kmers_create), next to the only way the library had
to produce such counts before: bwtm_find_batch over k-mers the caller already holds -- k LF steps per k-mer on walks that share nothing,
after the caller has brought the reads to the host, cut them up and removed the duplicates (none of which is timed here).

The index holds reads of a shared genome at 30x coverage with 1 % substitutions (the generator behind `bench.py --workload genome`, the
index of tools/overlap_bench.py).  A seeded sample of the returned k-mers (1 024 slices of 1 024 consecutive entries,
shuffled: a caller's k-mers come in no particular order) is then searched with bwtm_find_batch: every range must be [sp, sp + count - 1].

    python tools/kmer_bench.py [--reads 30000000] [--readlen 100] [--ks 21,31] [--min-counts 1,2] [--sample 1048576] [--repeats 5] [--out profiles/kmer_bench.json]
    bash tools/build_variant.sh diag "" -DBWTM_DIAGNOSTICS; BWTM_LIB=bwt-merge_amd/_variants/diag.so python tools/kmer_bench.py --out profiles/kmer_bench_lanes_diag.json
                                                      # a diagnostics build also holds the level kernels with four lanes per trie node (bwtm_tune("kmers_kernel", 1)): the call is
                                                      # then run in both forms, alternating, so that the two share whatever else the machine is doing: the A/B of DESIGN 3.10

Times are host clocks around calls that end in a stream synchronise (bwtm_kmers_create; bwtm_find_batch), medians of `--repeats` runs after one warm-up run of
the same shape, with the fastest and the slowest run next to them; kernel times are the library's own events in a run of their own.
Needs a GPU; prints one JSON object and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = {0: "one_lane_per_node", 1: "four_lanes_per_node"}        # values of the kmers_kernel knob of a diagnostics build; the product has form 0 only


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": len(times)}


def run_config(pkg, np, ix, k, min_count, args):
    lib, p_u64, p_u8 = pkg.capi.lib(), pkg.capi.p_u64, pkg.capi.p_u8
    out = {"k": k, "min_count": min_count}

    def create(form):
        if len(args.forms) > 1:
            pkg.tune("kmers_kernel", form)
        t0 = time.perf_counter()
        km = ix.kmers(k, min_count=min_count)                # ends in a synchronise (the total is read back)
        ms = (time.perf_counter() - t0) * 1e3
        return km, ms

    # warm-up of both forms, and the result itself
    for form in args.forms:
        km, _ = create(form)
        km.free()
    pkg.synchronize()
    pkg.trim()                                               # the peak below is this one call's: what the warm-up left with the pool goes back first
    held = pkg.pool_stats()["held_bytes"]
    pkg.device_bytes_peak(reset=True)
    km, _ = create(0)
    out["peak_bytes"] = pkg.device_bytes_peak()
    out["held_bytes_before"] = held
    levels = km.levels()
    out.update({"distinct": km.distinct, "total": km.total, "result_bytes": km.nbytes, "nodes_per_level": [int(v) for v in levels],
                "largest_level": int(levels.max()), "documented_bound_bytes": 240 * int(levels.max()) + (1 << 20)})
    # the sample, and the existing route on it
    distinct = km.distinct
    if distinct > 0:
        rng = np.random.default_rng(9)
        piece = 1024
        pieces = max(1, min(args.sample // piece, distinct // piece))
        starts = np.sort(rng.choice(max(distinct - piece + 1, 1), size=pieces, replace=False)) if distinct >= piece else np.zeros(1, dtype=np.int64)
        piece = min(piece, distinct)
        got = [km.download(int(s), piece) for s in starts.tolist()]
        codes, counts, sp = (np.concatenate([g[j] for g in got]) for j in range(3))
        order = rng.permutation(codes.size)
        codes, counts, sp = codes[order], counts[order], sp[order]
        text = np.ascontiguousarray(pkg.decode_kmers(codes, k, 5)).reshape(-1)
        offsets = (np.arange(codes.size + 1, dtype=np.uint64) * np.uint64(k))
        fsp = np.zeros(codes.size, dtype=np.uint64); fep = np.zeros(codes.size, dtype=np.uint64)

        def find():
            pkg.capi.check(lib.bwtm_find_batch(ix.h, text.ctypes.data_as(p_u8), offsets.ctypes.data_as(p_u64), codes.size, fsp.ctypes.data_as(p_u64), fep.ctypes.data_as(p_u64)))

        find()
        agree = bool(np.array_equal(fsp, sp) and np.array_equal(fep, sp + counts - np.uint64(1)))
        assert agree, "bwtm_find_batch and the k-mer list disagree on %d of %d ranges" % (int(np.sum((fsp != sp) | (fep != sp + counts - np.uint64(1)))), codes.size)
        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            find()
            times.append((time.perf_counter() - t0) * 1e3)
        out["find_batch"] = {"sample": int(codes.size), "ranges_agree": agree, "call": summary(times), "ns_per_kmer": statistics.median(times) * 1e6 / codes.size}
    km.free()
    # the two forms, alternating
    walls = {form: [] for form in args.forms}
    for form in args.forms:                                  # the pool was trimmed above: every form finds its blocks again
        km, _ = create(form)
        km.free()
    for _ in range(args.repeats):
        for form in args.forms:
            km, ms = create(form)
            km.free()
            walls[form].append(ms)
    for form in args.forms:
        out[FORMS[form]] = {"create_call": summary(walls[form])}
        if distinct > 0:
            out[FORMS[form]]["ns_per_kmer"] = statistics.median(walls[form]) * 1e6 / distinct
    # the kernels alone, from the library's own events (one call of each form)
    for form in args.forms:
        pkg.profile_reset(); pkg.profile_enable(True)
        km, _ = create(form)
        prof = pkg.profile_read()
        pkg.profile_enable(False)
        km.free()
        mine = {name: {"total_ms": round(v[0], 3), "launches": v[1]} for name, v in prof.items() if name.startswith("kmer_") or name.startswith("scan_")}
        out[FORMS[form]]["kernels_ms"] = mine
        out[FORMS[form]]["kernel_ms"] = round(sum(v["total_ms"] for v in mine.values()), 3)
    if distinct > 0 and "find_batch" in out:
        for form in args.forms:
            out[FORMS[form]]["find_batch_ns_over_kmers_ns"] = out["find_batch"]["ns_per_kmer"] / out[FORMS[form]]["ns_per_kmer"]
    if len(args.forms) > 1:
        pkg.tune("kmers_kernel", 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=30_000_000)
    ap.add_argument("--readlen", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--min-counts", default="1,2")
    ap.add_argument("--sample", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import _pkg
    pkg = _pkg.load()
    from bwt_merge_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("kmer_bench: no GPU (a CPU run cannot time this)")
    torch.cuda.set_device(0); pkg.init(0)
    try:
        pkg.tune("kmers_kernel", 0)                           # an unknown key on a product build: raises
        args.forms = (0, 1)
    except pkg.BwtmError:
        args.forms = (0,)
    t0 = time.perf_counter()
    ix = synth.build_index(pkg, args.seed, args.reads, args.readlen, device=torch.device("cuda", 0), workload="genome")
    pkg.synchronize()
    torch.cuda.empty_cache()
    result = {"reads": args.reads, "readlen": args.readlen, "workload": "genome, 30x coverage, 1 % substitutions", "device": torch.cuda.get_device_name(0),
              "library": os.path.basename(pkg.capi.LIB_PATH), "forms": [FORMS[f] for f in args.forms], "index_build_s": round(time.perf_counter() - t0, 2), "bases": ix.bases, "configs": []}
    assert ix.sequences == args.reads and ix.bases == args.reads * (args.readlen + 1)
    for k in (int(v) for v in args.ks.split(",")):
        for min_count in (int(v) for v in args.min_counts.split(",")):
            result["configs"].append(run_config(pkg, np, ix, k, min_count, args))
            print("k = %d, min_count = %d done" % (k, min_count), file=sys.stderr, flush=True)
    ix.free()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
