#!/usr/bin/env python3
"""Suffix-prefix overlaps on a device-resident index (Locator.overlaps, bwtm_overlap_sequences), next to the only way the library had to
produce the same hit counts before: bwtm_find_batch over the patterns (0, suffix) for every suffix of at least min_overlap symbols of a
read -- with the endmarker 0 in front, ep - sp + 1 of that pattern is the number of reads that start with the suffix.  That composition
costs sum(l + 1 for l in min_overlap .. L) LF steps per read against L, about 47 times more for 100 bp reads and min_overlap 30, and ends at
BWT ranges, not at read numbers.

The index holds reads of a shared genome at 30x coverage with 1 % substitutions (the generator behind `bench.py --workload genome`), so
reads do overlap; iid reads, which almost never do, are run as the "no hits" case.  Before anything is timed, the two ways are compared
on every (query, length) count of a sample of the queries.

    python tools/overlap_bench.py [--reads 30000000] [--readlen 100] [--queries 1048576] [--sample 10000] [--min-overlap 30] [--repeats 7] [--out profiles/NAME.json]
    bash tools/build_variant.sh diag "" -DBWTM_DIAGNOSTICS; BWTM_LIB=bwt-merge_amd/_variants/diag.so python tools/overlap_bench.py --kernel 1 --workloads genome
                                                      # the same search with one lane per query (k_find_batch's shape): the A/B of DESIGN 3.9

Times are host clocks around calls that end in a stream synchronise, medians of `--repeats` runs after one warm-up run of the same
shape, with the fastest and the slowest run next to them.  Needs a GPU; prints one JSON object and writes it to --out."""
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


def run_workload(pkg, synth, np, torch, args, workload, compose):
    n, L, tau, Q = args.reads, args.readlen, args.min_overlap, min(args.queries, args.reads)
    lib, p_u64, p_u8 = pkg.capi.lib(), pkg.capi.p_u64, pkg.capi.p_u8
    t0 = time.perf_counter()
    ix = synth.build_index(pkg, args.seed, n, L, device=torch.device("cuda", 0), workload=workload)
    pkg.synchronize()
    out = {"index_build_s": round(time.perf_counter() - t0, 2), "bases": ix.bases}
    assert ix.sequences == n and ix.bases == n * (L + 1)
    loc = ix.locator(max_len=L)
    first = (n - Q) // 2                                      # 2^20 contiguous ids from the middle of the collection
    hit_offsets = np.zeros(Q + 1, dtype=np.uint64)

    def sizing_call():
        pkg.capi.check(lib.bwtm_overlap_sequences(loc.h, None, first, Q, tau, 0, hit_offsets.ctypes.data_as(p_u64), None, None, 0))

    sizing_call()
    total = int(hit_offsets[-1])
    ids = np.zeros(max(total, 1), dtype=np.uint64)
    lengths = np.zeros(max(total, 1), dtype=np.uint64)

    def full_call():
        pkg.capi.check(lib.bwtm_overlap_sequences(loc.h, None, first, Q, tau, 0, hit_offsets.ctypes.data_as(p_u64), ids.ctypes.data_as(p_u64), lengths.ctypes.data_as(p_u64), ids.size))

    full_call()
    per_query = np.diff(hit_offsets.astype(np.int64))
    owner = np.repeat(np.arange(Q), per_query)
    # every query finds itself over its whole length, first
    assert np.all(per_query >= 1) and np.all(lengths[hit_offsets[:-1].astype(np.int64)] == L)
    out.update({"queries": Q, "first_id": first, "min_overlap": tau, "hits": total, "hits_per_query": total / Q,
                "hits_other_than_the_query_itself": total - Q})

    if compose:
        # the composition on a sample of the same queries, and the agreement of every (query, length) count
        S = min(args.sample, Q)
        rng = np.random.default_rng(8)
        sample = np.sort(rng.choice(Q, size=S, replace=False))
        rows = synth.reads_matrix(workload, args.seed, first + sample, L, n, L)
        parts, lens = [], []
        for l in range(tau, L + 1):                           # pattern (l - tau) * S + k = (0,) + the last l symbols of sample read k
            block = np.zeros((S, l + 1), dtype=np.uint8)
            block[:, 1:] = rows[:, L - l:]
            parts.append(block.reshape(-1)); lens.append(np.full(S, l + 1, dtype=np.uint64))
        text = np.ascontiguousarray(np.concatenate(parts))
        offsets = np.zeros(S * (L - tau + 1) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(np.concatenate(lens))
        npat = offsets.size - 1
        sp = np.zeros(npat, dtype=np.uint64); ep = np.zeros(npat, dtype=np.uint64)

        def composition():
            pkg.capi.check(lib.bwtm_find_batch(ix.h, text.ctypes.data_as(p_u8), offsets.ctypes.data_as(p_u64), npat, sp.ctypes.data_as(p_u64), ep.ctypes.data_as(p_u64)))

        composition()
        want = np.where(sp <= ep, ep.astype(np.int64) - sp.astype(np.int64) + 1, 0).reshape(L - tau + 1, S).T       # [k, l - tau]
        place = np.full(Q, -1, dtype=np.int64)
        place[sample] = np.arange(S)
        mine = place[owner] >= 0
        got = np.zeros((S, L + 1), dtype=np.int64)
        np.add.at(got, (place[owner][mine], lengths[:total].astype(np.int64)[mine]), 1)
        got = got[:, tau:]
        agree = bool(np.array_equal(got, want))
        assert agree, "the overlap call and the composition of find calls disagree on %d of %d counts" % (int(np.sum(got != want)), got.size)
        sample_ids = (first + sample).astype(np.uint64)
        s_off = np.zeros(S + 1, dtype=np.uint64)
        s_ids = np.zeros(max(int(got.sum()), 1), dtype=np.uint64); s_len = np.zeros_like(s_ids)

        def sample_call():
            pkg.capi.check(lib.bwtm_overlap_sequences(loc.h, sample_ids.ctypes.data_as(p_u64), 0, S, tau, 0, s_off.ctypes.data_as(p_u64), s_ids.ctypes.data_as(p_u64),
                                                      s_len.ctypes.data_as(p_u64), s_ids.size))

        sample_call()
        assert int(s_off[-1]) == int(got.sum())
        t_comp = timed(composition, args.repeats)
        t_sample = timed(sample_call, args.repeats)
        steps_comp = sum(l + 1 for l in range(tau, L + 1))
        out["composition"] = {"sample_queries": S, "patterns": int(npat), "pattern_symbols": int(offsets[-1]), "counts_compared": int(got.size), "counts_agree": agree,
                              "find_batch_call": t_comp, "overlap_call_same_sample": t_sample,
                              "lf_steps_per_query": {"composition": steps_comp, "overlap": L, "ratio": steps_comp / L}}

    t_size = timed(sizing_call, args.repeats)
    t_full = timed(full_call, args.repeats)
    out["sizing_call"] = t_size
    out["full_call"] = t_full
    out["full_call_us_per_query"] = t_full["median_ms"] * 1e3 / Q
    if compose:
        c = out["composition"]
        c["find_batch_us_per_query"] = c["find_batch_call"]["median_ms"] * 1e3 / c["sample_queries"]
        c["overlap_us_per_query_same_sample"] = c["overlap_call_same_sample"]["median_ms"] * 1e3 / c["sample_queries"]
        c["speedup_full_call"] = c["find_batch_us_per_query"] / out["full_call_us_per_query"]
        c["speedup_same_sample"] = c["find_batch_us_per_query"] / c["overlap_us_per_query_same_sample"]
        assert c["speedup_full_call"] > 1.0, "the overlap call is not faster per query than the composition of find calls"

    # the kernels alone, from the library's own events (one full call: count pass, emit pass, expansion)
    pkg.profile_reset(); pkg.profile_enable(True)
    full_call()
    prof = pkg.profile_read()
    pkg.profile_enable(False)
    out["kernels_ms"] = {k: {"total_ms": round(v[0], 3), "launches": v[1]} for k, v in prof.items() if k.startswith("overlap") or k.startswith("seq_")}
    scan = out["kernels_ms"].get("overlap_scan", {}).get("total_ms", 0.0)
    if scan > 0:
        out["scan_g_lf_steps_per_s"] = 2 * Q * L / scan / 1e6          # both passes walk every symbol of every query (an upper bound: a search ends at an empty range)
    loc.free()
    ix.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=30_000_000)
    ap.add_argument("--readlen", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--sample", type=int, default=10_000)
    ap.add_argument("--min-overlap", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernel", type=int, default=0, help="1: one lane per query, the A/B partner of a -DBWTM_DIAGNOSTICS build (BWTM_LIB=...)")
    ap.add_argument("--workloads", default="genome,iid")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import _pkg
    pkg = _pkg.load()
    from bwt_merge_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("overlap_bench: no GPU (a CPU run cannot time this)")
    torch.cuda.set_device(0); pkg.init(0)
    layout = "one quad per query, both rank positions loaded together"
    if args.kernel != 0:
        pkg.tune("overlap_kernel", args.kernel)               # an unknown key on a product build: raises
        layout = "one lane per query (k_find_batch's shape), diagnostics build"
    result = {"reads": args.reads, "readlen": args.readlen, "device": torch.cuda.get_device_name(0), "lane_layout": layout, "library": os.path.basename(pkg.capi.LIB_PATH)}
    if "genome" in args.workloads.split(","):
        result["genome_30x"] = run_workload(pkg, synth, np, torch, args, "genome", True)
    if "iid" in args.workloads.split(","):
        result["iid_no_hits"] = run_workload(pkg, synth, np, torch, args, "iid", False)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
