#!/usr/bin/env python3
"""Matching statistics and maximal exact matches on a device-resident index (bwtm_matching_stats_batch, bwtm_mem_batch), next to the only
route the library had before: for every end of a pattern, its suffixes of the prefix that ends there through bwtm_find_batch, longest
first, until one occurs -- one find call per round, round j searching P[j .. e) for every end e that has found nothing yet.

The index holds reads of a shared genome at 30x coverage with 1 % substitutions (the generator behind `bench.py --workload genome`, the
index of the other tools); the patterns are 2^16 of its reads, (a) unchanged, so that every read is one MEM, (b) with 1 % and (c) with
5 % of their symbols substituted; min_length is 1 and 19.  The route before runs on a seeded sample of the patterns (it is quadratic),
timing its find calls alone, and all lengths and ranges must be equal.

    python tools/mem_bench.py [--reads 30000000] [--readlen 100] [--patterns 65536] [--sample 512] [--repeats 5] [--out profiles/mem_bench.json]
    bash tools/build_variant.sh diag "" -DBWTM_DIAGNOSTICS; BWTM_LIB=bwt-merge_amd/_variants/diag.so python tools/mem_bench.py --out profiles/mem_bench_lanes_diag.json
                                                      # a diagnostics build also holds the MEM search with one quad per end (bwtm_tune("mem_kernel", 1)): the filling call is
                                                      # then also run in both forms, alternating, the bytes must be equal, and the times summed over the cases decide which ships

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

CASES = (("a_unchanged", 0.0), ("b_1_percent", 0.01), ("c_5_percent", 0.05))
MIN_LENGTHS = (1, 19)
FORMS = {0: "one_quad_per_pattern", 1: "one_quad_per_end"}          # values of the mem_kernel knob of a diagnostics build; the product has form 0 only


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": len(times)}


def substituted(np, rng, reads, rate):
    """The reads with `rate` of their symbols 1..4 replaced by another of 1..4."""
    out = reads.copy()
    hit = (rng.random(reads.shape) < rate) & (reads >= 1) & (reads <= 4)
    shift = rng.integers(1, 4, size=reads.shape).astype(np.uint8)
    out[hit] = (reads[hit] - 1 + shift[hit]) % 4 + 1
    return out, int(hit.sum())


def route_before(pkg, np, ix, patterns, repeats):
    """(lengths, sp, count) [S, m] of the sample by rounds of bwtm_find_batch, and the time of its find calls alone (the median of `repeats`
    runs of the whole route after one warm-up run)."""
    lib, p_u64, p_u8 = pkg.capi.lib(), pkg.capi.p_u64, pkg.capi.p_u8
    S, m = patterns.shape
    flat = np.ascontiguousarray(patterns).reshape(-1)

    def run():
        lengths = np.zeros((S, m), dtype=np.uint32); sp = np.zeros((S, m), dtype=np.uint64); cnt = np.zeros((S, m), dtype=np.uint64)
        todo = np.ones((S, m), dtype=bool)                                    # [k, e - 1]: end e of pattern k has found nothing yet
        spent, searches, calls = 0.0, 0, 0
        for j in range(m):
            ks, es = np.nonzero(todo[:, j:])
            if ks.size == 0:
                break
            ends = es + j + 1
            lens = (ends - j).astype(np.int64)
            offsets = np.zeros(ks.size + 1, dtype=np.uint64)
            offsets[1:] = np.cumsum(lens)
            total = int(offsets[-1])
            idx = np.repeat(ks * m + j, lens) + (np.arange(total) - np.repeat(offsets[:-1].astype(np.int64), lens))
            text = np.ascontiguousarray(flat[idx])
            fsp = np.zeros(ks.size, dtype=np.uint64); fep = np.zeros(ks.size, dtype=np.uint64)
            t0 = time.perf_counter()
            pkg.capi.check(lib.bwtm_find_batch(ix.h, text.ctypes.data_as(p_u8), offsets.ctypes.data_as(p_u64), ks.size, fsp.ctypes.data_as(p_u64), fep.ctypes.data_as(p_u64)))
            spent += (time.perf_counter() - t0) * 1e3
            searches += ks.size; calls += 1
            ok = (fsp <= fep) & (fep < np.uint64(ix.bases))
            lengths[ks[ok], ends[ok] - 1] = lens[ok]; sp[ks[ok], ends[ok] - 1] = fsp[ok]; cnt[ks[ok], ends[ok] - 1] = fep[ok] - fsp[ok] + np.uint64(1)
            todo[ks[ok], ends[ok] - 1] = False
            todo[:, j] = False                                                # end j + 1 has tried its only suffixes
        return lengths, sp, cnt, spent, searches, calls

    run()
    runs = [run() for _ in range(repeats)]
    lengths, sp, cnt, _, searches, calls = runs[0]
    return lengths, sp, cnt, summary([r[3] for r in runs]), searches, calls


def run_case(pkg, np, ix, patterns, name, rate, changed, args):
    lib, p_u64, p_u32, p_u8 = pkg.capi.lib(), pkg.capi.p_u64, pkg.capi.p_u32, pkg.capi.p_u8
    count, m = patterns.shape
    text = np.ascontiguousarray(patterns).reshape(-1)
    offsets = np.arange(count + 1, dtype=np.uint64) * np.uint64(m)
    tp, op = text.ctypes.data_as(p_u8), offsets.ctypes.data_as(p_u64)
    out = {"case": name, "substitution_rate": rate, "symbols_changed": changed, "patterns": count, "m": m}

    # matching statistics
    lengths = np.zeros(count * m, dtype=np.uint32); sp = np.zeros(count * m, dtype=np.uint64); cnt = np.zeros(count * m, dtype=np.uint64)

    def stats_call():
        t0 = time.perf_counter()
        pkg.capi.check(lib.bwtm_matching_stats_batch(ix.h, tp, op, count, lengths.ctypes.data_as(p_u32), sp.ctypes.data_as(p_u64), cnt.ctypes.data_as(p_u64)))
        return (time.perf_counter() - t0) * 1e3

    stats_call()
    st = pkg.mem_stats()
    walls = [stats_call() for _ in range(args.repeats)]
    out["matching_stats"] = {"call": summary(walls), "ns_per_pattern": statistics.median(walls) * 1e6 / count, "lf_steps_per_pattern": st["steps"] / count,
                             "tasks": st["tasks"], "mean_length": float(lengths.mean())}

    # MEMs
    hit_offsets = np.zeros(count + 1, dtype=np.uint64)
    results = {}
    out["mems"] = []
    for min_length in MIN_LENGTHS:
        def call(arrays, capacity):
            ptrs = [a.ctypes.data_as(p_u32 if a.dtype == np.uint32 else p_u64) for a in arrays] if arrays else [None] * 4
            t0 = time.perf_counter()
            pkg.capi.check(lib.bwtm_mem_batch(ix.h, tp, op, count, min_length, hit_offsets.ctypes.data_as(p_u64), ptrs[0], ptrs[1], ptrs[2], ptrs[3], capacity))
            return (time.perf_counter() - t0) * 1e3

        sizing = [call(None, 0)]
        total = int(hit_offsets[-1])
        arrays = [np.zeros(total, dtype=np.uint32), np.zeros(total, dtype=np.uint32), np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.uint64)]
        call(arrays, total)
        st = pkg.mem_stats()
        fills = [call(arrays, total) for _ in range(args.repeats)]
        sizing = [call(None, 0) for _ in range(args.repeats)]
        pkg.profile_reset(); pkg.profile_enable(True)
        wall = call(arrays, total)
        prof = pkg.profile_read()
        pkg.profile_enable(False)
        mine = {k: {"total_ms": round(v[0], 3), "launches": v[1]} for k, v in prof.items() if k.startswith("mem_") or k.startswith("ms_") or k.startswith("scan_")}
        results[min_length] = (hit_offsets.copy(), [a.copy() for a in arrays])
        out["mems"].append({"min_length": min_length, "mems": total, "mems_per_pattern": total / count, "mems_before_min_length_per_pattern": st["mems"] / count,
                            "lf_steps_per_pattern": st["steps"] / count, "fill_call": summary(fills), "sizing_call": summary(sizing),
                            "ns_per_pattern": statistics.median(fills) * 1e6 / count, "kernels_ms": mine, "profiled_call_ms": wall})
        # the MEMs against the matching statistics of the other call: the rule, on the host
        L = lengths.reshape(count, m).astype(np.int64)
        flag = (L >= min_length) & np.concatenate([L[:, 1:] <= L[:, :-1], np.ones((count, 1), dtype=bool)], axis=1)
        ks, es = np.nonzero(flag)
        assert total == ks.size and np.array_equal(np.diff(hit_offsets.astype(np.int64)), flag.sum(axis=1))
        assert np.array_equal(arrays[1], L[ks, es].astype(np.uint32)) and np.array_equal(arrays[0], (es + 1 - L[ks, es]).astype(np.uint32))
        assert np.array_equal(arrays[2], sp.reshape(count, m)[ks, es]) and np.array_equal(arrays[3], cnt.reshape(count, m)[ks, es])
    if rate == 0.0:
        assert np.all(np.diff(results[1][0]) == 1) and np.all(results[1][1][1] == m) and not results[1][1][0].any(), "an unchanged read is one MEM"

    # the route before, on a sample
    rng = np.random.default_rng(17)
    picks = np.sort(rng.choice(count, size=min(args.sample, count), replace=False))
    r_len, r_sp, r_cnt, r_time, searches, calls = route_before(pkg, np, ix, patterns[picks], args.repeats)
    mine_len = lengths.reshape(count, m)[picks]; mine_sp = sp.reshape(count, m)[picks]; mine_cnt = cnt.reshape(count, m)[picks]
    assert np.array_equal(r_len, mine_len) and np.array_equal(r_sp, mine_sp) and np.array_equal(r_cnt, mine_cnt), "%s: the route before disagrees" % name
    before_ns = r_time["median_ms"] * 1e6 / picks.size
    out["route_before"] = {"sample_patterns": int(picks.size), "find_batch_calls": calls, "searches": searches, "searches_per_pattern": searches / picks.size,
                           "lengths_and_ranges_equal": True, "find_batch_time": r_time, "ns_per_pattern": before_ns,
                           "over_matching_stats": before_ns / out["matching_stats"]["ns_per_pattern"],
                           "over_mem_batch": {str(e["min_length"]): before_ns / e["ns_per_pattern"] for e in out["mems"]}}

    # the two forms of the search, alternating (a diagnostics build only)
    if len(args.forms) > 1:
        ab = {}
        for min_length in MIN_LENGTHS:
            want_off, want = results[min_length]
            total = int(want_off[-1])
            arrays = [np.zeros_like(a) for a in want]
            ptrs = [a.ctypes.data_as(p_u32 if a.dtype == np.uint32 else p_u64) for a in arrays]

            def call():
                t0 = time.perf_counter()
                pkg.capi.check(lib.bwtm_mem_batch(ix.h, tp, op, count, min_length, hit_offsets.ctypes.data_as(p_u64), ptrs[0], ptrs[1], ptrs[2], ptrs[3], total))
                return (time.perf_counter() - t0) * 1e3

            entry = {}
            for form in args.forms:                                           # the warm-up, and the same bytes from both
                pkg.tune("mem_kernel", form)
                for a in arrays:
                    a[:] = 0
                hit_offsets[:] = 0
                call()
                assert np.array_equal(hit_offsets, want_off) and all(a.tobytes() == b.tobytes() for a, b in zip(arrays, want)), "%s, min_length %d: the forms disagree" % (name, min_length)
                entry[FORMS[form]] = {"same_bytes": True, "lf_steps_per_pattern": pkg.mem_stats()["steps"] / count}
            walls = {form: [] for form in args.forms}
            for _ in range(args.repeats):
                for form in args.forms:
                    pkg.tune("mem_kernel", form)
                    walls[form].append(call())
            for form in args.forms:
                entry[FORMS[form]]["fill_call"] = summary(walls[form])
            ab[str(min_length)] = entry
        pkg.tune("mem_kernel", 0)
        out["forms_ab"] = ab
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=30_000_000)
    ap.add_argument("--readlen", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--patterns", type=int, default=1 << 16)
    ap.add_argument("--sample", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import _pkg
    pkg = _pkg.load()
    from bwt_merge_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("mem_bench: no GPU (a CPU run cannot time this)")
    torch.cuda.set_device(0); pkg.init(0)
    try:
        pkg.tune("mem_kernel", 0)                             # an unknown key on a product build: raises
        args.forms = (0, 1)
    except pkg.BwtmError:
        args.forms = (0,)
    t0 = time.perf_counter()
    ix = synth.build_index(pkg, args.seed, args.reads, args.readlen, device=torch.device("cuda", 0), workload="genome")
    pkg.synchronize()
    torch.cuda.empty_cache()
    result = {"reads": args.reads, "readlen": args.readlen, "workload": "genome, 30x coverage, 1 % substitutions", "device": torch.cuda.get_device_name(0),
              "library": os.path.basename(pkg.capi.LIB_PATH), "forms": [FORMS[f] for f in args.forms], "index_build_s": round(time.perf_counter() - t0, 2), "bases": ix.bases, "cases": []}
    assert ix.sequences == args.reads and ix.bases == args.reads * (args.readlen + 1)
    rng = np.random.default_rng(5)
    ids = rng.choice(args.reads, size=args.patterns, replace=False).astype(np.uint64)
    roff, rtext = ix.extract_sequences(ids=ids, max_len=args.readlen)
    assert np.all(np.diff(roff) == args.readlen)
    reads = rtext.reshape(args.patterns, args.readlen)
    for name, rate in CASES:
        patterns, changed = substituted(np, rng, reads, rate)
        result["cases"].append(run_case(pkg, np, ix, patterns, name, rate, changed, args))
    if len(args.forms) > 1:
        sums = {FORMS[f]: sum(c["forms_ab"][str(ml)][FORMS[f]]["fill_call"]["median_ms"] for c in result["cases"] for ml in MIN_LENGTHS) for f in args.forms}
        result["decision"] = {"sum_of_median_fill_calls_ms": sums, "ships": min(sums, key=sums.get)}
    ix.free()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
