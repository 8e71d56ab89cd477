#!/usr/bin/env python3
"""Patterns with up to d substitutions on a device-resident index (Index.find_approx, bwtm_find_approx_batch), next to the only route the
library had before: every Hamming neighbour of a pattern enumerated on the host, all of them searched with bwtm_find_batch, the non-empty
ranges kept.  That route searches 401 strings for a 100-mer at one mismatch and 79 601 at two, each from scratch.

The index holds reads of a shared genome at 30x coverage with 1 % substitutions (the generator behind `bench.py --workload genome`, the
index of tools/kmer_bench.py).  The patterns are 2^16 windows of 32 and of 100 symbols cut from reads taken out of the index, searched at
d = 0, 1, 2 and, the 32-mers, d = 3 (in batches of 2^14 patterns at d = 3: the frontier of 2^16 of them is larger than it needs to be held).
The partner runs on a seeded sample of the patterns, small enough to finish; only its bwtm_find_batch calls are timed (not the enumeration),
and the hits of every pattern of the sample must be the same set, in the same order once the partner's are sorted by the reversed string.

    python tools/approx_bench.py [--reads 30000000] [--readlen 100] [--patterns 65536] [--repeats 5] [--out profiles/approx_bench.json]
    bash tools/build_variant.sh diag "" -DBWTM_DIAGNOSTICS; BWTM_LIB=bwt-merge_amd/_variants/diag.so python tools/approx_bench.py --out profiles/approx_bench_lanes_diag.json
                                                      # a diagnostics build also holds the level kernels with four lanes per node (bwtm_tune("approx_kernel", 1)): the filling call
                                                      # is then also run in both forms, alternating, so that the two share whatever else the machine is doing: the A/B of DESIGN 3.11

Times are host clocks around one filling call (the search and the gather; its capacity comes from a sizing call before, which is reported
too), medians of `--repeats` runs after one warm-up run of the same shape, with the fastest and the slowest run next to them; kernel times are
the library's own events in a run of their own, and the host-side share is what of the call's time they leave (one read-back per level, the
launches).  Needs a GPU; prints one JSON object and writes it to --out."""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ((32, 0), (32, 1), (32, 2), (32, 3), (100, 0), (100, 1), (100, 2))
SAMPLE = {(32, 0): 4096, (32, 1): 1024, (32, 2): 64, (32, 3): 4, (100, 0): 4096, (100, 1): 256, (100, 2): 16}      # patterns the partner searches
FORMS = {0: "one_lane_per_node", 1: "four_lanes_per_node"}        # values of the approx_kernel knob of a diagnostics build; the product has form 0 only
BATCH = {3: 1 << 14}                                                                                               # approx_batch per d; the default otherwise


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": len(times)}


def neighbours(np, p, d):
    """(strings [N, m], distance [N]) of every string within Hamming distance d of p over the comp values 1..5, p itself first."""
    m = p.size
    rows, dist = [p[None, :].copy()], [np.zeros(1, dtype=np.uint8)]
    for e in range(1, d + 1):
        places = np.array(list(itertools.combinations(range(m), e)), dtype=np.int64)                    # [C, e]
        shifts = np.array(list(itertools.product(range(1, 5), repeat=e)), dtype=np.uint8)              # [4^e, e]
        block = np.tile(p, (places.shape[0], shifts.shape[0], 1))
        for j in range(e):
            old = p[places[:, j]][:, None]
            block[np.arange(places.shape[0])[:, None], np.arange(shifts.shape[0])[None, :], places[:, j][:, None]] = (old - 1 + shifts[None, :, j]) % 5 + 1
        rows.append(block.reshape(-1, m)); dist.append(np.full(places.shape[0] * shifts.shape[0], e, dtype=np.uint8))
    return np.concatenate(rows), np.concatenate(dist)


def run_config(pkg, np, ix, patterns, m, d, args):
    lib, p_u64, p_u8 = pkg.capi.lib(), pkg.capi.p_u64, pkg.capi.p_u8
    count = patterns.shape[0]
    text = np.ascontiguousarray(patterns).reshape(-1)
    offsets = np.arange(count + 1, dtype=np.uint64) * np.uint64(m)
    hit_offsets = np.zeros(count + 1, dtype=np.uint64)
    out = {"m": m, "d": d, "patterns": count, "approx_batch": BATCH.get(d, 1 << 16)}
    pkg.tune("approx_batch", BATCH.get(d, 0))

    def call(sp, cnt, mm, capacity):
        t0 = time.perf_counter()
        pkg.capi.check(lib.bwtm_find_approx_batch(ix.h, text.ctypes.data_as(p_u8), offsets.ctypes.data_as(p_u64), count, d, 0, hit_offsets.ctypes.data_as(p_u64),
                                                  sp.ctypes.data_as(p_u64) if sp is not None else None, cnt.ctypes.data_as(p_u64) if cnt is not None else None,
                                                  mm.ctypes.data_as(p_u8) if mm is not None else None, capacity))
        return (time.perf_counter() - t0) * 1e3

    pkg.synchronize(); pkg.trim()
    held = pkg.pool_stats()["held_bytes"]
    pkg.device_bytes_peak(reset=True)
    sizing = [call(None, None, None, 0)]                                                                # the warm-up as well
    total = int(hit_offsets[-1])
    sp, cnt, mm = np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.uint8)
    call(sp, cnt, mm, total)
    stats = pkg.find_approx_stats()
    P, H = stats["frontier_peak"], stats["batch_hits"]
    out.update({"hits": total, "hits_per_pattern": total / count, "patterns_with_hits": int((np.diff(hit_offsets) > 0).sum()),
                "nodes_expanded": stats["expanded"], "nodes_expanded_per_pattern": stats["expanded"] / count, "frontier_peak_nodes": P, "levels": stats["levels"],
                "peak_bytes_beyond_held": pkg.device_bytes_peak() - held,
                "documented_bound_bytes_per_call": 240 * P + 128 * H + 2 * min(count, out["approx_batch"]) * m + (1 << 20)})
    walls = [call(sp, cnt, mm, total) for _ in range(args.repeats)]
    sizing += [call(None, None, None, 0) for _ in range(args.repeats)]
    out["fill_call"] = summary(walls)
    out["sizing_call"] = summary(sizing[1:])
    out["ns_per_pattern"] = statistics.median(walls) * 1e6 / count
    # the kernels alone, from the library's own events (one filling call)
    pkg.profile_reset(); pkg.profile_enable(True)
    wall = call(sp, cnt, mm, total)
    prof = pkg.profile_read()
    pkg.profile_enable(False)
    mine = {name: {"total_ms": round(v[0], 3), "launches": v[1]} for name, v in prof.items() if name.startswith("approx_") or name.startswith("scan_")}
    out["kernels_ms"] = mine
    out["kernel_ms"] = round(sum(v["total_ms"] for v in mine.values()), 3)
    out["profiled_call_ms"] = wall
    out["host_side_share"] = 1.0 - out["kernel_ms"] / wall if wall > 0 else None                        # of the profiled call: its events cost host time too
    # the partner: all neighbours of a seeded sample, through bwtm_find_batch
    rng = np.random.default_rng(17)
    picks = np.sort(rng.choice(count, size=min(SAMPLE[(m, d)], count), replace=False))
    strings, dist, owner = [], [], []
    for j, k in enumerate(picks.tolist()):
        s, e = neighbours(np, patterns[k], d)
        strings.append(s); dist.append(e); owner.append(np.full(e.size, j, dtype=np.int64))
    strings, dist, owner = np.concatenate(strings), np.concatenate(dist), np.concatenate(owner)
    ntext = np.ascontiguousarray(strings).reshape(-1)
    noff = np.arange(strings.shape[0] + 1, dtype=np.uint64) * np.uint64(m)
    fsp, fep = np.zeros(strings.shape[0], dtype=np.uint64), np.zeros(strings.shape[0], dtype=np.uint64)

    def find():
        t0 = time.perf_counter()
        pkg.capi.check(lib.bwtm_find_batch(ix.h, ntext.ctypes.data_as(p_u8), noff.ctypes.data_as(p_u64), strings.shape[0], fsp.ctypes.data_as(p_u64), fep.ctypes.data_as(p_u64)))
        return (time.perf_counter() - t0) * 1e3

    find()
    times = [find() for _ in range(args.repeats)]
    found = (fsp <= fep) & (fep < np.uint64(ix.bases))
    equal = 0
    for j, k in enumerate(picks.tolist()):
        sel = np.flatnonzero(found & (owner == j))
        order = np.lexsort(strings[sel].T)                                                              # by the reversed string: the documented order
        sel = sel[order]
        a, b = int(hit_offsets[k]), int(hit_offsets[k + 1])
        same = (b - a == sel.size and np.array_equal(sp[a:b], fsp[sel]) and np.array_equal(sp[a:b] + cnt[a:b] - np.uint64(1), fep[sel]) and np.array_equal(mm[a:b], dist[sel]))
        assert same, "m = %d, d = %d: the hits of pattern %d differ from those of its %d neighbours" % (m, d, k, int((owner == j).sum()))
        equal += 1
    out["enumeration"] = {"sample_patterns": int(picks.size), "searches": int(strings.shape[0]), "searches_per_pattern": strings.shape[0] / picks.size,
                          "hit_sets_equal": equal, "find_batch_calls": summary(times), "ns_per_pattern": statistics.median(times) * 1e6 / picks.size}
    out["enumeration_ns_over_approx_ns"] = out["enumeration"]["ns_per_pattern"] / out["ns_per_pattern"]
    # the two forms of the level kernels, alternating (a diagnostics build only)
    if len(args.forms) > 1:
        sp2, cnt2, mm2 = np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.uint8)
        ab = {FORMS[form]: {} for form in args.forms}
        for form in args.forms:                                                                         # the warm-up, and the same arrays from both
            pkg.tune("approx_kernel", form)
            sp2[:] = 0; cnt2[:] = 0; mm2[:] = 0
            call(sp2, cnt2, mm2, total)
            assert np.array_equal(sp2, sp) and np.array_equal(cnt2, cnt) and np.array_equal(mm2, mm), "m = %d, d = %d: the forms disagree" % (m, d)
            ab[FORMS[form]]["same_arrays"] = True
        walls = {form: [] for form in args.forms}
        for _ in range(args.repeats):
            for form in args.forms:
                pkg.tune("approx_kernel", form)
                walls[form].append(call(sp2, cnt2, mm2, total))
        for form in args.forms:
            pkg.tune("approx_kernel", form)
            pkg.profile_reset(); pkg.profile_enable(True)
            call(sp2, cnt2, mm2, total)
            prof = pkg.profile_read()
            pkg.profile_enable(False)
            mine = {name: round(v[0], 3) for name, v in prof.items() if name.startswith("approx_") or name.startswith("scan_")}
            ab[FORMS[form]].update({"fill_call": summary(walls[form]), "kernels_ms": mine, "kernel_ms": round(sum(mine.values()), 3)})
        pkg.tune("approx_kernel", 0)
        out["lanes_ab"] = ab
    pkg.tune("approx_batch", 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=30_000_000)
    ap.add_argument("--readlen", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--patterns", type=int, default=1 << 16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default=",".join("%d:%d" % c for c in CONFIGS), help="m:d pairs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import _pkg
    pkg = _pkg.load()
    from bwt_merge_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("approx_bench: no GPU (a CPU run cannot time this)")
    torch.cuda.set_device(0); pkg.init(0)
    try:
        pkg.tune("approx_kernel", 0)                          # an unknown key on a product build: raises
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
    rng = np.random.default_rng(5)
    ids = rng.choice(args.reads, size=args.patterns, replace=False).astype(np.uint64)
    roff, rtext = ix.extract_sequences(ids=ids, max_len=args.readlen)
    assert np.all(np.diff(roff) == args.readlen)
    reads = rtext.reshape(args.patterns, args.readlen)
    for m, d in (tuple(int(v) for v in c.split(":")) for c in args.configs.split(",")):
        assert (m, d) in SAMPLE and m <= args.readlen
        starts = rng.integers(0, args.readlen - m + 1, size=args.patterns)
        patterns = np.ascontiguousarray(reads[np.arange(args.patterns)[:, None], starts[:, None] + np.arange(m)[None, :]])
        result["configs"].append(run_config(pkg, np, ix, patterns, m, d, args))
        print("m = %d, d = %d done" % (m, d), file=sys.stderr, flush=True)
    ix.free()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
