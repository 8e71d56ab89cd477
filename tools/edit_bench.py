#!/usr/bin/env python3
"""Patterns within edit distance e on a device-resident index (Index.find_edit, bwtm_find_edit_batch), next to the bounded-mismatch search
at d = e on the same patterns (bwtm_find_approx_batch: the price of allowing indels) and, at e = 1, next to the only route the library had
before: every string within one edit of a pattern enumerated on the host, all of them searched with bwtm_find_batch, the non-empty ranges kept.

The index holds reads of a shared genome at 30x coverage with 1 % substitutions (the generator behind `bench.py --workload genome`, the
index of tools/approx_bench.py).  The patterns are 2^16 strings of 32 and of 100 symbols cut from reads taken out of the index; every second
one carries one indel (a piece one symbol longer with a symbol deleted, or one symbol shorter with a random symbol inserted), so that half
of the patterns have no exact occurrence of their own length.  32-mers run at e = 0 .. 3, 100-mers at e = 0 .. 2.  A case whose batch does
not fit the device halves bwtm_tune("approx_batch") until it does, and records the value it used.

    python tools/edit_bench.py [--reads 30000000] [--readlen 100] [--patterns 65536] [--repeats 3] [--out profiles/edit_bench.json]

Times are host clocks around one filling call (the search and the gather; its capacity comes from a sizing call before), medians of
`--repeats` runs after one warm-up run of the same shape, the edit and the Hamming call alternating so that the two share whatever else
the machine is doing; kernel times are the library's own events in a run of their own, and the host-side share is what of the call's time
they leave (one read-back per level, the launches).  Every Hamming hit must be among the edit hits, with length == m and edits <=
mismatches; at e = 1 the hits of every pattern of a seeded sample must equal the host enumeration's.  Needs a GPU; prints one JSON object
and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ((32, 0), (32, 1), (32, 2), (32, 3), (100, 0), (100, 1), (100, 2))
SAMPLE = 256                                                                      # patterns the host enumeration searches at e = 1
BATCH = {3: 1 << 13}                                                              # approx_batch to begin with, per e; the default otherwise


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": len(times)}


def within_one_edit(np, p):
    """[(string, distance)] of every distinct string within one edit of p over the comp values 1..5, p itself first."""
    found = {p.tobytes(): 0}
    for j in range(p.size):
        found.setdefault(np.concatenate([p[:j], p[j + 1:]]).tobytes(), 1)
        for c in range(1, 6):
            q = p.copy(); q[j] = c
            found.setdefault(q.tobytes(), 1)
    for j in range(p.size + 1):
        for c in range(1, 6):
            found.setdefault(np.concatenate([p[:j], np.array([c], dtype=np.uint8), p[j:]]).tobytes(), 1)
    return [(np.frombuffer(k, dtype=np.uint8), v) for k, v in found.items()]


def make_patterns(np, rng, reads, m):
    """One pattern of m symbols per read; every second one with one indel."""
    count, readlen = reads.shape
    out = np.zeros((count, m), dtype=np.uint8)
    indels = {"deletions": 0, "insertions": 0}
    for k in range(count):
        kind = (0 if k % 2 == 0 else int(rng.integers(1, 3)))                     # 0 none, 1 deletion, 2 insertion
        if kind == 1 and m + 1 > readlen:
            kind = 2                                                              # a pattern as long as a read: nothing longer to delete from
        cut = m + (1 if kind == 1 else -1 if kind == 2 else 0)
        if cut < 1:
            kind, cut = 0, m
        o = int(rng.integers(0, readlen - cut + 1))
        p = reads[k, o: o + cut]
        if kind == 1:
            j = int(rng.integers(0, cut)); p = np.concatenate([p[:j], p[j + 1:]]); indels["deletions"] += 1
        elif kind == 2:
            j = int(rng.integers(0, cut + 1)); p = np.concatenate([p[:j], rng.integers(1, 5, size=1).astype(np.uint8), p[j:]]); indels["insertions"] += 1
        out[k] = p
    return out, indels


def run_config(pkg, np, ix, patterns, m, e, args):
    lib, p_u64, p_u32, p_u8 = pkg.capi.lib(), pkg.capi.p_u64, pkg.capi.p_u32, pkg.capi.p_u8
    count = patterns.shape[0]
    text = np.ascontiguousarray(patterns).reshape(-1)
    offsets = np.arange(count + 1, dtype=np.uint64) * np.uint64(m)
    hit_offsets, ham_offsets = np.zeros(count + 1, dtype=np.uint64), np.zeros(count + 1, dtype=np.uint64)
    ptr = lambda a, t: a.ctypes.data_as(t) if a is not None else None
    out = {"m": m, "e": e, "patterns": count}

    def call(sp, cnt, ed, ln, capacity):
        t0 = time.perf_counter()
        pkg.capi.check(lib.bwtm_find_edit_batch(ix.h, ptr(text, p_u8), ptr(offsets, p_u64), count, e, 0, ptr(hit_offsets, p_u64), ptr(sp, p_u64), ptr(cnt, p_u64), ptr(ed, p_u8),
                                                ptr(ln, p_u32), capacity))
        return (time.perf_counter() - t0) * 1e3

    def hamming(sp, cnt, mm, capacity):
        t0 = time.perf_counter()
        pkg.capi.check(lib.bwtm_find_approx_batch(ix.h, ptr(text, p_u8), ptr(offsets, p_u64), count, e, 0, ptr(ham_offsets, p_u64), ptr(sp, p_u64), ptr(cnt, p_u64), ptr(mm, p_u8), capacity))
        return (time.perf_counter() - t0) * 1e3

    # the batch size: the default, halved while a frontier or the hit stream does not fit the device
    batch = BATCH.get(e, 1 << 16)
    while True:
        pkg.tune("approx_batch", batch)
        pkg.synchronize(); pkg.trim()
        held = pkg.pool_stats()["held_bytes"]
        pkg.device_bytes_peak(reset=True)
        try:
            sizing = call(None, None, None, None, 0)                                                    # the warm-up as well
            break
        except pkg.BwtmError as err:
            if batch <= 256 or "hipMalloc" not in str(err) and "do not fit" not in str(err) and "does not fit" not in str(err):
                raise
            out.setdefault("batches_that_did_not_fit", []).append(batch)
            batch //= 2
    out["approx_batch"] = batch
    total = int(hit_offsets[-1])
    sp, cnt, ed, ln = np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=np.uint32)
    first = call(sp, cnt, ed, ln, total)
    stats = pkg.find_edit_stats()
    P, H = stats["frontier_peak"], stats["batch_hits"]
    out.update({"hits": total, "hits_per_pattern": total / count, "patterns_with_hits": int((np.diff(hit_offsets) > 0).sum()),
                "hits_by_length_minus_m": {str(k - m): int(v) for k, v in enumerate(np.bincount(ln, minlength=m + e + 1).tolist()) if v},
                "hits_by_edits": np.bincount(ed, minlength=e + 1).tolist(),
                "nodes_expanded": stats["expanded"], "nodes_expanded_per_pattern": stats["expanded"] / count, "frontier_peak_nodes": P, "levels": stats["levels"],
                "peak_bytes_beyond_held": pkg.device_bytes_peak() - held,
                "documented_bound_bytes_per_call": (308 + 34 * e) * P + 132 * H + 2 * min(count, batch) * m + (1 << 20),
                "sizing_call_ms": sizing, "first_fill_call_ms": first})
    # the Hamming search at d = e on the same patterns, alternating with the edit search
    hamming(None, None, None, 0)
    htotal = int(ham_offsets[-1])
    hsp, hcnt, hmm = np.zeros(htotal, dtype=np.uint64), np.zeros(htotal, dtype=np.uint64), np.zeros(htotal, dtype=np.uint8)
    hamming(hsp, hcnt, hmm, htotal)
    hstats = pkg.find_approx_stats()
    repeats = (args.repeats if first < 4000 else 1)                                                     # a case of seconds per call runs once more, not `repeats` times
    walls, hwalls = [], []
    for _ in range(repeats):
        walls.append(call(sp, cnt, ed, ln, total))
        hwalls.append(hamming(hsp, hcnt, hmm, htotal))
    out["fill_call"] = summary(walls)
    out["ns_per_pattern"] = statistics.median(walls) * 1e6 / count
    # every Hamming hit is an edit hit of the pattern's own length with the same range, at no more edits than mismatches
    owner = np.repeat(np.arange(count, dtype=np.uint64), np.diff(hit_offsets).astype(np.int64))
    howner = np.repeat(np.arange(count, dtype=np.uint64), np.diff(ham_offsets).astype(np.int64))
    assert ix.bases < (1 << 34)
    own = np.flatnonzero(ln == m)
    keys = (owner[own] << np.uint64(34)) | sp[own]
    order = np.argsort(keys, kind="stable")
    keys, own = keys[order], own[order]
    assert np.all(np.diff(keys.astype(np.int64)) > 0), "m = %d, e = %d: two hits of one pattern and one length share a range" % (m, e)
    hkeys = (howner << np.uint64(34)) | hsp
    at = np.searchsorted(keys, hkeys)
    inside = (at < keys.size)
    inside[inside] = keys[at[inside]] == hkeys[inside]
    assert bool(np.all(inside)), "m = %d, e = %d: %d Hamming hits are not among the edit hits" % (m, e, int((~inside).sum()))
    assert np.array_equal(cnt[own[at]], hcnt) and bool(np.all(ed[own[at]] <= hmm)), "m = %d, e = %d: a Hamming hit's count or distance differs" % (m, e)
    out["hamming"] = {"d": e, "hits": htotal, "hits_per_pattern": htotal / count, "nodes_expanded_per_pattern": hstats["expanded"] / count, "frontier_peak_nodes": hstats["frontier_peak"],
                      "fill_call": summary(hwalls), "ns_per_pattern": statistics.median(hwalls) * 1e6 / count, "hits_among_the_edit_hits": htotal, "subset": True,
                      "edit_hits_cheaper_than_mismatches": int((ed[own[at]] < hmm).sum())}
    out["edit_ns_over_hamming_ns"] = out["ns_per_pattern"] / out["hamming"]["ns_per_pattern"]
    # the kernels alone, from the library's own events (one filling call)
    pkg.profile_reset(); pkg.profile_enable(True)
    wall = call(sp, cnt, ed, ln, total)
    prof = pkg.profile_read()
    pkg.profile_enable(False)
    mine = {name: {"total_ms": round(v[0], 3), "launches": v[1]} for name, v in prof.items() if name.startswith("edit_") or name.startswith("scan_")}
    out["kernels_ms"] = mine
    out["kernel_ms"] = round(sum(v["total_ms"] for v in mine.values()), 3)
    out["profiled_call_ms"] = wall
    out["host_side_share"] = 1.0 - out["kernel_ms"] / wall if wall > 0 else None                        # of the profiled call: its events cost host time too
    # the route before, at e = 1: every string within one edit of a seeded sample, through bwtm_find_batch
    if e == 1:
        rng = np.random.default_rng(17)
        picks = np.sort(rng.choice(count, size=min(SAMPLE, count), replace=False))
        strings, dist, owner2 = [], [], []
        for j, k in enumerate(picks.tolist()):
            for s, d in within_one_edit(np, patterns[k]):
                strings.append(s); dist.append(d); owner2.append(j)
        dist, owner2 = np.array(dist, dtype=np.uint8), np.array(owner2, dtype=np.int64)
        lens = np.array([s.size for s in strings], dtype=np.uint64)
        ntext = np.ascontiguousarray(np.concatenate(strings))
        noff = np.zeros(len(strings) + 1, dtype=np.uint64); noff[1:] = np.cumsum(lens)
        fsp, fep = np.zeros(len(strings), dtype=np.uint64), np.zeros(len(strings), dtype=np.uint64)

        def find():
            t0 = time.perf_counter()
            pkg.capi.check(lib.bwtm_find_batch(ix.h, ptr(ntext, p_u8), ptr(noff, p_u64), len(strings), ptr(fsp, p_u64), ptr(fep, p_u64)))
            return (time.perf_counter() - t0) * 1e3

        find()
        times = [find() for _ in range(args.repeats)]
        found = (fsp <= fep) & (fep < np.uint64(ix.bases))
        equal = 0
        for j, k in enumerate(picks.tolist()):
            sel = np.flatnonzero(found & (owner2 == j))
            rows = sorted((int(lens[s]), tuple(strings[s][::-1].tolist()), int(fsp[s]), int(fep[s]), int(dist[s])) for s in sel.tolist())   # shortest first, then by the reversed string
            a, b = int(hit_offsets[k]), int(hit_offsets[k + 1])
            mine_rows = [(int(ln[h]), int(sp[h]), int(sp[h] + cnt[h]) - 1, int(ed[h])) for h in range(a, b)]
            assert mine_rows == [(r[0], r[2], r[3], r[4]) for r in rows], "m = %d: the hits of pattern %d differ from those of its %d neighbours" % (m, k, int((owner2 == j).sum()))
            equal += 1
        out["enumeration"] = {"sample_patterns": int(picks.size), "searches": len(strings), "searches_per_pattern": len(strings) / picks.size, "hit_sets_equal": equal,
                              "find_batch_calls": summary(times), "ns_per_pattern": statistics.median(times) * 1e6 / picks.size}
        out["enumeration_ns_over_edit_ns"] = out["enumeration"]["ns_per_pattern"] / out["ns_per_pattern"]
    pkg.tune("approx_batch", 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=30_000_000)
    ap.add_argument("--readlen", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--patterns", type=int, default=1 << 16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default=",".join("%d:%d" % c for c in CONFIGS), help="m:e pairs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import _pkg
    pkg = _pkg.load()
    from bwt_merge_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("edit_bench: no GPU (a CPU run cannot time this)")
    torch.cuda.set_device(0); pkg.init(0)
    t0 = time.perf_counter()
    ix = synth.build_index(pkg, args.seed, args.reads, args.readlen, device=torch.device("cuda", 0), workload="genome")
    pkg.synchronize()
    torch.cuda.empty_cache()
    result = {"reads": args.reads, "readlen": args.readlen, "workload": "genome, 30x coverage, 1 % substitutions", "device": torch.cuda.get_device_name(0),
              "library": os.path.basename(pkg.capi.LIB_PATH), "index_build_s": round(time.perf_counter() - t0, 2), "bases": ix.bases, "configs": []}
    assert ix.sequences == args.reads and ix.bases == args.reads * (args.readlen + 1)
    rng = np.random.default_rng(5)
    ids = rng.choice(args.reads, size=args.patterns, replace=False).astype(np.uint64)
    roff, rtext = ix.extract_sequences(ids=ids, max_len=args.readlen)
    assert np.all(np.diff(roff) == args.readlen)
    reads = rtext.reshape(args.patterns, args.readlen)
    made = {}
    for m, e in (tuple(int(v) for v in c.split(":")) for c in args.configs.split(",")):
        assert m <= args.readlen and 0 <= e <= 7
        if m not in made:
            made[m] = make_patterns(np, rng, reads, m)
        config = run_config(pkg, np, ix, made[m][0], m, e, args)
        config["patterns_with_one_indel"] = made[m][1]
        result["configs"].append(config)
        print("m = %d, e = %d done: %.1f ns per pattern" % (m, e, config["ns_per_pattern"]), file=sys.stderr, flush=True)
        if args.out:                                                                                    # what has been measured so far stays if a later case does not finish
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")
    ix.free()
    result["every_hamming_hit_set_is_a_subset"] = all(c["hamming"]["subset"] for c in result["configs"])
    result["every_enumerated_hit_set_is_equal"] = all(c["enumeration"]["hit_sets_equal"] == c["enumeration"]["sample_patterns"] for c in result["configs"] if "enumeration" in c)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
