#!/usr/bin/env python3
"""The unitigs of the k-mer graph of a device-resident index (Kmers.unitigs, bwtm_unitigs_create): the time of the call and of its phases,
the graph's size, the longest unitig (whose serial walk the call's time contains), the device peak and the download; next to the only
other route there is: the solid k-mers brought to the host (bwtm_kmers_download), links by np.searchsorted there and the walk in Python.
The host route runs on a SMALLER index of the same kind (--host-reads), small enough for the Python walk to finish, and there the two
routes' graphs are compared in full -- offsets, text, nodes, occurrences, flags, links; nothing is extrapolated to the large index.

The large index holds reads of a shared genome at 30x coverage with 1 % substitutions (the generator behind `bench.py --workload genome`,
the index of tools/kmer_bench.py and tools/correct_bench.py).

    python tools/unitig_bench.py [--reads 30000000] [--host-reads 300000] [--readlen 100] [--ks 21,31] [--threshold 3] [--repeats 5] [--out profiles/unitig_bench.json]

Times are host clocks around calls that end in a stream synchronise, medians of `--repeats` runs after one warm-up run of the same shape, with
the fastest and the slowest run next to them; kernel times are the library's own events in a run of their own.
Needs a GPU; prints one JSON object and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NONE = (1 << 64) - 1
SLICE = 1 << 20                                               # unitigs per download call, as bwt_unitigs takes them


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": len(times)}


def timed(fn):
    t0 = time.perf_counter()
    got = fn()
    return got, (time.perf_counter() - t0) * 1e3


def host_route(np, codes, counts, k, skip=5):
    """(offsets, text, nodes, occurrences, flags, links) from the sorted solid codes: degrees and successors by np.searchsorted, the walk
    of every path and cycle in Python, the text and the links by numpy.  Returns the arrays and the milliseconds of the three parts."""
    t0 = time.perf_counter()
    S = codes.size
    mask = np.uint64((1 << (2 * k)) - 1)
    base = (codes << np.uint64(2)) & mask
    lo = np.searchsorted(codes, base, side="left")
    hi = np.searchsorted(codes, base + np.uint64(3), side="right")
    out = hi - lo
    inn = np.zeros(S, dtype=np.int64)
    for r in range(4):
        p = (np.uint64(r) << np.uint64(2 * (k - 1))) | (codes >> np.uint64(2))
        at = np.minimum(np.searchsorted(codes, p), S - 1)
        inn += codes[at] == p
    one = np.flatnonzero(out == 1)
    one = one[inn[lo[one]] == 1]
    nxt = np.full(S, -1, dtype=np.int64)
    nxt[one] = lo[one]
    has_prev = np.zeros(S, dtype=bool)
    has_prev[nxt[one]] = True
    t1 = time.perf_counter()
    # the walk, in Python
    nx = nxt.tolist()
    seen = bytearray(S)
    order, firsts, lens, circ = [], [], [], []
    for s in np.flatnonzero(~has_prev).tolist():
        n, cur = 0, s
        while cur >= 0:
            order.append(cur); seen[cur] = 1; n += 1
            cur = nx[cur]
        firsts.append(s); lens.append(n); circ.append(0)
    if len(order) < S:
        for s in range(S):                                    # ascending: s is its cycle's smallest node
            if seen[s]:
                continue
            n, cur = 0, s
            while not seen[cur]:
                order.append(cur); seen[cur] = 1; n += 1
                cur = nx[cur]
            firsts.append(s); lens.append(n); circ.append(1)
    t2 = time.perf_counter()
    firsts = np.array(firsts, dtype=np.int64); lens = np.array(lens, dtype=np.int64); circ = np.array(circ, dtype=np.uint8)
    order = np.array(order, dtype=np.int64)
    begin = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)          # of a unitig in `order`, in the order of the walks
    by_code = np.argsort(firsts, kind="stable")
    U = firsts.size
    number = np.empty(U, dtype=np.int64); number[by_code] = np.arange(U)          # a walk's unitig
    walk_of = np.repeat(np.arange(U), lens)
    unitig_of = np.empty(S, dtype=np.int64); unitig_of[order] = number[walk_of]
    off_in = np.empty(S, dtype=np.int64); off_in[order] = np.arange(S) - begin[walk_of]
    n_u = lens[by_code]
    offsets = np.zeros(U + 1, dtype=np.uint64); offsets[1:] = np.cumsum(n_u + k - 1)
    kept = np.array([c for c in range(1, 6) if c != skip], dtype=np.uint8)
    text = np.zeros(int(offsets[-1]), dtype=np.uint8)
    text[offsets[unitig_of].astype(np.int64) + off_in + k - 1] = kept[(codes & np.uint64(3)).astype(np.int64)]
    first_codes = codes[firsts[by_code]]
    for q in range(k - 1):
        text[offsets[:-1].astype(np.int64) + q] = kept[((first_codes >> np.uint64(2 * (k - 1 - q))) & np.uint64(3)).astype(np.int64)]
    occ = np.zeros(U, dtype=np.uint64); np.add.at(occ, unitig_of, counts)
    last = order[begin[by_code] + n_u - 1]
    links = np.full((U, 4), NONE, dtype=np.uint64)
    flags = circ[by_code]
    for e in range(4):
        at = lo[last] + e
        ok = (at < hi[last]) & (flags == 0)
        rows = np.flatnonzero(ok)
        r = (codes[at[rows]] - base[last[rows]]).astype(np.int64)
        links[rows, r] = unitig_of[at[rows]].astype(np.uint64)
    t3 = time.perf_counter()
    arrays = (offsets, text, n_u.astype(np.uint64), occ, flags, links)
    return arrays, {"links_ms": (t1 - t0) * 1e3, "walk_ms": (t2 - t1) * 1e3, "text_and_links_ms": (t3 - t2) * 1e3}


def download_all(u):
    parts = [u.download(first, min(SLICE, u.count - first)) for first in range(0, u.count, SLICE)]
    return parts


def gpu_config(pkg, np, ix, k, args, compare_host):
    t = args.threshold
    out = {"k": k, "threshold": t}
    km = ix.kmers(k, min_count=t)
    km.unitigs(t).free()                                      # the warm-up
    walls = []
    for _ in range(args.repeats):
        u, ms = timed(lambda: km.unitigs(t))
        walls.append(ms); u.free()
    out["unitigs_create"] = summary(walls)
    pkg.synchronize(); pkg.trim()
    held = pkg.pool_stats()["held_bytes"]
    pkg.device_bytes_peak(reset=True)
    pkg.profile_reset(); pkg.profile_enable(True)
    u = km.unitigs(t)
    prof = pkg.profile_read()
    pkg.profile_enable(False)
    out["device_peak_bytes_beyond_index_and_kmers"] = pkg.device_bytes_peak() - held
    out["kernels_ms"] = {name: {"total_ms": round(v[0], 3), "launches": v[1]} for name, v in prof.items()}
    out["stats"] = pkg.unitigs_stats()
    out.update({"kmers": km.distinct, "kmers_bytes": km.nbytes, "nodes": u.nodes, "unitigs": u.count, "symbols": u.symbols, "handle_bytes": u.bytes})
    out["longest_unitig_nodes"] = out["stats"]["longest"]
    out["walk_kernel_ms"] = out["kernels_ms"].get("unitig_walk", {}).get("total_ms")
    parts, ms = timed(lambda: download_all(u))
    out["download"] = {"ms": ms, "bytes": int(sum(a.nbytes for p in parts for a in p)), "slices": len(parts)}
    flags = np.concatenate([p[4] for p in parts]) if parts else np.zeros(0, dtype=np.uint8)
    links = np.concatenate([p[5] for p in parts]) if parts else np.zeros((0, 4), dtype=np.uint64)
    out["circular_unitigs"] = int((flags & 1).sum())
    out["links"] = int((links != np.uint64(NONE)).sum())
    if compare_host:
        (codes, counts, _), ms_down = timed(lambda: km.download())
        keep = counts >= np.uint64(t)
        want, parts_ms = host_route(np, codes[keep], counts[keep], k)
        names = ("offsets", "text", "nodes", "occurrences", "flags", "links")
        got = u.download()
        for name, a, b in zip(names, got, want):
            assert a.shape == b.shape and np.array_equal(a, b), "the two routes disagree in %s" % name
        host_ms = ms_down + sum(parts_ms.values())
        out["host_route"] = dict(parts_ms, kmers_download_ms=ms_down, kmers_download_bytes=int(24 * codes.size), total_ms=host_ms, graphs_equal=True,
                                 what="bwtm_kmers_download, degrees and successors by np.searchsorted, the walk of every path in Python, text and links by numpy; one run, not repeated")
        out["host_route"]["total_over_create_plus_download"] = host_ms / (out["unitigs_create"]["median_ms"] + out["download"]["ms"])
    u.free(); km.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=30_000_000)
    ap.add_argument("--host-reads", type=int, default=300_000)
    ap.add_argument("--readlen", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--threshold", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import _pkg
    pkg = _pkg.load()
    from bwt_merge_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("unitig_bench: no GPU (a CPU run cannot time this)")
    torch.cuda.set_device(0); pkg.init(0)
    result = {"readlen": args.readlen, "workload": "genome, 30x coverage, 1 % substitutions", "device": torch.cuda.get_device_name(0),
              "library": os.path.basename(pkg.capi.LIB_PATH), "indexes": []}
    for reads, compare_host in ((args.host_reads, True), (args.reads, False)):
        if reads <= 0:
            continue
        t0 = time.perf_counter()
        ix = synth.build_index(pkg, args.seed, reads, args.readlen, device=torch.device("cuda", 0), workload="genome")
        pkg.synchronize()
        torch.cuda.empty_cache()
        entry = {"reads": reads, "bases": ix.bases, "index_build_s": round(time.perf_counter() - t0, 2), "host_route_run": compare_host, "configs": []}
        for k in (int(v) for v in args.ks.split(",")):
            entry["configs"].append(gpu_config(pkg, np, ix, k, args, compare_host))
            print("%d reads, k = %d done" % (reads, k), file=sys.stderr, flush=True)
        ix.free()
        pkg.trim()
        result["indexes"].append(entry)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
