#!/usr/bin/env python3
"""The k-mers of two device-resident indexes side by side (Index.kmer_join, bwtm_kmer_join_create), next to the only route the library had
for that question before: two bwtm_kmers_create calls, two downloads of codes and counts, and np.intersect1d / np.setdiff1d (np.union1d for
the union) on the host.

Two read sets of `--readlen` bp at 30x coverage with 1 % substitutions are cut from one random genome (the generator behind
`bench.py --workload genome`); the genome of the second set differs from it by substitutions at `--divergence-ppm` positions per million.
Three questions at every k: the union with both counts (all defaults), the shared k-mers (min_a = min_b = 1), and those that are in b at
least twice and absent from a (min_b = 2, max_a = 0).  Both routes must give the same k-mers with the same counts.

The default size is a fifteenth of tools/kmer_bench.py's index per set: the union's frontiers hold both sets' error k-mers (about 250 bytes of
device memory per node of the largest level at the peak), and the host join of the old route sorts both lists, seconds at this size.

    python tools/kmer_join_bench.py [--reads 2000000] [--readlen 100] [--divergence-ppm 1000] [--ks 21,31] [--repeats 5] [--host-repeats 5] [--out profiles/kmer_join_bench.json]

Times are host clocks around calls that end in a stream synchronise or on the host, medians of `--repeats` runs after one warm-up run of the
same shape, with the fastest and the slowest run next to them; kernel times are the library's own events in a run of their own.
Needs a GPU; prints one JSON object and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUERIES = (("union", {}), ("shared", dict(min_a=1, min_b=1)), ("in_b_twice_absent_from_a", dict(min_b=2, max_a=0)))
VARIANT_SEED = 424243


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": len(times)}


def variant_genome_reads(synth, torch, seed, first_read, nreads, readlen, genome_len, device, divergence_ppm, error_percent=1):
    """synth.generate_genome_reads on a genome whose base at position p is another one when splitmix64(p) % 10^6 < divergence_ppm: the same
    counters otherwise, so divergence_ppm = 0 gives that generator's reads."""
    j = synth._read_ids(first_read, nreads, device)
    t = torch.arange(readlen, dtype=torch.int64, device=device).unsqueeze(0)
    span = max(1, genome_len - readlen + 1)
    start = synth._lsr(synth._mix(j * synth._s64(synth._GAMMA) + synth._s64(seed * 3 + 1)), 1) % span
    pos = start + t
    g = synth._mix(pos * synth._s64(synth._GAMMA) + synth._s64(synth.GENOME_SEED)) & 3
    v = synth._mix(pos * synth._s64(synth._GAMMA) + synth._s64(VARIANT_SEED))
    g = torch.where((synth._lsr(v, 8) % 1000000) < divergence_ppm, (g + 1 + ((v & 0xFF) % 3)) & 3, g)
    z = synth._mix((j * 256 + t) * synth._s64(2 * synth._GAMMA) + synth._s64(seed + 5 * synth._GAMMA))
    is_sub = (synth._lsr(z, 8) % 100) < error_percent
    other = (g + 1 + ((z & 0xFF) % 3)) & 3
    return (1 + torch.where(is_sub, other, g)).to(torch.uint8)


def build_index(pkg, synth, torch, seed, nreads, readlen, genome_len, device, divergence_ppm, leaf_reads=1 << 19):
    builder = pkg.Builder(leaf_reads)
    for first in range(0, nreads, leaf_reads):
        count = min(leaf_reads, nreads - first)
        reads = variant_genome_reads(synth, torch, seed, first, count, readlen, genome_len, device, divergence_ppm).contiguous()
        torch.cuda.synchronize()
        builder.add_device(reads.data_ptr(), count, reads.shape[1])
        del reads
    return builder.finish()


def download_kmers(pkg, np, km):
    """codes and counts of a bwtm_kmers handle (sp is not asked for)."""
    p_u64 = pkg.capi.p_u64
    codes, counts = np.empty(km.distinct, dtype=np.uint64), np.empty(km.distinct, dtype=np.uint64)
    pkg.capi.check(pkg.capi.lib().bwtm_kmers_download(km.h, 0, km.distinct, codes.ctypes.data_as(p_u64), counts.ctypes.data_as(p_u64), None))
    return codes, counts


def download_join(pkg, np, kj):
    """codes and both counts of a bwtm_kmer_join handle (the insertion points are not asked for)."""
    p_u64 = pkg.capi.p_u64
    arrays = [np.empty(kj.distinct, dtype=np.uint64) for _ in range(3)]
    pkg.capi.check(pkg.capi.lib().bwtm_kmer_join_download(kj.h, 0, kj.distinct, *[a.ctypes.data_as(p_u64) for a in arrays], None, None))
    return arrays


def old_route(pkg, np, A, B, k, name):
    """The parent's route: (codes, count_a, count_b) and the milliseconds of its steps."""
    t0 = time.perf_counter()
    ka = A.kmers(k)
    t1 = time.perf_counter()
    kb = B.kmers(k, min_count=2 if name == "in_b_twice_absent_from_a" else 1)
    t2 = time.perf_counter()
    codes_a, counts_a = download_kmers(pkg, np, ka)
    codes_b, counts_b = download_kmers(pkg, np, kb)
    t3 = time.perf_counter()
    ka.free(); kb.free()
    if name == "shared":
        codes, ia, ib = np.intersect1d(codes_a, codes_b, assume_unique=True, return_indices=True)
        out = (codes, counts_a[ia], counts_b[ib])
    elif name == "in_b_twice_absent_from_a":
        codes = np.setdiff1d(codes_b, codes_a, assume_unique=True)
        out = (codes, np.zeros(codes.size, dtype=np.uint64), counts_b[np.searchsorted(codes_b, codes)])
    else:
        codes = np.union1d(codes_a, codes_b)
        ca, cb = np.zeros(codes.size, dtype=np.uint64), np.zeros(codes.size, dtype=np.uint64)
        ca[np.searchsorted(codes, codes_a)] = counts_a
        cb[np.searchsorted(codes, codes_b)] = counts_b
        out = (codes, ca, cb)
    t4 = time.perf_counter()
    ms = {"create_a_ms": (t1 - t0) * 1e3, "create_b_ms": (t2 - t1) * 1e3, "downloads_ms": (t3 - t2) * 1e3, "host_join_ms": (t4 - t3) * 1e3, "total_ms": (t4 - t0) * 1e3}
    return out, ms


def run_config(pkg, np, A, B, k, name, bounds, args):
    out = {"k": k, "query": name, "bounds": bounds}

    def create():
        t0 = time.perf_counter()
        kj = A.kmer_join(B, k, **bounds)                      # ends in a synchronise (the summary is read back)
        return kj, (time.perf_counter() - t0) * 1e3

    kj, _ = create()                                          # warm-up
    kj.free()
    pkg.synchronize()
    pkg.trim()                                                # the peak below is this one call's
    held = pkg.pool_stats()["held_bytes"]
    pkg.device_bytes_peak(reset=True)
    kj, _ = create()
    levels = kj.levels()
    out.update({"peak_bytes": pkg.device_bytes_peak(), "held_bytes_before": held, "distinct": kj.distinct, "summary": kj.summary(), "result_bytes": kj.nbytes,
                "nodes_per_level": [int(v) for v in levels], "largest_level": int(levels.max()), "documented_bound_bytes": 392 * int(levels.max()) + (1 << 20)})
    got = download_join(pkg, np, kj)
    kj.free()
    # the old route: once for the comparison (its warm-up), then timed
    want, _ = old_route(pkg, np, A, B, k, name)
    out["results_agree"] = bool(all(np.array_equal(g, w) for g, w in zip(got, want)))
    assert out["results_agree"], "the join and the host route disagree at k = %d, %s" % (k, name)
    del got, want
    runs = [old_route(pkg, np, A, B, k, name)[1] for _ in range(args.host_repeats)]
    out["old_route"] = {key: summary([r[key] for r in runs]) for key in runs[0]}
    out["old_route"]["two_creates_ms"] = summary([r["create_a_ms"] + r["create_b_ms"] for r in runs])
    # the join: the call, and the call with the download of codes and both counts
    kj, _ = create()
    kj.free()
    walls, with_download = [], []
    for _ in range(args.repeats):
        kj, ms = create()
        kj.free()
        walls.append(ms)
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        kj = A.kmer_join(B, k, **bounds)
        download_join(pkg, np, kj)
        with_download.append((time.perf_counter() - t0) * 1e3)
        kj.free()
    out["join"] = {"create_call": summary(walls), "create_and_download": summary(with_download)}
    if out["distinct"] > 0:
        out["join"]["ns_per_kmer"] = statistics.median(walls) * 1e6 / out["distinct"]
    pkg.profile_reset(); pkg.profile_enable(True)
    kj, _ = create()
    prof = pkg.profile_read()
    pkg.profile_enable(False)
    kj.free()
    mine = {n: {"total_ms": round(v[0], 3), "launches": v[1]} for n, v in prof.items() if n.startswith("kmer_join_") or n.startswith("scan_")}
    out["join"]["kernels_ms"] = mine
    out["join"]["kernel_ms"] = round(sum(v["total_ms"] for v in mine.values()), 3)
    out["old_total_over_join_with_download"] = out["old_route"]["total_ms"]["median_ms"] / out["join"]["create_and_download"]["median_ms"]
    out["old_two_creates_over_join_create"] = out["old_route"]["two_creates_ms"]["median_ms"] / out["join"]["create_call"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000, help="reads per set")
    ap.add_argument("--readlen", type=int, default=100)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--divergence-ppm", type=int, default=1000, help="substituted positions per million of the second set's genome")
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import _pkg
    pkg = _pkg.load()
    from bwt_merge_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("kmer_join_bench: no GPU (a CPU run cannot time this)")
    torch.cuda.set_device(0); pkg.init(0)
    dev = torch.device("cuda", 0)
    genome_len = max(args.readlen, args.reads * args.readlen // args.coverage)
    t0 = time.perf_counter()
    A = build_index(pkg, synth, torch, args.seed, args.reads, args.readlen, genome_len, dev, 0)
    B = build_index(pkg, synth, torch, args.seed + 1, args.reads, args.readlen, genome_len, dev, args.divergence_ppm)
    pkg.synchronize()
    torch.cuda.empty_cache()
    result = {"reads_per_set": args.reads, "readlen": args.readlen, "genome_len": genome_len, "divergence_ppm": args.divergence_ppm,
              "workload": "two sets, %dx coverage each, 1 %% substitutions; the second genome differs at %d positions per million" % (args.coverage, args.divergence_ppm),
              "device": torch.cuda.get_device_name(0), "library": os.path.basename(pkg.capi.LIB_PATH), "index_build_s": round(time.perf_counter() - t0, 2),
              "bases_a": A.bases, "bases_b": B.bases, "repeats": args.repeats, "host_repeats": args.host_repeats, "configs": []}
    assert A.sequences == B.sequences == args.reads
    for k in (int(v) for v in args.ks.split(",")):
        for name, bounds in QUERIES:
            result["configs"].append(run_config(pkg, np, A, B, k, name, bounds, args))
            print("k = %d, %s done" % (k, name), file=sys.stderr, flush=True)
    A.free(); B.free()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
