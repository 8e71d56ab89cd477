#!/usr/bin/env python3
"""K-mer error correction of the reads of a device-resident index (Kmers.corrector, bwtm_correct_sequences), next to its floor --
bwtm_sequences_extract of the same ids: the corrector reads the same reads -- and next to the host route: the solid k-mers and the reads
brought to the host and corrected there by the brute force of tests/correct_inputs.py, on a seeded sample of the same reads, its time per
read extrapolated (the two downloads are timed apart and counted in the route's total; every compared read must be equal in text, status
and edits).  Where two kernel forms run, their text, status and edits must be equal before any ratio between them is reported.

The index holds reads of a shared genome at 30x coverage with 1 % substitutions (the generator behind `bench.py --workload genome`, the
index of tools/kmer_bench.py).

    python tools/correct_bench.py [--reads 30000000] [--readlen 100] [--ks 21,31] [--threshold 3] [--ids 1048576] [--sample 512] [--repeats 5] [--out profiles/correct_bench.json]
    bash tools/build_variant.sh diag "" -DBWTM_DIAGNOSTICS; BWTM_LIB=bwt-merge_amd/_variants/diag.so python tools/correct_bench.py --out profiles/correct_bench_lanes_diag.json
                                                      # a diagnostics build also holds the kernel with one lane per read (bwtm_tune("correct_kernel", 1)): the calls are
                                                      # then run in both forms, alternating, so that the two share whatever else the machine is doing

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

FORMS = {0: "one_wave_per_read", 1: "one_lane_per_read"}          # values of the correct_kernel knob of a diagnostics build; the product has form 0 only


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": len(times)}


def timed(fn):
    t0 = time.perf_counter()
    got = fn()
    return got, (time.perf_counter() - t0) * 1e3


class HostTable:
    """The solid k-mers on the host as the brute force wants them: get(window) -> count, a binary search in the downloaded codes."""

    def __init__(self, np, codes, counts, k, skip=5):
        self.np, self.codes, self.counts, self.k = np, codes, counts, k
        self.rank = {c: j for j, c in enumerate(c for c in range(1, 6) if c != skip)}

    def get(self, window, default=0):
        code = 0
        for s in window:
            code = (code << 2) | self.rank[s]
        at = int(self.np.searchsorted(self.codes, self.np.uint64(code)))
        return int(self.counts[at]) if at < self.codes.size and int(self.codes[at]) == code else default


def run_config(pkg, np, ix, k, args):
    from correct_inputs import correct
    t, ids, first = args.threshold, args.ids, args.first
    out = {"k": k, "threshold": t, "ids": ids, "first_id": first, "max_rounds": args.rounds}
    # the spectrum above the threshold, and the table
    for _ in range(2):
        km, ms = timed(lambda: ix.kmers(k, min_count=t))
        km.free()
    walls = []
    for _ in range(args.repeats):
        km, ms = timed(lambda: ix.kmers(k, min_count=t))
        walls.append(ms); km.free()
    out["kmers_create"] = summary(walls)
    km = ix.kmers(k, min_count=t)
    km.corrector(t).free()
    walls = []
    for _ in range(args.repeats):
        cor, ms = timed(lambda: km.corrector(t))
        walls.append(ms); cor.free()
    out["corrector_create"] = summary(walls)
    cor = km.corrector(t)
    out.update({"kmers": km.distinct, "solid": cor.solid, "kmers_bytes": km.nbytes, "corrector_bytes": cor.nbytes})

    def status_call():
        return cor.correct_sequences(ix, first=first, count=ids, max_len=args.readlen, max_rounds=args.rounds, text=False)

    offsets = ix.sequences(first=first, count=ids, max_len=args.readlen)[0]
    text = np.zeros(int(offsets[-1]), dtype=np.uint8); status = np.zeros(ids, dtype=np.uint8); edits = np.zeros(ids, dtype=np.uint32)
    lib, capi = pkg.capi.lib(), pkg.capi

    def filling_call():                                       # one call, the buffers sized before: the sizing call is the floor's own first half
        capi.check(lib.bwtm_correct_sequences(cor.h, ix.h, None, first, ids, args.readlen, args.rounds, offsets.ctypes.data_as(capi.p_u64), text.ctypes.data_as(capi.p_u8), text.size,
                                              status.ctypes.data_as(capi.p_u8), edits.ctypes.data_as(capi.p_u32)))

    plain = np.zeros_like(text)

    def extract_call():
        capi.check(lib.bwtm_sequences_extract(ix.h, None, first, ids, args.readlen, offsets.ctypes.data_as(capi.p_u64), plain.ctypes.data_as(capi.p_u8), plain.size))

    walls = {(form, what): [] for form in args.forms for what in ("status_call", "filling_call")}
    floor = []
    results = {}                                              # form -> the text, status and edits of its filling call
    for rep in range(args.repeats + 1):                       # the first round is the warm-up
        for form in args.forms:
            if len(args.forms) > 1:
                pkg.tune("correct_kernel", form)
            for what, fn in (("status_call", status_call), ("filling_call", filling_call)):
                _, ms = timed(fn)
                if rep > 0:
                    walls[(form, what)].append(ms)
        _, ms = timed(extract_call)
        if rep > 0:
            floor.append(ms)
    out["sequences_extract"] = summary(floor)
    for form in args.forms:
        if len(args.forms) > 1:
            pkg.tune("correct_kernel", form)
        o = {what: summary(walls[(form, what)]) for what in ("status_call", "filling_call")}
        for what in ("status_call", "filling_call"):
            o[what + "_over_extract"] = o[what]["median_ms"] / out["sequences_extract"]["median_ms"]
        pkg.profile_reset(); pkg.profile_enable(True)
        filling_call()
        prof = pkg.profile_read()
        pkg.profile_enable(False)
        o["kernels_ms"] = {name: {"total_ms": round(v[0], 3), "launches": v[1]} for name, v in prof.items()}
        o["stats"] = pkg.correct_stats()
        o["statuses"] = np.bincount(status, minlength=4).tolist()
        o["edits"] = int(edits.sum())
        out[FORMS[form]] = o
        results[form] = (text.copy(), status.copy(), edits.copy())
    if len(args.forms) > 1:
        for name, a, b in zip(("text", "status", "edits"), results[0], results[1]):       # no ratio between kernels that disagree
            assert np.array_equal(a, b), "the two kernels disagree in %s (%d places)" % (name, int(np.count_nonzero(a != b)))
        out["forms_equal"] = True
        a, b = out[FORMS[0]], out[FORMS[1]]
        out["lane_over_wave_filling_call"] = b["filling_call"]["median_ms"] / a["filling_call"]["median_ms"]
        out["lane_over_wave_kernel"] = b["kernels_ms"]["correct"]["total_ms"] / a["kernels_ms"]["correct"]["total_ms"]
        pkg.tune("correct_kernel", 0)
        filling_call()
    # the host route on a sample: the solid k-mers down, the reads down, the brute force
    (codes, counts, _), ms_kmers = timed(lambda: km.download())
    keep = counts >= np.uint64(t)
    table = HostTable(np, codes[keep], counts[keep], k)
    _, ms_reads = timed(extract_call)
    picks = np.sort(np.random.default_rng(9).choice(ids, size=min(args.sample, ids), replace=False))
    t0 = time.perf_counter()
    equal = 0
    for j in picks.tolist():
        row = plain[int(offsets[j]): int(offsets[j + 1])]
        got = correct(row, table, k, t, args.rounds)
        equal += int(got == (bytes(bytearray(text[int(offsets[j]): int(offsets[j + 1])].tolist())), int(status[j]), int(edits[j])))
    brute_ms = (time.perf_counter() - t0) * 1e3
    assert equal == picks.size, "the brute force and the library disagree on %d of %d reads" % (picks.size - equal, picks.size)
    per_read = brute_ms / picks.size
    out["host_route"] = {"sample": int(picks.size), "reads_equal": equal, "brute_ms_per_read": per_read, "brute_ms_extrapolated": per_read * ids,
                         "kmers_download_ms": ms_kmers, "kmers_download_bytes": int(24 * codes.size), "reads_download_ms": ms_reads,
                         "what": "tests/correct_inputs.py correct() in Python over a binary search in the downloaded codes; one run, not repeated; the ingest of the corrected reads is not timed"}
    out["host_route"]["total_ms_extrapolated"] = ms_kmers + ms_reads + per_read * ids                    # the k-mers down, the reads down, the brute force
    out["host_route"]["extrapolated_over_filling_call"] = out["host_route"]["total_ms_extrapolated"] / out[FORMS[0]]["filling_call"]["median_ms"]
    cor.free(); km.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=30_000_000)
    ap.add_argument("--readlen", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--ks", default="21,31")
    ap.add_argument("--threshold", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--ids", type=int, default=1 << 20)
    ap.add_argument("--first", type=int, default=1 << 22)
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
        raise SystemExit("correct_bench: no GPU (a CPU run cannot time this)")
    torch.cuda.set_device(0); pkg.init(0)
    try:
        pkg.tune("correct_kernel", 0)                         # an unknown key on a product build: raises
        args.forms = (0, 1)
    except pkg.BwtmError:
        args.forms = (0,)
    args.ids = min(args.ids, args.reads); args.first = min(args.first, args.reads - args.ids)
    t0 = time.perf_counter()
    ix = synth.build_index(pkg, args.seed, args.reads, args.readlen, device=torch.device("cuda", 0), workload="genome")
    pkg.synchronize()
    torch.cuda.empty_cache()
    result = {"reads": args.reads, "readlen": args.readlen, "workload": "genome, 30x coverage, 1 % substitutions", "device": torch.cuda.get_device_name(0),
              "library": os.path.basename(pkg.capi.LIB_PATH), "forms": [FORMS[f] for f in args.forms], "index_build_s": round(time.perf_counter() - t0, 2), "bases": ix.bases, "configs": []}
    assert ix.sequences == args.reads and ix.bases == args.reads * (args.readlen + 1)
    for k in (int(v) for v in args.ks.split(",")):
        result["configs"].append(run_config(pkg, np, ix, k, args))
        print("k = %d done" % k, file=sys.stderr, flush=True)
    ix.free()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
