"""One-shot bwtm_merge_host against bwtm_merge_host_streamed, host to host with COMPACT samples, alternately in one process.

    python tools/streamed_merge_bench.py [--reads 50000000] [--readlen 100] [--pairs 3] [--slices 262144,1048576,4194304,0]
    python tools/streamed_merge_bench.py --stream-upload [--pairs 3] [--slices 0] [--reads-a N]

The inputs are bench.py's (two synthetic read sets built on the device, encoded, parked in page-locked host memory; the default is
BASELINE config 2).  For every slice size (0 = the library's choice) `--pairs` pairs of calls: one-shot, then streamed.  Every call
runs twice: once behind bwtm_trim + bwtm_device_bytes_peak(reset), so that `peak_bytes` is what that call alone made the pool hold
(its time, `ms_after_trim`, includes obtaining that memory from the driver again: hundreds of ms that land in whichever phase allocates
first), and once more on the warm pool, which is the time reported as `ms`.  The streamed call runs with a sink that only counts
(what the library itself costs) and with one that copies every piece into one page-locked result buffer, which is what the one-shot
call's allocator-provided buffers amount to.  Prints one JSON line per call and a summary.

--stream-upload: the streamed call alone (counting sink), alternately with the stream_upload knob off and on (the chunked upload: no
input's native stream resident as a whole), one warm-up pair and then `--pairs` pairs per slice size; per call `peak_bytes` (the pool
after a trim), `slice_bytes_peak` (with the knob on it counts the upload's ring too) and the phases, and a summary with the median and
the min .. max of each setting.  With a library that does not know the knob (an older build, BWTM_LIB) only the off calls run: the
same lines, for comparing the default path across builds.  At the end one call per setting runs with the copying sink: the two results
must be equal byte for byte, and equal to the one-shot call's (`# verified`).  --reads-a N: input a of N reads instead of --reads (an asymmetric merge, BASELINE config 4's
shape)."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--reads-a", type=int, default=0)
    ap.add_argument("--readlen", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slices", default=None)
    ap.add_argument("--stream-upload", action="store_true")
    ap.add_argument("--warm-only", action="store_true", help="no bwtm_trim and no cold call before the timed one: ms_after_trim and peak_bytes are not measured")
    args = ap.parse_args()
    if args.slices is None:
        args.slices = "0" if args.stream_upload else "262144,1048576,4194304,0"
    import numpy as np
    import torch
    import _pkg
    pkg = _pkg.load()
    from bwt_merge_amd import synth
    capi = pkg.capi
    pkg.init(0)
    dev = torch.device("cuda", 0)
    host_in, meta = [], []
    t0 = time.time()
    for seed in (1001, 1002):
        ix = synth.build_index(pkg, seed, args.reads_a if (seed == 1001 and args.reads_a) else args.reads, args.readlen, device=dev)
        ix.encode()
        hb = pkg.HostBuffer(ix.nbytes)
        ix.download_into(hb.array)
        meta.append((ix.sequences, ix.bases))
        ix.free()
        host_in.append(hb)
    torch.cuda.empty_cache(); pkg.trim()
    a = (host_in[0].array, meta[0][0], meta[0][1]); b = (host_in[1].array, meta[1][0], meta[1][1])
    print("# inputs: %d + %d reads of %d: %d + %d bases, %d + %d bytes (%.0f s)" % (args.reads_a or args.reads, args.reads, args.readlen, meta[0][1], meta[1][1], host_in[0].nbytes, host_in[1].nbytes,
                                                                                time.time() - t0), flush=True)
    buffers = {}
    for _ in range(args.warmup):                                         # page-locked output buffers, the pool, the link (bench.py's warmup)
        res = pkg.merge_host(a, b, samples=2, buffers=buffers)
    out_bytes = res.out.nbytes
    result = pkg.HostBuffer(out_bytes + 64)
    lib = capi.lib()

    def one_shot():
        pkg.trim(); pkg.device_bytes_peak(reset=True)
        t = time.perf_counter()
        pkg.merge_host(a, b, samples=2, buffers=buffers)
        cold = (time.perf_counter() - t) * 1e3
        peak = pkg.device_bytes_peak()
        t = time.perf_counter()
        r = pkg.merge_host(a, b, samples=2, buffers=buffers)
        dt = (time.perf_counter() - t) * 1e3
        return {"call": "one_shot", "ms": round(dt, 1), "ms_after_trim": round(cold, 1), "peak_bytes": peak, "phases_ms": {k: round(v, 1) for k, v in r.times.items()}}

    def streamed(slice_records, copy):
        seen = [0, 0]

        def on_piece(user, piece):
            p = piece.contents
            if copy and p.nbytes:
                ctypes.memmove(result.ptr + p.byte_first, p.data, p.nbytes)
            seen[0] += 1; seen[1] += p.nbytes
            return 0

        cb = capi.PIECE_FN(on_piece)
        ha, hb_ = capi._host_input(*a), capi._host_input(*b)
        out, stats = capi.HostOutput(), capi.StreamStats()
        cold, peak = 0.0, 0
        if not args.warm_only:
            pkg.trim(); pkg.device_bytes_peak(reset=True)
            t = time.perf_counter()
            capi.check(lib.bwtm_merge_host_streamed(None, ctypes.byref(ha), ctypes.byref(hb_), slice_records, 2, cb, None, ctypes.byref(out), ctypes.byref(stats)))
            cold = (time.perf_counter() - t) * 1e3
            peak = pkg.device_bytes_peak()
        t = time.perf_counter()
        capi.check(lib.bwtm_merge_host_streamed(None, ctypes.byref(ha), ctypes.byref(hb_), slice_records, 2, cb, None, ctypes.byref(out), ctypes.byref(stats)))
        dt = (time.perf_counter() - t) * 1e3
        assert seen[1] == (1 if args.warm_only else 2) * out.nbytes and out.nbytes == out_bytes
        return {"call": "streamed", "sink": "copy" if copy else "count", "slice_records_asked": slice_records, "slice_records": int(stats.slice_records), "ms": round(dt, 1),
                "ms_after_trim": round(cold, 1), "peak_bytes": peak, "slice_bytes_peak": int(stats.slice_bytes_peak), "pieces": int(stats.pieces) ,
                "phases_ms": {"upload": round(stats.ms_upload, 1), "search": round(stats.ms_search, 1), "second_half": round(stats.ms_second_half, 1)}}

    rows = []
    if args.stream_upload:
        stream_upload_pairs(pkg, args, streamed, result, out_bytes, buffers[0].array)
        return
    for sr in [int(x) for x in args.slices.split(",")]:
        for _ in range(args.pairs):
            for rec in (one_shot(), streamed(sr, False), streamed(sr, True)):
                rec["slice_records_asked"] = sr
                rows.append(rec)
                print(json.dumps(rec), flush=True)
    # the copied result is the one-shot call's
    assert np.array_equal(result.array[:out_bytes], buffers[0].array[:out_bytes])
    print("# summary: mean ms on the warm pool (min .. max), second half of the fastest call, peak GB of the pool after a trim, per slice size asked for")
    for sr in sorted({r["slice_records_asked"] for r in rows}):
        for kind in (("one_shot", None), ("streamed", "count"), ("streamed", "copy")):
            sel = [r for r in rows if r["slice_records_asked"] == sr and r["call"] == kind[0] and r.get("sink") == kind[1]]
            ms = [r["ms"] for r in sel]
            fastest = min(sel, key=lambda r: r["ms"])["phases_ms"]
            half = fastest["second_half"] if kind[0] == "streamed" else fastest["ms_interleave"] + fastest["ms_encode_download"] + fastest["ms_samples"]
            print("# slice %9d  %-8s %-5s  %7.1f ms (%7.1f .. %7.1f)  second half %6.1f  peak %6.2f GB  %s" % (
                sr, kind[0], kind[1] or "", sum(ms) / len(ms), min(ms), max(ms), half, max(r["peak_bytes"] for r in sel) / 1e9,
                ("slices of %d records, %d pieces, %.3f GB of slices" % (sel[0]["slice_records"], sel[0]["pieces"], max(r["slice_bytes_peak"] for r in sel) / 1e9)) if kind[0] == "streamed" else ""))


def stream_upload_pairs(pkg, args, streamed, result, out_bytes, one_shot_bytes):
    try:
        pkg.tune("stream_upload", 0)
        settings = (0, 1)
    except pkg.BwtmError:
        settings = (0,)
        print("# this library has no stream_upload knob: the off calls only", flush=True)
    rows = []
    try:
        for sr in [int(x) for x in args.slices.split(",")]:
            for pair in range(-1, args.pairs):                            # pair -1 warms up
                for knob in settings:
                    if len(settings) > 1:
                        pkg.tune("stream_upload", knob)
                    rec = streamed(sr, False)
                    rec["stream_upload"] = knob; rec["slice_records_asked"] = sr; rec["warmup"] = (pair < 0)
                    rows.append(rec)
                    print(json.dumps(rec), flush=True)
        if len(settings) > 1:
            # the result with the knob on is the result with the knob off
            streamed(0, True)
            off = result.array[:out_bytes].copy()
            result.array[:out_bytes] = 0
            pkg.tune("stream_upload", 1)
            streamed(0, True)
            same = bool((result.array[:out_bytes] == off).all()) and bool((off == one_shot_bytes[:out_bytes]).all())
            print("# verified: the %d bytes delivered with stream_upload on equal those with it off and the one-shot call's: %s" % (out_bytes, same), flush=True)
            assert same
    finally:
        if len(settings) > 1:
            pkg.tune("stream_upload", 0)
    print("# summary: median ms on the warm pool (min .. max) and upload phase of the median call, peak GB of the pool after a trim, GB of slices + ring")
    for sr in sorted({r["slice_records_asked"] for r in rows}):
        for knob in settings:
            sel = sorted((r for r in rows if r["slice_records_asked"] == sr and r["stream_upload"] == knob and not r["warmup"]), key=lambda r: r["ms"])
            mid = sel[len(sel) // 2]
            print("# slice %9d  stream_upload %d  %7.1f ms (%7.1f .. %7.1f)  upload %6.1f  peak %6.2f GB  slices + ring %.3f GB" % (
                sr, knob, mid["ms"], sel[0]["ms"], sel[-1]["ms"], mid["phases_ms"]["upload"], max(r["peak_bytes"] for r in sel) / 1e9,
                max(r["slice_bytes_peak"] for r in sel) / 1e9))


if __name__ == "__main__":
    main()
