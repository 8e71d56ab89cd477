"""One family of GPU parity cases in a process of its own: the child that tests/test_gpu_poisoned_pool.py starts (not a test module).
Usage: python poison_child.py FAMILY

The library reads BWTM_POOL_POISON (and the pool's other variables) once per process, so the parent sets the environment and starts one
child per case.  Every family compares bit for bit with the CPU oracle; the larger input runs first and a smaller, differently shaped one
after it, so that the second one's buffers are cut from recycled blocks whose tails hold the first one's bytes or the poison.  The checks
are the suite's own helpers (and, where a test's body is the check, the test function itself, called with the library and the oracle in
place of its fixtures).  The last lines on stdout are "POISON fills=<n> bytes=<n>" (bwtm_pool_poison_stats) and "OK"."""
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

READS = ((1001, 3000, 100), (1002, 2500, 100))          # the `reads` pair: 303 000 + 252 500 positions
SMALL = ((1003, 300, 30), (1004, 7, 5))


def pair(orc, spec):
    ta = orc.generate_reads(*spec[0]); tb = orc.generate_reads(*spec[1])
    return orc.FMI.from_text(ta), orc.FMI.from_text(tb)


def upload(pkg, f):
    return pkg.Index.upload(f.data, f.sequences, f.bases)


def check_merged(pkg, orc, M, m, a, b):
    """Bytes, C, both forms of the samples of a merged index against the oracle's merge m."""
    from parts_inputs import check_against_oracle
    assert (M.sequences, M.bases, M.nbytes, M.blocks) == (m.sequences, m.bases, m.nbytes, m.blocks)
    assert np.array_equal(M.C, m.C)
    be, cum = M.samples()
    check_against_oracle(orc, a, b, M.data(), be, cum[:, :-1])
    obe, ocum = m.samples
    assert np.array_equal(cum, ocum)
    width, fields, anchors = M.samples_compact()
    if width != 8:
        xbe, xcum = pkg.capi.expand_samples(width, fields, anchors, M.blocks, M.bases)
        assert np.array_equal(xbe, obe) and np.array_equal(xcum, ocum)


def merge_path(pkg, orc, a, b, queries):
    """upload x 2, bwtm_merge under every dispatch of the search, the rank array's runs, and the queries on the merged index."""
    from test_gpu_parity import check_index
    m, _ = orc.merge(a.clone(), b.clone(), threads=2)
    searched = (a.sequences > 0 and b.sequences > 0)
    if searched:
        oranks, ocounts, _ = orc.search(a, b, threads=2)
    A, B = upload(pkg, a), upload(pkg, b)
    try:
        for algo, ratio in ((2, 0), (2, -1), (1, -1), (0, -1)):
            pkg.tune("search_algo", algo); pkg.tune("range_ratio", ratio)
            M = pkg.merge(A, B)
            check_merged(pkg, orc, M, m, a, b)
            if searched:
                ra = pkg.RankArray(A, B)
                ra.search(A, B, 0, b.sequences - 1)
                ra.finalize()
                assert ra.values == b.bases
                ranks, counts = ra.runs()
                assert np.array_equal(ranks, oranks) and np.array_equal(counts, ocounts), (algo, ratio)
                ra.free()
            if queries and algo == 2:
                rng = np.random.default_rng(3)
                check_index(M, m.symbols, rng, nq=2000)
                check_find(orc, M, m, rng)
            M.free()
    finally:
        pkg.tune("search_algo", 0); pkg.tune("range_ratio", -1)
    A.free(); B.free()


def check_find(orc, M, m, rng):
    """bwtm_find_batch against the oracle's backward search: pieces of the merged stream and random patterns."""
    sym = m.symbols
    pats = [np.zeros(0, dtype=np.uint8)]
    for _ in range(100):
        p = int(rng.integers(0, max(sym.size - 30, 1)))
        s = sym[p:p + int(rng.integers(1, 25))]
        pats.append(s[s != 0][:20] if rng.random() < 0.7 else rng.integers(1, 6, int(rng.integers(1, 12))).astype(np.uint8))
    sp, ep = M.find(pats)
    for k, p in enumerate(pats):
        osp, oep = orc.FMI.find(m, p)
        empty_o = (osp + 1) % (1 << 64) > (oep + 1) % (1 << 64)
        empty_g = (int(sp[k]) + 1) % (1 << 64) > (int(ep[k]) + 1) % (1 << 64)
        assert empty_o == empty_g, k
        assert empty_o or (int(sp[k]), int(ep[k])) == (osp, oep), k


def family_reads(pkg, orc):
    for spec in (READS, SMALL):
        a, b = pair(orc, spec)
        merge_path(pkg, orc, a, b, queries=True)


def family_odd(pkg, orc):
    from parts_inputs import ODD_CASES, odd_collection, truly_empty
    for case in ODD_CASES:
        ta, tb = odd_collection(case)
        merge_path(pkg, orc, orc.FMI.from_text(ta), orc.FMI.from_text(tb), queries=False)
    for which in ("a", "b"):
        a, b = truly_empty(orc, which)
        merge_path(pkg, orc, a, b, queries=False)


def ragged(n):
    """n positions end inside a record, an interleave chunk, an encoder tile / chunk / segment and every transcode window."""
    return all(n % unit != 0 for unit in (64, 128, 4096, 8192, 16384, 32768, 65536))


def family_runs(pkg, orc):
    """k_build_recs (both deposits, all three LDS windows), the rank structure, and the encoder on the records alone."""
    from test_gpu_parity import check_index, run_symbols
    rng = np.random.default_rng(1)
    # the stream beyond a super block first (> 2^25 positions), then the three length sets of upload_cases: dense, long windows, giant runs
    streams = [run_symbols(rng, 200000, [1, 2, 3, 50, 400, 1500]), run_symbols(rng, 60000, [1, 1, 1, 2, 3]),
               run_symbols(rng, 8000, [5, 20, 42, 60, 83, 90, 168, 169, 170, 400]), run_symbols(rng, 300, [3, 8, 40000, 14, 70000, 21])]
    assert streams[0].size > (1 << 25) + 1000
    for k, sym in enumerate(streams):
        if not ragged(sym.size):
            sym = sym[:-1]
        assert ragged(sym.size)
        f = orc.FMI.from_symbols(sym)
        obe, ocum = f.samples
        for deposit in ((0,) if k == 0 else (0, 1, -1)):
            pkg.tune("recs_uniform", deposit)
            try:
                ix = upload(pkg, f)
            finally:
                pkg.tune("recs_uniform", 0)
            assert (ix.sequences, ix.nbytes, ix.blocks) == (f.sequences, f.nbytes, f.blocks) and np.array_equal(ix.C, f.C)
            check_index(ix, sym, rng, nq=2000)
            be, cum = ix.samples()
            assert np.array_equal(be, obe) and np.array_equal(cum, ocum)
            ix.drop_native()
            ix.encode()
            assert ix.nbytes == f.nbytes and np.array_equal(ix.data(), f.data)
            be, cum = ix.samples()
            assert np.array_equal(be, obe) and np.array_equal(cum, ocum)
            ix.free()


def family_encoder(pkg, orc):
    """from_symbols_device + encode + samples: the `halves` streams of test_encoder_block_rule cut to 2 * 10^5 runs, its second `giant`
    stream, then its `tiny` list."""
    import torch
    from test_gpu_parity import run_symbols
    rng = np.random.default_rng(11)
    syms = [run_symbols(rng, 200000, [1, 1, 1, 1, 2, 42, 43, 44, 50, 63, 64, 65]), run_symbols(rng, 200000, [1] * 40 + [42, 83, 200]),
            run_symbols(rng, 200000, [1] * 12 + [2, 3, 31, 32, 33, 42, 52, 62, 82, 83, 90, 1000, 70000]),
            np.concatenate([np.full(70000, 1, np.uint8), np.full(1, 2, np.uint8), np.full(4096 * 64 * 16 + 5, 4, np.uint8)])]
    syms += [np.array([4], np.uint8), np.array([0, 0], np.uint8), np.full(63, 2, np.uint8), np.full(64, 2, np.uint8), np.full(4096, 5, np.uint8),
             run_symbols(rng, 3, [1])] + [run_symbols(rng, 40, [1, 2])[:k] for k in (64, 127, 128, 129)]
    for sym in syms:
        f = orc.FMI.from_symbols(sym)
        d = torch.from_numpy(sym).cuda()
        torch.cuda.synchronize()
        ix = pkg.Index.from_symbols_device(d.data_ptr(), sym.size)
        assert ix.sequences == f.sequences and np.array_equal(ix.C, f.C), sym.size
        ix.encode()
        assert ix.nbytes == f.nbytes and np.array_equal(ix.data(), f.data), sym.size
        be, cum = ix.samples(); obe, ocum = f.samples
        assert np.array_equal(be, obe) and np.array_equal(cum, ocum), sym.size
        ix.free()


def family_epochs(pkg, orc):
    """The frontier search across epoch boundaries (tiles built every 7 steps), and level-1 regions that overflow into the exact fallbacks."""
    from test_gpu_branches import test_frontier_epoch_rollover
    test_frontier_epoch_rollover(pkg, orc, 7, 0, 0)
    test_frontier_epoch_rollover(pkg, orc, 7, 0, -1)
    a, b = pair(orc, READS)
    oranks, ocounts, _ = orc.search(a, b, threads=2)
    A, B = upload(pkg, a), upload(pkg, b)
    pkg.tune("search_algo", 2); pkg.tune("l1_cap", 5000)
    try:
        ra = pkg.RankArray(A, B)
        ra.search(A, B, 0, b.sequences - 1)
        ra.finalize()
        ranks, counts = ra.runs()
        assert ra.values == b.bases and np.array_equal(ranks, oranks) and np.array_equal(counts, ocounts)
        ra.free()
    finally:
        pkg.tune("search_algo", 0); pkg.tune("l1_cap", 0)


def family_host(pkg, orc):
    from test_gpu_branches import test_host_to_host_merge, test_pipelined_chain_of_host_merges
    test_host_to_host_merge(pkg, orc, (1, 1))
    test_host_to_host_merge(pkg, orc, (8192, 4096))
    test_pipelined_chain_of_host_merges(pkg, orc, 4096)


def family_slices(pkg, orc):
    from test_gpu_slices import test_range_finalize_after_a_reduce_scatter, test_sliced_merge_of_read_sets
    test_range_finalize_after_a_reduce_scatter(pkg, orc, 3)
    test_sliced_merge_of_read_sets(pkg, orc, 3)


def family_parts(pkg, orc):
    """Three parts as threads; then two merges of different sizes through ONE group, the larger first: the second merge's exported buffers
    are the first one's arena, reused."""
    from bwt_merge_amd import capi, partitioned
    from parts_inputs import check_against_oracle
    from test_gpu_parts import host, merge_parts
    big, small = pair(orc, READS), pair(orc, ((1005, 900, 45), (1006, 400, 70)))
    for rr in (0, 8):
        pkg.tune("range_ratio", rr)
        try:
            data, be, cum, _, _ = merge_parts(pkg, big[0], big[1], 3, 3)
        finally:
            pkg.tune("range_ratio", 8)
        check_against_oracle(orc, big[0], big[1], data, be, cum)
    parts = 3
    name = partitioned.unique_group_name("poison")
    ctxs = [pkg.Context(0) for _ in range(parts)]
    results = [[None] * parts for _ in range(2)]
    errors = []

    def worker(g):
        try:
            ctxs[g].make_current()
            group = capi.Group(name, g, parts)
            for k, (a, b) in enumerate((big, small)):
                S, _ = partitioned.merge_part(group, host(pkg, a), host(pkg, b), kmer=3)
                results[k][g] = partitioned.slice_arrays(S)
                S.free()
            group.free()
        except Exception as e:                                          # noqa: BLE001
            errors.append(e)
            raise

    threads = [threading.Thread(target=worker, args=(g,)) for g in range(parts)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    pkg.make_default_current()
    for c in ctxs:
        c.destroy()
    assert not errors, errors
    for k, (a, b) in enumerate((big, small)):
        r = results[k]
        check_against_oracle(orc, a, b, np.concatenate([x[0] for x in r]), np.concatenate([x[1] for x in r]), np.concatenate([x[2] for x in r], axis=1))


def family_ingest(pkg, orc):
    from test_gpu_ingest import test_iid_reads_match_brute_force, test_ragged_duplicate_and_empty_reads
    pkg.tune("ingest_verify", 1)
    try:
        test_ragged_duplicate_and_empty_reads(pkg, orc)
        test_iid_reads_match_brute_force(pkg, orc, 300, 30, 0)
        test_iid_reads_match_brute_force(pkg, orc, 300, 30, 64)
    finally:
        pkg.tune("ingest_verify", 0)


def family_exact_builders(pkg, orc):
    """Every single-index builder on every small stream whose size is on a record, group, chunk or segment edge (tests/boundary_inputs.py):
    a last record, a last chunk or a last super row that nobody wrote holds the poison, not a zero."""
    import boundary_inputs as bi
    from test_gpu_exact_sizes import BUILDERS, check_small_builder
    for kind, n in bi.SMALL_STREAMS:
        for builder in BUILDERS:
            check_small_builder(pkg, orc, kind, n, builder)


def family_exact_merges(pkg, orc):
    """Every form of the merge at every exact n_out under both dispatches of the search, the consumers included."""
    import boundary_inputs as bi
    from test_gpu_exact_sizes import FORMS, PairCase, check_input_consumers, check_merge_form
    for name in bi.READ_PAIRS:
        case = PairCase(pkg, orc, name)
        for form in FORMS:
            for algo in (1, 2):
                check_merge_form(pkg, orc, case, form, algo, consumers=(algo == 2))
        check_input_consumers(pkg, case)
        case.free()
        pkg.trim()


def family_transcode_forms(pkg, orc):
    """k_build_recs and k_build_recs_chunk forced onto streams they are not chosen for (tests/test_gpu_transcode_forms.py): the smallest and
    the largest window, both deposits, through the one-shot and the chunked upload.  A small window over a giant group reads more of blen,
    the group tables and the records per wave than any other case; the form counter shows that the setting took effect."""
    from test_gpu_transcode_forms import case, check_setting
    for name in ("giants_with_dense", "edges_8192"):
        c = case(orc, name)
        for window, uniform in ((8192, -1), (8192, 1), (32768, -1), (32768, 1)):
            for entry in ("upload", "streamed_1"):
                check_setting(pkg, c, window, uniform, entry)


FAMILIES = {"reads": family_reads, "odd": family_odd, "runs": family_runs, "encoder": family_encoder, "epochs": family_epochs, "host": family_host,
            "slices": family_slices, "parts": family_parts, "ingest": family_ingest, "exact_builders": family_exact_builders,
            "exact_merges": family_exact_merges, "transcode_forms": family_transcode_forms}


def main(family):
    import _pkg
    from oracle import oracle as orc
    pkg = _pkg.load()
    pkg.init(0)
    FAMILIES[family](pkg, orc)
    pkg.make_default_current()
    pkg.synchronize()
    print("POISON fills=%d bytes=%d" % pkg.pool_poison_stats())
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1])
