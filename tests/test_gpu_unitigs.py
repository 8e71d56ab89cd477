"""The unitigs of the k-mer graph on the GPU (bwtm_unitigs_*; Kmers.unitigs).  Every result is compared byte for byte -- offsets, text,
nodes, occurrences, flags, links, and the place of every node -- with the brute force of tests/unitig_inputs.py, which restates the rule
of include/bwtm.h over Python sets and never uses the library (tests/test_unitigs_host.py checks it on its own)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from kmer_inputs import genome_reads, text_of
from unitig_inputs import CIRCULAR, COLLECTIONS, HAND, NONE, Graph, case, table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GUARD = 4096


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    yield bwtm
    bwtm.tune("unitig_launch", 0)


def uploaded(pkg, oracle, rows):
    f = oracle.FMI.from_text(text_of(list(rows)))
    assert f.sequences == len(rows)
    return pkg.Index.upload(f.data, f.sequences, f.bases)


def built(pkg, oracle, name, t=None, min_count=1):
    """(Unitigs, Graph) of a case of tests/unitig_inputs.py; the k-mer handle is freed before the graph is used."""
    rows, k, t0, skip, g = case(name)
    x = uploaded(pkg, oracle, rows)
    km = x.kmers(k, skip=skip, min_count=min_count)
    u = km.unitigs(t0 if t is None else t, skip=skip)
    km.free(); x.free()
    return u, g


def absent_codes(g, n=200, seed=5):
    """Codes that are no nodes: random ones below 4^k, the neighbours of nodes, 0 and the largest code, and for k < 32 codes of 4^k and more."""
    top = (1 << (2 * g.k)) - 1
    rng = np.random.default_rng(seed)
    picks = [int(v) & top for v in rng.integers(0, 1 << 63, size=n, dtype=np.uint64)] + [0, top] + [min(x + 1, top) for x in g.nodes[:50]]
    if g.k < 32:
        picks += [top + 1, (1 << 64) - 1, (top + 1) | (g.nodes[0] if g.nodes else 0)]
    solid = set(g.nodes)
    return np.array([c for c in picks if c not in solid], dtype=np.uint64)


def same(pkg, u, g):
    """Everything the handle gives against the brute force."""
    assert (u.count, u.nodes, u.symbols, u.k) == (g.U, g.S, g.symbols, g.k)
    got, want = u.download(), g.arrays()
    for name, a, b in zip(("offsets", "text", "nodes", "occurrences", "flags", "links"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a.ravel(), b), (name, np.flatnonzero(a.ravel()[: b.size] != b[: a.size])[:10])
    codes = np.concatenate([np.array(g.nodes, dtype=np.uint64), absent_codes(g)])
    pu, po = u.place(codes)
    wu, wo = g.place(codes)
    assert np.array_equal(pu, wu) and np.array_equal(po, wo)
    assert (pu[g.S:] == NONE).all() and (po[g.S:] == NONE).all()


@pytest.mark.parametrize("name", list(HAND) + list(COLLECTIONS))
def test_every_case_against_the_brute_force(gpu, oracle, name):
    u, g = built(gpu, oracle, name)
    stats = gpu.unitigs_stats()
    same(gpu, u, g)
    assert stats["longest"] == g.longest and stats["circular_nodes"] == g.circular_nodes
    assert stats["lookups"] == 5 * g.S + sum(1 for unitig in g.unitigs if not unitig[3] & CIRCULAR)     # a circular unitig's links need no lookup
    cycles = sorted(n for _, n, _, f, _ in g.unitigs if f & CIRCULAR)
    assert stats["jump_rounds"] == (int(np.ceil(np.log2(sum(cycles)))) if cycles else 0)
    u.free()


def test_sizes_of_the_collections(gpu, oracle):
    for name, want in (("genome_k12_t3", (2977, 4, 1470)), ("genome_k12_t1", (9218, 1550, None)), ("iid_k12_t1", (51433, 2802, None)), ("iid_k6_t1", (4096, 4096, 1))):
        u, g = built(gpu, oracle, name)
        assert (u.nodes, u.count) == want[:2] and (want[2] is None or gpu.unitigs_stats()["longest"] == want[2])
        u.free()


def test_several_launches_per_phase_give_the_same_graph(gpu, oracle):
    """bwtm_tune("unitig_launch"): 1 000 nodes per launch, so that every one-lane-per-node kernel runs in parts, as beyond 2^31 nodes."""
    gpu.tune("unitig_launch", 1000)
    try:
        for name in ("iid_k12_t1", "long_cycle", "genome_k12_t1"):
            u, g = built(gpu, oracle, name)
            same(gpu, u, g)
            u.free()
    finally:
        gpu.tune("unitig_launch", 0)


def test_threshold_above_every_count_gives_an_empty_graph(gpu, oracle):
    u, g = built(gpu, oracle, "genome_k12_t3", t=10 ** 6)
    assert (u.count, u.nodes, u.symbols) == (0, 0, 0)
    got = u.download()
    assert got[0].tolist() == [0] and all(a.size == 0 for a in got[1:])
    assert all(a.size == 0 for a in u.download(0, 0)[1:])
    pu, po = u.place(np.array(g.nodes[:10], dtype=np.uint64))
    assert (pu == NONE).all() and (po == NONE).all()
    assert gpu.unitigs_stats() == {"lookups": 0, "longest": 0, "circular_nodes": 0, "jump_rounds": 0}
    with pytest.raises(gpu.BwtmError, match="beyond the 0 unitigs"):
        u.download(0, 1)
    u.free()
    # no k-mer in the handle at all
    rows, k, _, skip, _ = case("genome_k12_t3")
    x = uploaded(gpu, oracle, rows)
    u = x.kmers(k, min_count=10 ** 6).unitigs(1)
    assert (u.count, u.nodes) == (0, 0) and u.download()[0].tolist() == [0]
    u.free(); x.free()


def test_kmers_created_with_a_min_count_above_the_threshold(gpu, oracle):
    rows, k, _, skip, _ = case("genome_k12_t1")
    u, _ = built(gpu, oracle, "genome_k12_t1", t=2, min_count=4)
    g = Graph(table_of(rows, k, skip), k, 4, skip)
    assert g.S not in (0, case("genome_k12_t3")[4].S)
    same(gpu, u, g)
    u.free()
    u, _ = built(gpu, oracle, "genome_k12_t1", t=0)                                # 0 is taken as 1
    same(gpu, u, case("genome_k12_t1")[4])
    u.free()


def raw(gpu):
    from bwt_merge_amd import capi
    return capi, capi.lib()


def guarded(nbytes):
    return np.full(nbytes + 2 * GUARD, 0xA5, dtype=np.uint8)


def ptr(buf, ctype):
    return C.cast(C.c_void_p(buf.ctypes.data + GUARD), C.POINTER(ctype))


def inner(buf, dtype, n):
    return buf[GUARD: GUARD + n * np.dtype(dtype).itemsize].view(dtype)


def untouched(*bufs):
    return all((b == 0xA5).all() for b in bufs)


def test_sliced_downloads_and_null_outputs(gpu, oracle):
    capi, lib = raw(gpu)
    u, g = built(gpu, oracle, "genome_k12_t1")
    U = g.U
    names = ("offsets", "text", "nodes", "occurrences", "flags", "links")
    windows = [(0, 1), (1, 499), (500, 0), (500, 1049), (1549, 1), (1550, 0)]
    assert sum(c for _, c in windows) == U
    parts = {n: [] for n in names}
    for w, (first, count) in enumerate(windows):
        want = g.arrays(first, count)
        sizes = {"offsets": 8 * (count + 1), "text": int(want[0][-1]) + 7, "nodes": 8 * count, "occurrences": 8 * count, "flags": count, "links": 32 * count}
        # the sizing call fills everything but the text
        bufs = {n: guarded(sizes[n]) for n in names}
        capi.check(lib.bwtm_unitigs_download(u.h, first, count, ptr(bufs["offsets"], C.c_uint64), ptr(bufs["text"], C.c_uint8) if w % 2 else None, 0 if w % 2 else 99,
                                             ptr(bufs["nodes"], C.c_uint64), ptr(bufs["occurrences"], C.c_uint64), ptr(bufs["flags"], C.c_uint8), ptr(bufs["links"], C.c_uint64)))
        assert untouched(bufs["text"]) and np.array_equal(inner(bufs["offsets"], np.uint64, count + 1), want[0])
        assert np.array_equal(inner(bufs["links"], np.uint64, 4 * count), want[5])
        # every output alone and all of them together: nothing outside the arrays is written
        for only in names + (None,):
            bufs = {n: guarded(sizes[n]) for n in names}
            args = [ptr(bufs[n], C.c_uint8 if n in ("text", "flags") else C.c_uint64) if only in (n, None) else None for n in names]
            capi.check(lib.bwtm_unitigs_download(u.h, first, count, args[0], args[1], sizes["text"], args[2], args[3], args[4], args[5]))
            for j, n in enumerate(names):
                if only not in (n, None):
                    assert untouched(bufs[n]), (only, n)
                    continue
                dtype = np.uint8 if n in ("text", "flags") else np.uint64
                assert np.array_equal(inner(bufs[n], dtype, want[j].size), want[j]), (first, count, n)
                assert (bufs[n][:GUARD] == 0xA5).all() and (bufs[n][GUARD + want[j].nbytes:] == 0xA5).all(), (first, count, n)
        got = u.download(first, count)
        for n, a in zip(names, got):
            parts[n].append(a.ravel())
    whole = g.arrays()
    glued, base = [0], 0
    for p in parts["offsets"]:                                                                    # every window's offsets start at 0
        glued += (p[1:] + np.uint64(base)).tolist(); base += int(p[-1])
    assert glued == whole[0].tolist()
    for j, n in enumerate(names[1:], 1):
        assert np.array_equal(np.concatenate(parts[n]), whole[j]), n
    u.free()


def test_refused_calls_name_the_offender_and_write_nothing(gpu, oracle):
    capi, lib = raw(gpu)
    rows, k, t, skip, g = case("genome_k12_t3")
    x = uploaded(gpu, oracle, rows)
    km = x.kmers(k)
    out = capi.vp()

    def refused(rc, what):
        assert rc != 0 and what in lib.bwtm_last_error().decode(), (rc, lib.bwtm_last_error().decode())

    refused(lib.bwtm_unitigs_create(None, 5, 3, C.byref(out)), "bwtm_unitigs_create: null argument")
    refused(lib.bwtm_unitigs_create(km.h, 5, 3, None), "bwtm_unitigs_create: null argument")
    refused(lib.bwtm_unitigs_create(km.h, 0, 3, C.byref(out)), "skip = 0 is no comp value")
    refused(lib.bwtm_unitigs_create(km.h, 6, 3, C.byref(out)), "skip = 6 is no comp value")
    assert not out.value
    u = km.unitigs(t)
    km.free(); x.free()
    U = g.U
    assert U == 4
    want = g.arrays()
    names = ("offsets", "text", "nodes", "occurrences", "flags", "links")
    bufs = {n: guarded(64 * 1024) for n in names}
    args = [ptr(bufs[n], C.c_uint8 if n in ("text", "flags") else C.c_uint64) for n in names]

    def download(first, count, capacity):
        return lib.bwtm_unitigs_download(u.h, first, count, args[0], args[1], capacity, args[2], args[3], args[4], args[5])

    refused(lib.bwtm_unitigs_download(None, 0, 1, args[0], args[1], 64 * 1024, args[2], args[3], args[4], args[5]), "bwtm_unitigs_download: null argument")
    refused(download(0, U + 1, 64 * 1024), "unitigs 0 + 5 lie beyond the 4 unitigs")
    refused(download(U + 1, 0, 64 * 1024), "unitigs 5 + 0 lie beyond the 4 unitigs")
    refused(download(2, (1 << 64) - 1, 64 * 1024), "lie beyond the 4 unitigs")                   # first + count wraps to 1
    refused(download(3, 2, 64 * 1024), "unitigs 3 + 2 lie beyond the 4 unitigs")
    refused(download(0, U, int(want[0][-1]) - 1), "capacity %d is too small (%d bytes of text)" % (int(want[0][-1]) - 1, int(want[0][-1])))
    refused(download(1, 2, 1), "capacity 1 is too small (%d bytes of text)" % int(want[0][3] - want[0][1]))
    assert untouched(*bufs.values())
    capi.check(download(0, U, int(want[0][-1])))                                                  # the exact capacity is enough
    assert np.array_equal(inner(bufs["text"], np.uint8, want[1].size), want[1])
    codes = np.array(g.nodes[:5], dtype=np.uint64)
    pu, po = guarded(40), guarded(40)
    refused(lib.bwtm_unitigs_place(None, codes.ctypes.data_as(capi.p_u64), 5, ptr(pu, C.c_uint64), ptr(po, C.c_uint64)), "bwtm_unitigs_place: null argument")
    refused(lib.bwtm_unitigs_place(u.h, None, 5, ptr(pu, C.c_uint64), ptr(po, C.c_uint64)), "bwtm_unitigs_place: null argument")
    assert untouched(pu, po)
    capi.check(lib.bwtm_unitigs_place(u.h, None, 0, None, None))
    capi.check(lib.bwtm_unitigs_place(u.h, codes.ctypes.data_as(capi.p_u64), 5, None, ptr(po, C.c_uint64)))     # either output may be NULL
    assert untouched(pu) and np.array_equal(inner(po, np.uint64, 5), g.place(codes)[1]) and (po[GUARD + 40:] == 0xA5).all()
    refused(lib.bwtm_unitigs_stats(None), "bwtm_unitigs_stats: null argument")
    assert lib.bwtm_unitigs_count(None) == 0 and lib.bwtm_unitigs_nodes(None) == 0 and lib.bwtm_unitigs_symbols(None) == 0
    assert lib.bwtm_unitigs_bytes(None) == 0 and lib.bwtm_unitigs_k(None) == 0
    lib.bwtm_unitigs_free(None)
    u.free()
    with pytest.raises(gpu.BwtmError, match="freed"):
        u.download()


def test_two_runs_give_equal_bytes(gpu, oracle):
    for name in ("iid_k12_t1", "long_cycle"):
        runs = []
        for _ in range(2):
            u, g = built(gpu, oracle, name)
            runs.append(u.download() + u.place(np.array(g.nodes, dtype=np.uint64)))
            u.free()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))


def handle_bytes(g):
    """H of include/bwtm.h."""
    D = min(2 * g.k, 24, max(1, int(np.ceil(np.log2(max(g.S, 1))))))
    return 8 * max(g.S, 1) + 8 * (2 ** D + 1) + 16 * g.S + 57 * g.U + 8 + g.symbols


def peak_bound(g, n, cycle):
    """include/bwtm.h: 17/16 (H + 8 n + 25 S + 8 U + C + (n + 2 S + U) / 128) + 2^16."""
    exact = handle_bytes(g) + 8 * n + 25 * g.S + 8 * g.U + (32 * g.S if cycle else 0) + (n + 2 * g.S + g.U) // 128
    return 17 * exact // 16 + (1 << 16)


@pytest.mark.parametrize("name", ["iid_k12_t1", "long_cycle"])
def test_handle_and_device_memory_stay_within_the_documented_bounds(gpu, oracle, name):
    rows, k, t, skip, g = case(name)
    x = uploaded(gpu, oracle, rows)
    km = x.kmers(k)
    n = km.distinct
    gpu.synchronize(); gpu.trim()
    held = gpu.pool_stats()["held_bytes"]
    gpu.device_bytes_peak(reset=True)
    u = km.unitigs(t)
    peak = gpu.device_bytes_peak()
    H = handle_bytes(g)
    assert g.S > 1000 and H <= u.bytes <= 9 * (17 * H // 16 + 2560) // 8, (H, u.bytes)
    assert held + H <= peak <= held + peak_bound(g, n, g.circular_nodes > 0), (held, peak, H, peak_bound(g, n, g.circular_nodes > 0))
    same(gpu, u, g)
    u.free(); km.free(); x.free()


def test_the_graph_of_a_merged_index_and_of_both_strands(gpu, oracle):
    """An index that holds both strands gives the reverse complements: every unitig's reverse complement is a unitig too."""
    rows = list(genome_reads()[:400])
    both = rows + [(5 - r[::-1]).astype(np.uint8) for r in rows]
    x = uploaded(gpu, oracle, both)
    km = x.kmers(11)
    u = km.unitigs(2)
    g = Graph(table_of(both, 11), 11, 2)
    same(gpu, u, g)
    offsets, text = u.download()[:2]
    texts = {text[int(offsets[j]): int(offsets[j + 1])].tobytes() for j in range(u.count)}
    linear = [j for j in range(u.count) if not g.unitigs[j][3]]
    assert linear and all((5 - g.unitigs[j][0][::-1]).astype(np.uint8).tobytes() in texts for j in linear)
    u.free(); km.free(); x.free()


@pytest.mark.parametrize("word", ["0x00000000", "0xA5A5A5A5"])
def test_on_a_poisoned_pool(bwtm, word):
    """Cases with and without cycles in a fresh process whose pool hands out blocks filled with `word`: every flag, successor, start,
    offset, count, text byte and link that is read was written by the kernels."""
    env = dict(os.environ, BWTM_POOL_POISON=word)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "unitigs_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout.split(), "exit status %s\n%s%s" % (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    got = re.search(r"POISON fills=(\d+) bytes=(\d+)", out.stdout)
    assert got and int(got.group(1)) > 0 and int(got.group(2)) >= 256 * int(got.group(1)), out.stdout[-3000:]
