"""Merges at the size where the product's own dispatch runs, certified bit for bit against the read generator alone.

Every other parity test gets its expected BWT from a suffix sort on the CPU, which bounds it to a few tens of Mbase, or compares the
library with itself.  Here the increment B always holds more than 2^21 sequences, so bwtm_search picks the frontier search by size, with
the default node phase, default epochs, multi-tile segment tables and a grid that shrinks -- no knob is touched in this module -- and the
whole output (native bytes, samples, C, header counts) is certified by inversion (tests/bwt_certificate.py): decoded, re-encoded
canonically, and walked back into the 2.6 million reads the generator makes on the CPU.  The inputs come from the library's builder
(2^19-read leaves) and are not trusted: only the output is certified, and when a case fails the inputs are certified on their own first,
so the message says whether the builder or the merge is at fault.  There is no tolerance anywhere: every comparison is exact.

What the profile can and cannot show: `frontier_step`, `range_step`, `lf_walk` and `tile_build` are launch counts of the final merge alone
(the builder's own merges of 2^19-read leaves take the walk and are not counted).  The two deposits of k_build_recs run under one
profile name, `build_recs`, so the profile cannot tell that the upload of a genome stream takes the straight-line deposit by density; it
is not asserted here (tests/test_gpu_parity.py::test_upload_builds_exact_rank_structure forces both deposits at oracle size).

Measured once on the MI355X box (16 host threads; seconds; gpu = build of the inputs + merge + downloads, reads = the generator on the
CPU, certificate = decode + canonical re-encode + inversion; tile builds of the final merge are recorded, not asserted):

  case                              merged bases   gpu   reads  certificate  tile builds  frontier + node steps
  iid (2^19 + NB)                    271 835 440   0.73   0.42      3.85          1            100 + 9
    its mutant beyond row 2^28                      -      -        2.40   (rejected, names a sequence)
    oracle.merge(threads=16) of the same pair       -      -       15.42   (same bytes, samples and C)
    merge_host, samples = 1 and 2                  0.47    -     by equality with the certified stream
  mixed (2^17 + NB)                  278 085 024   0.44   0.49      4.21          2            150 + 9
  genome 300 x (2^17 + NB)           232 120 624   0.20   0.42      2.61          1             99 + 10
    merge_parts(parts=4, kmer=4)                   0.07    -     by equality with the certified stream
  genome 30 x (2^17 + NB)            232 120 624   0.20   0.39      2.57          1             99 + 10
  asymmetric (2^22 + NB)             642 507 056   0.62   0.68      9.31          1            100 + 9
  chain (4 x 2^20 mixed)             507 510 704   0.59   0.76      8.23          -               -
  builder alone, genome 300 x 2^21   211 812 352   0.17   0.51      2.48
  builder alone, mixed 2^21          253 755 352   0.29   1.02      3.85

The module took 66 s of wall time and 13.7 GB of host memory at its peak (the asymmetric case).  Budget: at most the wall time of the
slowest GPU test module of the parent commit on the same box, tests/test_gpu_bench.py with 97.4 s (then test_gpu_parts_processes.py 52.2 s,
test_gpu_experimental.py 21.3 s).  Reduced from the sizes the issue starts from to stay inside it, A sides only: iid 2^19 instead of NB
(the least that puts the output beyond 2^28 rows), mixed and genome 2^17, asymmetric 2^22 instead of 2^23; both genome coverages, the
chain and both builder cases are kept at full size, and every increment B holds more than 2^21 sequences.
"""
import resource
import time

import numpy as np
import pytest

from bwt_certificate import certify, certify_native

pytestmark = pytest.mark.gpu

NB = (1 << 21) + 70_000                      # sequences of every increment: above FRONTIER_MIN_SEQUENCES = 2^21 (csrc/api/search.hip.h)
NA = 1 << 17                                 # the base of the mixed and genome cases (reduced from NB for the time budget; B never is)
LEAF = 1 << 19


@pytest.fixture(scope="module")
def gpu(bwtm):
    bwtm.init(0)
    yield bwtm
    bwtm.profile_enable(False)
    bwtm.trim()


def expected_reads(workload, seed, nreads, **args):
    """The generator's reads of a set on the CPU: ([nreads, width] uint8 zero padded, lengths or None)."""
    import torch
    from bwt_merge_amd import synth
    step = 1 << 13                                                                       # (the generator's int64 temporaries stay in cache)
    rows = [synth.make_reads(workload, seed, first, min(step, nreads - first), 100, nreads, device="cpu", **args) for first in range(0, nreads, step)]
    lengths = synth.read_lengths(workload, 0, nreads, 100)
    return torch.cat(rows).numpy(), (None if lengths is None else lengths.numpy())


def stack_reads(sets):
    """The ordered collection of several sets: one matrix, and lengths when any set is ragged."""
    reads = np.concatenate([r for r, _ in sets])
    if all(l is None for _, l in sets):
        return reads, None
    return reads, np.concatenate([np.full(r.shape[0], r.shape[1], dtype=np.int64) if l is None else l for r, l in sets])


def build(gpu, workload, seed, nreads, **args):
    import torch
    from bwt_merge_amd import synth
    ix = synth.build_index(gpu, seed, nreads, 100, leaf_reads=LEAF, device=torch.device("cuda", 0), workload=workload, native=True, **args)
    gpu.synchronize()
    return ix


def profiled_merge(gpu, A, B):
    gpu.profile_enable(True); gpu.profile_reset()
    try:
        M = gpu.merge(A, B)
        gpu.synchronize()
        prof = gpu.profile_read()
    finally:
        gpu.profile_enable(False)
    return M, prof


def native_of(ix):
    """Everything the product hands out for an index, on the host."""
    be, cum = ix.samples()
    return dict(data=ix.data(), sequences=ix.sequences, bases=ix.bases, block_end=be, cum=cum, C=ix.C)


def verdict_of(oracle, out, reads, lengths):
    return certify_native(oracle, out["data"], out["sequences"], out["bases"], out["block_end"], out["cum"], out["C"], reads, lengths)


def report(name, **figures):
    figures["peak_host_GB"] = round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20, 1)
    print("certified[%s] %s" % (name, " ".join("%s=%s" % (k, round(v, 2) if isinstance(v, float) else v) for k, v in figures.items())))


def assert_certified(oracle, name, out, sets, inputs):
    """certify_native of a merge's output against the stacked reads of `sets`; on failure the inputs ((name, native form, set) ...) are
    certified on their own so that the message names the builder or the merge."""
    reads, lengths = stack_reads(sets)
    verdict = verdict_of(oracle, out, reads, lengths)
    if verdict is not None:
        blame = ["%s: %s" % (n, verdict_of(oracle, x, *stack_reads([s])) or "is the BWT of its reads") for n, x, s in inputs]
        pytest.fail("%s: the output is not the BWT of the generated reads: %s\n  inputs: %s" % (name, verdict, "; ".join(blame)))
    return reads, lengths


def assert_dispatch(prof, steps_at_least=100):
    """The final merge took the frontier search by size, behind the default node phase."""
    launches = lambda k: prof.get(k, (0, 0))[1]
    assert launches("frontier_step") > 0 and "lf_walk" not in prof, sorted(prof)
    assert launches("range_step") > 0, sorted(prof)
    assert launches("frontier_step") + launches("range_step") >= steps_at_least, (launches("frontier_step"), launches("range_step"))
    return launches("tile_build")


def merged_case(gpu, oracle, name, workload, na, seeds, steps_at_least, **args):
    """A (na reads) + B (NB reads) of one workload through the product's merge; -> everything the follow-up checks need."""
    t0 = time.time()
    A = build(gpu, workload, seeds[0], na, **args); B = build(gpu, workload, seeds[1], NB, **args)
    a, b = native_of(A.encode()), native_of(B.encode())               # (a builder's index holds the rank structure only)
    M, prof = profiled_merge(gpu, A, B)
    out = native_of(M)
    assert (M.sequences, M.bases) == (na + NB, a["bases"] + b["bases"])
    for x in (A, B, M):
        x.free()
    gpu.trim()
    t1 = time.time()
    tiles = assert_dispatch(prof, steps_at_least)
    sets = [expected_reads(workload, seeds[0], na, **args), expected_reads(workload, seeds[1], NB, **args)]
    t2 = time.time()
    reads, lengths = assert_certified(oracle, name, out, sets, [("A", a, sets[0]), ("B", b, sets[1])])
    report(name, bases=out["bases"], gpu_s=t1 - t0, reads_s=t2 - t1, certificate_s=time.time() - t2, tile_builds=tiles,
           frontier_steps=prof["frontier_step"][1], range_steps=prof["range_step"][1])
    return dict(a=a, b=b, out=out, reads=reads, lengths=lengths, prof=prof)


def same_output(got, out):
    return all(np.array_equal(np.asarray(got[k]), np.asarray(out[k])) for k in ("data", "block_end", "cum", "C")) and \
        (int(got["sequences"]), int(got["bases"])) == (int(out["sequences"]), int(out["bases"]))


def assert_same_as_certified(oracle, name, got, case):
    """`got` must be the stream, samples and C that the case's certificate accepted; certify_native is a function of exactly these, so equal
    arrays pass it too.  When they differ the certificate runs on `got` and its diagnosis is the message."""
    if not same_output(got, case["out"]):
        verdict = verdict_of(oracle, got, case["reads"], case["lengths"])
        pytest.fail("%s: differs from the certified merge of the same inputs; its own certificate: %s" % (name, verdict or "passes (two accepted streams differ: the certificate is broken)"))


@pytest.fixture(scope="module")
def iid_case(gpu, oracle):
    return merged_case(gpu, oracle, "iid", "iid", 1 << 19, (5101, 5102), 100)


def test_iid_merge_is_the_bwt_of_the_generated_reads(gpu, oracle, iid_case):
    """2^19 + (2^21 + 70 000) iid reads x 100 (272 Mbase merged, more than 2^28 rows).  Dispatch by size: frontier steps, no walk, node
    levels first.  Then the sensitivity of the whole check on this real output, on the host alone: two unequal neighbouring symbols beyond
    row 2^28 exchanged must be rejected with a sequence named -- what a subtly wrong kernel would look like, without making one."""
    out = iid_case["out"]
    assert out["bases"] > (1 << 28) + 4096
    sym = oracle.FMI.from_native(out["data"], out["sequences"], out["bases"]).symbols
    rng = np.random.default_rng(20)
    i = int(rng.integers(1 << 28, out["bases"] - 1))
    while sym[i] == sym[i + 1]:
        i += 1
    assert (1 << 28) < i < out["bases"] - 1
    sym[i], sym[i + 1] = sym[i + 1], sym[i]
    t0 = time.time()
    verdict = certify(sym, iid_case["reads"], iid_case["lengths"])
    report("iid_mutant", row=i, certificate_s=time.time() - t0)
    assert verdict is not None and "first: sequence" in verdict, verdict


def test_iid_merge_agrees_with_the_oracles_merge(gpu, oracle, iid_case):
    """A second, independent verdict on the same output: the oracle's merge (its restated search, no suffix sort) of the builder's two
    streams gives the same bytes and samples.  The certificate and the oracle must agree."""
    a, b, out = iid_case["a"], iid_case["b"], iid_case["out"]
    t0 = time.time()
    fa = oracle.FMI.from_native(a["data"], a["sequences"], a["bases"]); fb = oracle.FMI.from_native(b["data"], b["sequences"], b["bases"])
    m, _ = oracle.merge(fa, fb, threads=16)
    report("iid_oracle_merge", oracle_s=time.time() - t0)
    be, cum = m.samples
    assert same_output(dict(data=m.data, sequences=m.sequences, bases=m.bases, block_end=be, cum=cum, C=m.C), out)


def test_host_to_host_merge_of_the_iid_pair(gpu, oracle, iid_case):
    """bwtm_merge_host on the builder's two streams as (data, sequences, bases) tuples, default chunk sizes, with full samples and with the
    compact form expanded: both give the certified stream, samples and C; the two sample forms expand to the same arrays."""
    a, b = iid_case["a"], iid_case["b"]
    inputs = ((a["data"], a["sequences"], a["bases"]), (b["data"], b["sequences"], b["bases"]))
    forms = []
    for samples in (1, 2):
        r = gpu.merge_host(*inputs, samples=samples)
        be, cum = r.expanded_samples()
        got = dict(data=r.data.copy(), sequences=r.out.sequences, bases=r.out.bases, block_end=np.array(be), cum=np.array(cum), C=r.C)
        r.free()
        assert_same_as_certified(oracle, "merge_host(samples=%d)" % samples, got, iid_case)
        forms.append(got)
    assert np.array_equal(forms[0]["block_end"], forms[1]["block_end"]) and np.array_equal(forms[0]["cum"], forms[1]["cum"])
    gpu.trim()


def test_mixed_length_merge_is_the_bwt_of_the_generated_reads(gpu, oracle):
    """100 / 150 bp reads (BASELINE config 5's mix): the frontier shrinks after step 100 and the grid follows it; at least 150 steps."""
    merged_case(gpu, oracle, "mixed", "mixed", NA, (5201, 5202), 150)


@pytest.fixture(scope="module")
def genome_case(gpu, oracle):
    return merged_case(gpu, oracle, "genome300", "genome", NA, (5301, 5302), 100, coverage=300)


def test_genome_300x_merge_is_the_bwt_of_the_generated_reads(gpu, oracle, genome_case):
    """Reads of a genome at 300 x coverage with 1 % substitutions: long runs, many equal reads (ties go by sequence index, also between
    A and B), trie levels of few nodes."""
    assert genome_case["out"]["data"].size < genome_case["out"]["bases"] // 3            # a compressible stream: the long-run forms of the encoder


def test_partitioned_merge_of_the_genome_pair(gpu, oracle, genome_case):
    """The same pair as four parts (threads of this process over contexts of the GPU), each transcoding its windows from its byte share of
    the host-resident streams: the parts' bytes and samples laid end to end are the certified stream; every part searched."""
    from bwt_merge_amd import partitioned
    a, b, out = genome_case["a"], genome_case["b"], genome_case["out"]
    ha = gpu.host_index(a["data"], a["cum"], a["sequences"], a["bases"]); hb = gpu.host_index(b["data"], b["cum"], b["sequences"], b["bases"])
    res = partitioned.merge_parts(gpu, ha, hb, 4, kmer=4, collect=lambda g, s: partitioned.slice_arrays(s))
    try:
        got, stats = res["collected"], res["stats"]
    finally:
        res["release"]()
    assert all(s["steps"] > 0 for s in stats), stats
    cum = np.concatenate([g[2] for g in got], axis=1)
    totals = (out["C"][1:] - out["C"][:-1]).reshape(6, 1)                                 # the column behind the last block: the symbol counts
    laid = dict(data=np.concatenate([g[0] for g in got]), block_end=np.concatenate([g[1] for g in got]), cum=np.concatenate([cum, totals], axis=1),
                C=out["C"], sequences=out["sequences"], bases=out["bases"])
    assert_same_as_certified(oracle, "merge_parts(parts=4, kmer=4)", laid, genome_case)
    gpu.make_default_current(); gpu.trim()


def test_genome_30x_merge_is_the_bwt_of_the_generated_reads(gpu, oracle):
    """The bench's default coverage: shorter runs than at 300 x, few equal reads."""
    merged_case(gpu, oracle, "genome30", "genome", NA, (5311, 5312), 100, coverage=30)


def test_asymmetric_merge_is_the_bwt_of_the_generated_reads(gpu, oracle):
    """BASELINE config 4's shape, an increment inserted into a larger index: 2^22 + (2^21 + 70 000) iid reads (643 Mbase merged;
    half of the base the issue starts from, for the time budget and the certificate's host memory)."""
    merged_case(gpu, oracle, "asymmetric", "iid", 1 << 22, (5601, 5602), 100)


def test_chain_of_four_mixed_sets_is_the_bwt_of_all_reads(gpu, oracle):
    """BASELINE config 5's shape: four sets of 2^20 reads of 100 / 150 bp merged in command-line order (bwt_merge.cpp:167-173), the
    intermediates without their native form.  Each increment is below 2^21 sequences, so these searches take the walk; the certificate is
    on the final index only (the inputs are certified when it fails)."""
    n, seeds = 1 << 20, (5501, 5502, 5503, 5504)
    t0 = time.time()
    running, natives = None, []
    for k, seed in enumerate(seeds):
        X = build(gpu, "mixed", seed, n).encode()
        natives.append(native_of(X))
        if running is None:
            running = X
            continue
        nxt = gpu.merge(running, X)
        running.free(); X.free()
        if k < len(seeds) - 1:
            nxt.drop_native()
        running = nxt
    out = native_of(running)
    running.free(); gpu.trim()
    t1 = time.time()
    assert (out["sequences"], out["bases"]) == (4 * n, sum(x["bases"] for x in natives))
    sets = [expected_reads("mixed", seed, n) for seed in seeds]
    t2 = time.time()
    assert_certified(oracle, "chain", out, sets, [("set %d" % k, natives[k], sets[k]) for k in range(4)])
    report("chain", bases=out["bases"], gpu_s=t1 - t0, reads_s=t2 - t1, certificate_s=time.time() - t2)


@pytest.mark.parametrize("workload,args", [("genome", {"coverage": 300}), ("mixed", {})])
def test_builder_alone(gpu, oracle, workload, args):
    """Builder(2^19) over 2^21 reads: four leaves, two levels of the library's own merge tree.  The rank structure's symbols (extract) are the
    symbols of the encoded stream, and that stream, its samples and C are the BWT of the generated reads; equal reads that fall into
    different leaves must come out in read order, which the certificate checks like everything else.  (Counted on the host: of the 2^21
    genome reads at 300 x, 514 058 have an equal partner, and 315 478 pairs of equal reads -- 172 351 groups -- lie in different leaves;
    the mixed iid reads have none, they are there for the ragged leaves.)"""
    n = 1 << 21
    t0 = time.time()
    X = build(gpu, workload, 5401, n, **args)
    sym = X.extract(0, X.bases)
    X.encode()
    out = native_of(X)
    X.free(); gpu.trim()
    t1 = time.time()
    assert np.array_equal(sym, oracle.FMI.from_native(out["data"], out["sequences"], out["bases"]).symbols)
    del sym
    sets = [expected_reads(workload, 5401, n, **args)]
    t2 = time.time()
    assert_certified(oracle, "builder[%s]" % workload, out, sets, [])
    report("builder_" + workload, bases=out["bases"], gpu_s=t1 - t0, reads_s=t2 - t1, certificate_s=time.time() - t2)
