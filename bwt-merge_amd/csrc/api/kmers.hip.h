/*
  api/kmers.hip.h -- the distinct k-mers of an index with their counts and ranges (bwtm_kmers_*): the suffix trie down to depth k, one level
  per step (kernels/kmers.hip.h), and the spectrum of the result.  Part of bwtm_api.hip.

  Device memory of bwtm_kmers_create beyond the index, with P = max_t nodes[t] (bwtm_kmers_levels):

      peak <= 240 P + 2^20 bytes                                       (every block below 512 MiB)

  192 P  two frontiers of 24 bytes per node, whose capacities at least double when they grow (api/frontier.hip.h: the blocks one frontier
         ever had hold fewer than 4 P nodes together).  The early levels grow fourfold and are allocated exactly; a deep level of a read
         collection hardly grows at all.
   24 P  the result at its exact size, when the last frontier's block is larger: the handle keeps 24 bytes per k-mer and nothing else.
    8 P  the per-workgroup totals of the split (32 bytes per 256 nodes, the same doubling) and the partial sums of their scan.
   16 P + 2^20  what the pool rounds up: a block of 1 MiB or more to 64 KiB, of 64 MiB or more to 2 MiB, a smaller one to 256 bytes.
  A block of 512 MiB or more is made of whole chunks of 1 GiB (api/context.hip.h): at that size add one chunk per block, six at most.
*/
#pragma once

struct bwtm_kmers
{
  bwtm_context* ctx = nullptr;
  bwtm_kmers() : ctx(t_ctx) { if(ctx) { ctx->live_handles++; } }
  ~bwtm_kmers() { if(ctx) { ctx->live_handles--; } }
  bwtm_kmers(const bwtm_kmers&) = delete; bwtm_kmers& operator=(const bwtm_kmers&) = delete;
  DevBuf nodes;                       // 3 x capacity u64: sp, count, code of the kept k-mers, ascending
  u64 capacity = 0;
  u64 distinct = 0, total = 0;
  u64 levels[KMER_MAX_K] = {};        // kept (t + 1)-mers, t < k
  u32 k = 0;
  const u64* sp() const { return nodes.as<const u64>(); }
  const u64* cnt() const { return nodes.as<const u64>() + capacity; }
  const u64* code() const { return nodes.as<const u64>() + 2 * capacity; }
};

namespace
{

// The two launches of a level over the frontier `in` (sp, count, code).
template<bool QUAD>
int kmers_level_count(const IndexView& v, u32 skip, u64 min_count, u32 t, const Frontier<3>& in, u64 count, u64 nblocks, u64* totals)
{
  LAUNCH("kmer_count", (k_kmer_level<QUAD, false>), nblocks, BLOCK_THREADS, v, skip, min_count, t, (const u64*)in.array(0), (const u64*)in.array(1), (const u64*)in.array(2), count, nblocks,
    totals, (u64*)nullptr, (u64*)nullptr, (u64*)nullptr, (u64)0);
  return BWTM_OK;
}

template<bool QUAD>
int kmers_level_emit(const IndexView& v, u32 skip, u64 min_count, u32 t, const Frontier<3>& in, u64 count, u64 nblocks, u64* totals, const Frontier<3>& out, u64 kept)
{
  LAUNCH("kmer_expand", (k_kmer_level<QUAD, true>), nblocks, BLOCK_THREADS, v, skip, min_count, t, (const u64*)in.array(0), (const u64*)in.array(1), (const u64*)in.array(2), count, nblocks,
    totals, out.array(0), out.array(1), out.array(2), kept);
  return BWTM_OK;
}

int kmers_build(bwtm_kmers* km, const bwtm_index* x, u32 k, u32 skip, u64 min_count)
{
#ifdef BWTM_DIAGNOSTICS
  const bool quad = (g_tune.kmers_kernel == 1);                                                 // the A/B partner: four lanes per node
#else
  const bool quad = false;
#endif
  const u64 block_nodes = (quad ? kmer_block_nodes<true>() : kmer_block_nodes<false>());
  const IndexView v = x->view();
  const char* const who = "bwtm_kmers_create";
  Frontier<3> cur, next;
  LevelTotals totals;
  // level 1: the kept symbols that occur often enough
  u64 h_nodes[12]; u64 count = 0;
  for(u32 j = 0; j < 4; j++)
  {
    const u32 c = kmer_comp(j, skip);
    const u64 occ = x->C[c + 1] - x->C[c];
    if(occ >= min_count) { h_nodes[count] = x->C[c]; h_nodes[4 + count] = occ; h_nodes[8 + count] = j; count++; }
  }
  km->levels[0] = count;
  if(count > 0)
  {
    TRY(cur.reserve(count, who));
    for(u32 w = 0; w < 3; w++) { HIP_TRY(hipMemcpyAsync(cur.array(w), h_nodes + 4 * w, count * sizeof(u64), hipMemcpyHostToDevice, CTX.stream)); }
    HIP_TRY(hipStreamSynchronize(CTX.stream));                                                  // h_nodes is on the stack
  }
  for(u32 t = 1; t < k && count > 0; t++)
  {
    const u64 nblocks = div_up(count, block_nodes);
    TRY(totals.reserve(4, nblocks));
#ifdef BWTM_DIAGNOSTICS
    if(quad) { TRY(kmers_level_count<true>(v, skip, min_count, t, cur, count, nblocks, totals.p())); } else
#endif
    { TRY(kmers_level_count<false>(v, skip, min_count, t, cur, count, nblocks, totals.p())); }
    TRY(totals.scan_and_read(4, nblocks, 4));                                                   // the size of the next frontier
    const u64 kept = CTX.host_scratch[0];
    if(kept > 4 * count) { return fail(BWTM_EINVAL, "bwtm_kmers_create: level %u counted %llu children of %llu nodes", t + 1, (unsigned long long)kept, (unsigned long long)count); }
    km->levels[t] = kept;
    if(kept > 0)
    {
      TRY(next.reserve(kept, who));
#ifdef BWTM_DIAGNOSTICS
      if(quad) { TRY(kmers_level_emit<true>(v, skip, min_count, t, cur, count, nblocks, totals.p(), next, kept)); } else
#endif
      { TRY(kmers_level_emit<false>(v, skip, min_count, t, cur, count, nblocks, totals.p(), next, kept)); }
      cur.swap(next);
    }
    count = kept;
  }
  next.buf.release(); totals.buf.release();
  km->distinct = count; km->k = k;
  if(count == 0) { return BWTM_OK; }                                                            // the handle holds no block
  TRY(cur.shrink_to(count, who));                                                               // the result at its exact size
  km->nodes.swap(cur.buf); km->capacity = cur.cap;
  DevBuf d_total;
  TRY(d_total.alloc(sizeof(u64), true));
  LAUNCH("kmer_sum", k_kmer_sum, std::min<u64>(div_up(count, BLOCK_THREADS), 1024), BLOCK_THREADS, km->cnt(), count, d_total.as<unsigned long long>());
  TRY(fetch_u64(d_total.as<u64>(), 0));
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  km->total = CTX.host_scratch[0];
  return BWTM_OK;
}

} // namespace

extern "C" int bwtm_kmers_create(const bwtm_index* x, uint32_t k, uint32_t skip, uint64_t min_count, bwtm_kmers** out)
{
  if(!x || !out) { return fail(BWTM_EINVAL, "bwtm_kmers_create: null argument"); }
  WHOLE_INDEX(x, "bwtm_kmers_create");
  ENTER(x->ctx);
  if(k == 0 || k > KMER_MAX_K) { return fail(BWTM_EINVAL, "bwtm_kmers_create: k = %u is outside 1..%u", (unsigned)k, (unsigned)KMER_MAX_K); }
  if(skip < 1 || skip > 5) { return fail(BWTM_EINVAL, "bwtm_kmers_create: skip = %u is no comp value 1..5", (unsigned)skip); }
  if(min_count == 0) { min_count = 1; }
  bwtm_kmers* km = new bwtm_kmers();
  const int rc = kmers_build(km, x, k, skip, min_count);
  if(rc != BWTM_OK) { (void)hipStreamSynchronize(CTX.stream); delete km; return rc; }
  *out = km;
  return BWTM_OK;
}

extern "C" void bwtm_kmers_free(bwtm_kmers* kmers)
{
  if(!kmers) { return; }
  Scope scope(kmers->ctx);
  delete kmers;                                       // the result returns to the pool (stream ordered)
}

extern "C" uint64_t bwtm_kmers_distinct(const bwtm_kmers* kmers) { return kmers ? kmers->distinct : 0; }
extern "C" uint64_t bwtm_kmers_total(const bwtm_kmers* kmers) { return kmers ? kmers->total : 0; }
extern "C" uint64_t bwtm_kmers_bytes(const bwtm_kmers* kmers) { return kmers ? kmers->nodes.bytes : 0; }

extern "C" int bwtm_kmers_levels(const bwtm_kmers* kmers, uint64_t nodes[32])
{
  if(!kmers || !nodes) { return fail(BWTM_EINVAL, "bwtm_kmers_levels: null argument"); }
  for(u32 t = 0; t < KMER_MAX_K; t++) { nodes[t] = (t < kmers->k ? kmers->levels[t] : 0); }
  return BWTM_OK;
}

extern "C" int bwtm_kmers_download(const bwtm_kmers* kmers, uint64_t first, uint64_t count, uint64_t* codes, uint64_t* counts, uint64_t* sp)
{
  if(!kmers) { return fail(BWTM_EINVAL, "bwtm_kmers_download: null argument"); }
  ENTER(kmers->ctx);
  if(first > kmers->distinct || count > kmers->distinct - first)
  {
    return fail(BWTM_EINVAL, "bwtm_kmers_download: entries %llu + %llu lie beyond the %llu k-mers", (unsigned long long)first, (unsigned long long)count,
      (unsigned long long)kmers->distinct);
  }
  if(count == 0) { return BWTM_OK; }
  if(codes) { HIP_TRY(hipMemcpyAsync(codes, kmers->code() + first, count * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream)); }
  if(counts) { HIP_TRY(hipMemcpyAsync(counts, kmers->cnt() + first, count * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream)); }
  if(sp) { HIP_TRY(hipMemcpyAsync(sp, kmers->sp() + first, count * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream)); }
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  return BWTM_OK;
}

extern "C" int bwtm_kmers_histogram(const bwtm_kmers* kmers, uint64_t bins, uint64_t* hist)
{
  if(!kmers || !hist) { return fail(BWTM_EINVAL, "bwtm_kmers_histogram: null argument"); }
  ENTER(kmers->ctx);
  if(bins < 2) { return fail(BWTM_EINVAL, "bwtm_kmers_histogram: bins = %llu, at least 2 are needed (the last one collects the larger counts)", (unsigned long long)bins); }
  if(bins > (~0ull) / sizeof(u64)) { return fail(BWTM_ENOMEM, "bwtm_kmers_histogram: %llu bins do not fit", (unsigned long long)bins); }
  if(kmers->distinct == 0) { std::memset(hist, 0, bins * sizeof(u64)); return BWTM_OK; }
  DevBuf d_hist;
  TRY(d_hist.alloc(bins * sizeof(u64), true));
  LAUNCH("kmer_hist", k_kmer_hist, std::min<u64>(div_up(kmers->distinct, BLOCK_THREADS), 1024), BLOCK_THREADS, kmers->cnt(), kmers->distinct, (u64)bins,
    d_hist.as<unsigned long long>());
  HIP_TRY(hipMemcpyAsync(hist, d_hist.p, bins * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream));
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  return BWTM_OK;
}
