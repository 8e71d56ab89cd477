/*
  api/kmer_join.hip.h -- the k-mers of two indexes with their counts and insertion points in each (bwtm_kmer_join_*): one joint walk down
  both suffix tries, one level per step (kernels/kmer_join.hip.h), and the summary of the result.  Part of bwtm_api.hip.

  Device memory of bwtm_kmer_join_create beyond the two indexes, with P = max_t nodes[t] (bwtm_kmer_join_levels):

      peak <= 392 P + 2^20 bytes                                       (every block below 512 MiB)

  320 P  two frontiers of 40 bytes per node, whose capacities at least double when they grow (api/frontier.hip.h: the blocks one frontier
         ever had hold fewer than 4 P nodes together).
   40 P  the result at its exact size, when the last frontier's block is larger: the handle keeps 40 bytes per k-mer and nothing else.
    8 P  the per-workgroup totals of the split (32 bytes per 256 nodes, the same doubling) and the partial sums of their scan.
   24 P + 2^20  what the pool rounds up: a block of 1 MiB or more to 64 KiB, of 64 MiB or more to 2 MiB, a smaller one to 256 bytes
         (the seven sums of the summary are one such block).
  A block of 512 MiB or more is made of whole chunks of 1 GiB (api/context.hip.h): at that size add one chunk per block, six at most.
*/
#pragma once

struct bwtm_kmer_join
{
  bwtm_context* ctx = nullptr;
  bwtm_kmer_join() : ctx(t_ctx) { if(ctx) { ctx->live_handles++; } }
  ~bwtm_kmer_join() { if(ctx) { ctx->live_handles--; } }
  bwtm_kmer_join(const bwtm_kmer_join&) = delete; bwtm_kmer_join& operator=(const bwtm_kmer_join&) = delete;
  DevBuf nodes;                       // 5 x capacity u64: sp_a, cnt_a, sp_b, cnt_b, code of the kept k-mers, ascending
  u64 capacity = 0;
  u64 distinct = 0;
  u64 stats[KMER_JOIN_STATS] = {};
  u64 levels[KMER_MAX_K] = {};        // kept (t + 1)-mers, t < k
  u32 k = 0;
  const u64* array(u32 which) const { return nodes.as<const u64>() + which * capacity; }
};

namespace
{

KmerJoinNodes kmer_join_nodes(const Frontier<5>& f) { return KmerJoinNodes{f.array(0), f.array(1), f.array(2), f.array(3), f.array(4)}; }

bool kmer_join_keeps(u64 ca, u64 cb, const KmerJoinBounds& bd)
{
  return ca >= bd.min_a && ca <= bd.max_a && cb >= bd.min_b && cb <= bd.max_b && ca + cb >= bd.min_sum;
}

int kmer_join_build(bwtm_kmer_join* kj, const bwtm_index* a, const bwtm_index* b, u32 k, u32 skip, const KmerJoinBounds& last)
{
  const IndexView va = a->view(), vb = b->view();
  KmerJoinBounds inner = last;                                                                  // upper bounds cannot prune above level k
  inner.max_a = ~0ull; inner.max_b = ~0ull;
  const char* const who = "bwtm_kmer_join_create";
  Frontier<5> cur, next;
  LevelTotals totals;
  // level 1, from both C arrays
  u64 h_nodes[20]; u64 count = 0;
  for(u32 j = 0; j < 4; j++)
  {
    const u32 c = kmer_comp(j, skip);
    const u64 ca = a->C[c + 1] - a->C[c], cb = b->C[c + 1] - b->C[c];
    if(kmer_join_keeps(ca, cb, k == 1 ? last : inner))
    {
      h_nodes[count] = a->C[c]; h_nodes[4 + count] = ca; h_nodes[8 + count] = b->C[c]; h_nodes[12 + count] = cb; h_nodes[16 + count] = j; count++;
    }
  }
  kj->levels[0] = count;
  if(count > 0)
  {
    TRY(cur.reserve(count, who));
    for(u32 w = 0; w < 5; w++) { HIP_TRY(hipMemcpyAsync(cur.array(w), h_nodes + 4 * w, count * sizeof(u64), hipMemcpyHostToDevice, CTX.stream)); }
    HIP_TRY(hipStreamSynchronize(CTX.stream));                                                  // h_nodes is on the stack
  }
  for(u32 t = 1; t < k && count > 0; t++)
  {
    const KmerJoinBounds& bd = (t + 1 < k ? inner : last);
    const u64 nblocks = div_up(count, (u64)BLOCK_THREADS);
    TRY(totals.reserve(4, nblocks));
    LAUNCH("kmer_join_count", (k_kmer_join_level<false>), nblocks, BLOCK_THREADS, va, vb, skip, bd, t, kmer_join_nodes(cur), count, nblocks, totals.p(), KmerJoinNodes{}, (u64)0);
    TRY(totals.scan_and_read(4, nblocks, 4));                                                   // the size of the next frontier
    const u64 kept = CTX.host_scratch[0];
    if(kept > 4 * count) { return fail(BWTM_EINVAL, "bwtm_kmer_join_create: level %u counted %llu children of %llu nodes", t + 1, (unsigned long long)kept, (unsigned long long)count); }
    kj->levels[t] = kept;
    if(kept > 0)
    {
      TRY(next.reserve(kept, who));
      LAUNCH("kmer_join_expand", (k_kmer_join_level<true>), nblocks, BLOCK_THREADS, va, vb, skip, bd, t, kmer_join_nodes(cur), count, nblocks, totals.p(), kmer_join_nodes(next), kept);
      cur.swap(next);
    }
    count = kept;
  }
  next.buf.release(); totals.buf.release();
  kj->distinct = count; kj->k = k;
  if(count == 0) { return BWTM_OK; }                                                            // the handle holds no block
  TRY(cur.shrink_to(count, who));                                                               // the result at its exact size
  kj->nodes.swap(cur.buf); kj->capacity = cur.cap;
  DevBuf d_stats;
  TRY(d_stats.alloc(KMER_JOIN_STATS * sizeof(u64), true));
  LAUNCH("kmer_join_summary", k_kmer_join_summary, std::min<u64>(div_up(count, (u64)BLOCK_THREADS), 1024), BLOCK_THREADS, kj->array(1), kj->array(3), count,
    d_stats.as<unsigned long long>());
  TRY(fetch_u64(d_stats.as<u64>(), 0, KMER_JOIN_STATS));
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  for(u32 s = 0; s < KMER_JOIN_STATS; s++) { kj->stats[s] = CTX.host_scratch[s]; }
  return BWTM_OK;
}

} // namespace

extern "C" int bwtm_kmer_join_create(const bwtm_index* a, const bwtm_index* b, uint32_t k, uint32_t skip,
  uint64_t min_a, uint64_t max_a, uint64_t min_b, uint64_t max_b, uint64_t min_sum, bwtm_kmer_join** out)
{
  if(!a || !b || !out) { return fail(BWTM_EINVAL, "bwtm_kmer_join_create: null argument"); }
  if(a->windowed) { return fail(BWTM_EINVAL, "bwtm_kmer_join_create: a is a window of an index (bwtm_index_upload_window), which only serves the merge over partitioned records"); }
  if(b->windowed) { return fail(BWTM_EINVAL, "bwtm_kmer_join_create: b is a window of an index (bwtm_index_upload_window), which only serves the merge over partitioned records"); }
  if(a->ctx != b->ctx) { return fail(BWTM_EINVAL, "bwtm_kmer_join_create: the two indexes live in different contexts"); }
  ENTER(a->ctx);
  if(k == 0 || k > KMER_MAX_K) { return fail(BWTM_EINVAL, "bwtm_kmer_join_create: k = %u is outside 1..%u", (unsigned)k, (unsigned)KMER_MAX_K); }
  if(skip < 1 || skip > 5) { return fail(BWTM_EINVAL, "bwtm_kmer_join_create: skip = %u is no comp value 1..5", (unsigned)skip); }
  if(min_a > max_a) { return fail(BWTM_EINVAL, "bwtm_kmer_join_create: min_a = %llu exceeds max_a = %llu", (unsigned long long)min_a, (unsigned long long)max_a); }
  if(min_b > max_b) { return fail(BWTM_EINVAL, "bwtm_kmer_join_create: min_b = %llu exceeds max_b = %llu", (unsigned long long)min_b, (unsigned long long)max_b); }
  if(min_sum == 0) { min_sum = 1; }
  const KmerJoinBounds bounds{min_a, max_a, min_b, max_b, min_sum};
  bwtm_kmer_join* kj = new bwtm_kmer_join();
  const int rc = kmer_join_build(kj, a, b, k, skip, bounds);
  if(rc != BWTM_OK) { (void)hipStreamSynchronize(CTX.stream); delete kj; return rc; }
  *out = kj;
  return BWTM_OK;
}

extern "C" void bwtm_kmer_join_free(bwtm_kmer_join* join)
{
  if(!join) { return; }
  Scope scope(join->ctx);
  delete join;                                        // the result returns to the pool (stream ordered)
}

extern "C" uint64_t bwtm_kmer_join_distinct(const bwtm_kmer_join* join) { return join ? join->distinct : 0; }
extern "C" uint64_t bwtm_kmer_join_bytes(const bwtm_kmer_join* join) { return join ? join->nodes.bytes : 0; }

extern "C" int bwtm_kmer_join_levels(const bwtm_kmer_join* join, uint64_t nodes[32])
{
  if(!join || !nodes) { return fail(BWTM_EINVAL, "bwtm_kmer_join_levels: null argument"); }
  for(u32 t = 0; t < KMER_MAX_K; t++) { nodes[t] = (t < join->k ? join->levels[t] : 0); }
  return BWTM_OK;
}

extern "C" int bwtm_kmer_join_download(const bwtm_kmer_join* join, uint64_t first, uint64_t count,
  uint64_t* codes, uint64_t* count_a, uint64_t* count_b, uint64_t* sp_a, uint64_t* sp_b)
{
  if(!join) { return fail(BWTM_EINVAL, "bwtm_kmer_join_download: null argument"); }
  ENTER(join->ctx);
  if(first > join->distinct || count > join->distinct - first)
  {
    return fail(BWTM_EINVAL, "bwtm_kmer_join_download: entries %llu + %llu lie beyond the %llu k-mers", (unsigned long long)first, (unsigned long long)count,
      (unsigned long long)join->distinct);
  }
  if(count == 0) { return BWTM_OK; }
  uint64_t* const dst[5] = {sp_a, count_a, sp_b, count_b, codes};
  for(u32 w = 0; w < 5; w++)
  {
    if(dst[w]) { HIP_TRY(hipMemcpyAsync(dst[w], join->array(w) + first, count * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream)); }
  }
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  return BWTM_OK;
}

extern "C" int bwtm_kmer_join_summary(const bwtm_kmer_join* join, uint64_t stats[7])
{
  if(!join || !stats) { return fail(BWTM_EINVAL, "bwtm_kmer_join_summary: null argument"); }
  for(u32 s = 0; s < KMER_JOIN_STATS; s++) { stats[s] = join->stats[s]; }
  return BWTM_OK;
}
