/*
  api/approx.hip.h -- patterns with up to d substitutions (bwtm_find_approx_batch): the backward search of a batch of patterns as one
  frontier of ranges, level by level (kernels/approx.hip.h), its hits collected per pattern.  Part of bwtm_api.hip.  Batches: see
  api/batches.hip.h.

  Device memory of the call beyond the index, per batch of bwtm_tune("approx_batch") patterns, with P = the largest frontier of the batch
  (its first one has a root per pattern, so P >= patterns of the batch), H = the hits of the batch before max_hits and T = the bytes of its
  pattern text (bwtm_find_approx_stats reports P and H):

      peak <= 240 P + 128 H + 2 T + 2^20 bytes                         (every block below 512 MiB)

  192 P  two frontiers of 24 bytes per node, whose capacities at least double when they grow (api/frontier.hip.h: the blocks one frontier
         ever had hold fewer than 4 P nodes together, and a block taken back stays with the pool).
   96 H  the hit stream of the batch, 24 bytes per hit.  It grows by a level's hits at a time and keeps what it holds: the same doubling,
         so its blocks, the one being copied from included, hold fewer than 4 H hits together.
   17 H  the kept hits in pattern order before they travel: sp, count and one byte of mismatches.
   33 P  per pattern: its offset, the first and the last slot of its hits, its kept count (32 bytes); per 256 nodes (per 64 with four lanes per node): the two workgroup totals
         of a level, doubled as the frontiers are, and the partial sums of their scan.
      T  the pattern text.
   15 P + 15 H + T + 2^20  what the pool rounds up: a block of 1 MiB or more to 64 KiB, of 64 MiB or more to 2 MiB, a smaller one to 256 bytes.
  A block of 512 MiB or more is made of whole chunks of 1 GiB (api/context.hip.h): at that size add one chunk per block.
*/
#pragma once

namespace
{
// What the last call of this thread did: nodes expanded (the frontiers' sizes summed over the levels and batches), the largest frontier
// of a batch, the most hits of a batch before max_hits, levels run.
thread_local CallStats t_approx_stats;

u64 pattern_batch_size() { return std::min<u64>((u64)g_tune.approx_batch, WALK_BATCH_LIMIT); }

// Where a pattern search's hits go: the caller's arrays, any of them null.  cost = mismatches or edits; lengths only for the edit search.
struct PatternHits
{
  u64* sp; u64* count; u8* cost; u32* lengths;
  bool any() const { return sp || count || cost || lengths; }
  PatternHits at(u64 i) const { return PatternHits{at_or_null(sp, i), at_or_null(count, i), at_or_null(cost, i), at_or_null(lengths, i)}; }
};

// What one batch of patterns is to this search and to that of api/edit.hip.h: its staged text and offsets, the hit stream (sp, count,
// meta) of its levels, every pattern's slots in it, and the batch's hit offsets.
struct PatternBatch : StagedTexts
{
  const bwtm_index* x = nullptr;
  u32 max_cost = 0; u64 max_hits = 0;                   // the search's budget of mismatches or edits; hits kept per pattern (0: all)
  DevBuf d_slots, d_base, d_out;
  LevelTotals totals;
  Frontier<3> hits;
  u64 nhits = 0, kept_total = 0;

  ApproxNodes hit_nodes(u64 capacity) const { return ApproxNodes{hits.array(0), hits.array(1), hits.array(2), std::min(capacity, hits.cap)}; }

  // The patterns of offsets[0 .. nb] to the device, `slot_words` zeroed u64 for the marks, and an empty hit stream.
  int stage(const u8* patterns, const u64* offsets, u64 nb, u64 slot_words)
  {
    nhits = 0;
    TRY(StagedTexts::stage(patterns, offsets, nb));
    TRY(d_slots.alloc(slot_words * sizeof(u64), true)); TRY(d_base.alloc((nb + 1) * sizeof(u64)));
    return BWTM_OK;
  }

  // d_base[0 .. nb] holds the capped counts: hit_offsets[0 .. nb] = their scan, continuing `before`, the hits of the call's earlier batches.
  int finish_offsets(const char* who, u64 nb, u64 before, u64* hit_offsets)
  {
    TRY(device_scan<0>(d_base.as<const u64>(), d_base.as<u64>(), nb + 1));
    TRY(to_host(hit_offsets, d_base.as<const u64>(), nb + 1));
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    kept_total = hit_offsets[nb];
    if(kept_total > nhits) { return fail(BWTM_EINVAL, "%s: %llu hits kept of %llu found", who, (unsigned long long)kept_total, (unsigned long long)nhits); }
    if(before != 0) { for(u64 k = 0; k <= nb; k++) { hit_offsets[k] += before; } }
    return BWTM_OK;
  }
};

// A call of a pattern search, over a Batch with search() and fill(): batches of pattern_batch_size() in the two rounds of api/batches.hip.h.
// stats[0] counts the nodes expanded, once.
template<class Batch>
int pattern_run(const char* who, CallStats* stats, const bwtm_index* x, const u8* patterns, const u64* offsets, u64 count, u32 max_cost, u64 max_hits, u64* hit_offsets,
                const PatternHits& out, u64 capacity)
{
  const u64 batch = std::min(pattern_batch_size(), count);
  Batch b;
  b.x = x; b.max_cost = max_cost; b.max_hits = max_hits;
  return two_round_call(who, "hits", count, hit_offsets, out.any(), capacity, stats,
    [&](u64 done) { return std::min(batch, count - done); },
    [&](u64 done, u64 nb, u64* batch_offsets) { return b.search(patterns, offsets + done, nb, batch_offsets); },
    [&](u64, u64 nb, u64 at) { return b.fill(nb, out.at(at)); });
}

ApproxNodes approx_nodes(const Frontier<3>& f, u64 capacity) { return ApproxNodes{f.array(0), f.array(1), f.array(2), std::min(capacity, f.cap)}; }

// One batch of patterns: the search, which leaves the hit stream, every pattern's slots in it and the batch's hit offsets on the device,
// and the gather that brings the kept hits to the caller.
struct ApproxBatch : PatternBatch
{
  Frontier<3> cur, next;                               // sp, count, meta

  // One pass of a level over the frontier `cur`: the count pass, or the expand pass into `next` and the hit stream.
  template<bool QUAD>
  int level(bool emit, const IndexView& v, u64 nb, u64 count, u64 nblocks, u64 kept, u64 found)
  {
    if(emit)
    {
      LAUNCH("approx_expand", (k_approx_level<QUAD, true>), nblocks, BLOCK_THREADS, v, d_text.as<const u8>(), bytes, d_off.as<const u64>(), nb, max_cost,
        (const u64*)cur.array(0), (const u64*)cur.array(1), (const u64*)cur.array(2), count, nblocks, totals.p(), approx_nodes(next, kept), hit_nodes(nhits + found), nhits);
    }
    else
    {
      LAUNCH("approx_count", (k_approx_level<QUAD, false>), nblocks, BLOCK_THREADS, v, d_text.as<const u8>(), bytes, d_off.as<const u64>(), nb, max_cost,
        (const u64*)cur.array(0), (const u64*)cur.array(1), (const u64*)cur.array(2), count, nblocks, totals.p(), ApproxNodes{nullptr, nullptr, nullptr, 0}, ApproxNodes{nullptr, nullptr, nullptr, 0}, (u64)0);
    }
    return BWTM_OK;
  }
  int level(bool emit, const IndexView& v, u64 nb, u64 count, u64 nblocks, u64 kept, u64 found)
  {
#ifdef BWTM_DIAGNOSTICS
    if(g_tune.approx_kernel == 1) { return level<true>(emit, v, nb, count, nblocks, kept, found); }      // the A/B partner: four lanes per node
#endif
    return level<false>(emit, v, nb, count, nblocks, kept, found);
  }

  u64* first() const { return d_slots.as<u64>(); }
  u64* end(u64 nb) const { return d_slots.as<u64>() + nb; }

  // The patterns first .. first + nb - 1 of the call; hit_offsets[0 .. nb] continue hit_offsets[0] by the kept counts.
  int search(const u8* patterns, const u64* offsets, u64 nb, u64* hit_offsets)
  {
    const char* const who = "bwtm_find_approx_batch";
    const u64 before = hit_offsets[0];
    const IndexView v = x->view();
#ifdef BWTM_DIAGNOSTICS
    const u64 block_nodes = (g_tune.approx_kernel == 1 ? approx_block_nodes<true>() : approx_block_nodes<false>());
#else
    const u64 block_nodes = approx_block_nodes<false>();
#endif
    TRY(stage(patterns, offsets, nb, 2 * nb));
    TRY(cur.reserve(nb, who));
    LAUNCH("approx_roots", k_approx_roots, div_up(nb, BLOCK_THREADS), BLOCK_THREADS, d_off.as<const u64>(), nb, x->n, approx_nodes(cur, nb));
    u64 count = nb, peak = nb;
    const u64 levels = std::max<u64>(longest(), 1);                                               // an empty pattern's root becomes its hit in the first one
    for(u64 t = 0; t < levels && count > 0; t++)
    {
      const u64 nblocks = div_up(count, block_nodes);
      TRY(totals.reserve(2, nblocks));
      TRY(level(false, v, nb, count, nblocks, 0, 0));
      TRY(totals.scan_and_read(2, nblocks, 1));                                                 // the next frontier's size, and that plus the level's hits
      const u64 kept = CTX.host_scratch[0], both = CTX.host_scratch[1];
      if(kept > 5 * count || both < kept || both - kept > 5 * count)
      {
        return fail(BWTM_EINVAL, "bwtm_find_approx_batch: level %llu counted %llu children and %llu hits of %llu nodes", (unsigned long long)(t + 1), (unsigned long long)kept,
          (unsigned long long)(both - kept), (unsigned long long)count);
      }
      const u64 found = both - kept;
      t_approx_stats[0] += count; t_approx_stats[3] = std::max(t_approx_stats[3], t + 1);
      if(kept > 0) { TRY(next.reserve(kept, who)); }
      if(found > 0) { TRY(hits.grow_keeping(nhits, nhits + found, who)); }
      if(both > 0) { TRY(level(true, v, nb, count, nblocks, kept, found)); }
      if(found > 0)
      {
        LAUNCH("approx_mark", k_approx_mark, div_up(found, BLOCK_THREADS), BLOCK_THREADS, (const u64*)hits.array(2), nhits, found, nb, first(), end(nb));
        nhits += found;
      }
      if(kept > 0) { cur.swap(next); }
      count = kept; peak = std::max(peak, kept);
    }
    t_approx_stats[1] = std::max(t_approx_stats[1], peak); t_approx_stats[2] = std::max(t_approx_stats[2], nhits);
    LAUNCH("approx_cap", k_approx_cap, div_up(nb + 1, BLOCK_THREADS), BLOCK_THREADS, (const u64*)first(), (const u64*)end(nb), nb, max_hits, d_base.as<u64>());
    return finish_offsets(who, nb, before, hit_offsets);
  }

  // The kept hits of the batch search() has just seen, in pattern order, into the caller's arrays (any of them null).
  int fill(u64 nb, const PatternHits& out)
  {
    if(kept_total == 0) { return BWTM_OK; }
    if(kept_total > (~0ull) / 24) { return fail(BWTM_ENOMEM, "bwtm_find_approx_batch: %llu hits do not fit", (unsigned long long)kept_total); }
    TRY(d_out.alloc(17 * kept_total));
    u64* o_sp = d_out.as<u64>(); u64* o_cnt = o_sp + kept_total; u8* o_mm = (u8*)(o_cnt + kept_total);
    LAUNCH("approx_gather", k_approx_gather, div_up(nhits, BLOCK_THREADS), BLOCK_THREADS, (const u64*)hits.array(0), (const u64*)hits.array(1), (const u64*)hits.array(2), nhits, nb,
      (const u64*)first(), d_base.as<const u64>(), o_sp, o_cnt, o_mm, kept_total);
    TRY(to_host(out.sp, o_sp, kept_total)); TRY(to_host(out.count, o_cnt, kept_total)); TRY(to_host(out.cost, o_mm, kept_total));
    HIP_TRY(hipStreamSynchronize(CTX.stream));                                                  // the batch's buffers are reused
    return BWTM_OK;
  }
};

} // namespace

extern "C" int bwtm_find_approx_batch(const bwtm_index* x, const uint8_t* patterns, const uint64_t* offsets, uint64_t count, uint32_t max_mismatches, uint64_t max_hits,
                                      uint64_t* hit_offsets, uint64_t* out_sp, uint64_t* out_count, uint8_t* out_mismatches, uint64_t capacity)
{
  if(!x || !hit_offsets || (count > 0 && !offsets)) { return fail(BWTM_EINVAL, "bwtm_find_approx_batch: null argument"); }
  WHOLE_INDEX(x, "bwtm_find_approx_batch");
  ENTER(x->ctx);
  if(max_mismatches > APPROX_MAX_MISMATCHES)
  {
    return fail(BWTM_EINVAL, "bwtm_find_approx_batch: max_mismatches = %u is outside 0..%u", (unsigned)max_mismatches, (unsigned)APPROX_MAX_MISMATCHES);
  }
  t_approx_stats.reset();
  hit_offsets[0] = 0;
  if(count == 0) { return BWTM_OK; }
  TRY(validate_texts("bwtm_find_approx_batch", "pattern", patterns, offsets, count, APPROX_MAX_LEN));
  const int rc = pattern_run<ApproxBatch>("bwtm_find_approx_batch", &t_approx_stats, x, patterns, offsets, count, max_mismatches, max_hits, hit_offsets,
    PatternHits{out_sp, out_count, out_mismatches, nullptr}, capacity);
  if(rc != BWTM_OK) { (void)hipStreamSynchronize(CTX.stream); }                                 // the half-built state goes back to the pool behind this
  return rc;
}

extern "C" int bwtm_find_approx_stats(uint64_t stats[4]) { return t_approx_stats.get("bwtm_find_approx_stats", stats); }
