/*
  api/edit.hip.h -- patterns within edit distance e (bwtm_find_edit_batch): the backward search of a batch of patterns as one frontier of
  ranges whose nodes carry a band of the edit-distance matrix, level by level (kernels/edit.hip.h), its hits collected per pattern and
  length.  Part of bwtm_api.hip, behind api/approx.hip.h, whose hit stream it shares.  Batches: see api/batches.hip.h.

  Device memory of the call beyond the index, per batch of bwtm_tune("approx_batch") patterns, with P = the largest frontier of the batch
  (its first one has a root per pattern, so P >= patterns of the batch), H = the hits of the batch before max_hits, T = the bytes of its
  pattern text and e = max_edits (bwtm_find_edit_stats reports P and H):

      peak <= (308 + 34 e) P + 132 H + 2 T + 2^20 bytes                (every block below 512 MiB)

  256 P  two frontiers of 32 bytes per node (range, pattern and band), whose capacities at least double when they grow (api/frontier.hip.h:
         the blocks one frontier ever had hold fewer than 4 P nodes together, and a block taken back stays with the pool).
   96 H  the hit stream of the batch, 24 bytes per hit (range, and pattern / length / edits in one word).  It grows by a level's hits at a
         time and keeps what it holds: the same doubling, so its blocks, the one being copied from included, hold fewer than 4 H hits together.
   21 H  the kept hits in pattern order before they travel: sp, count, four bytes of length and one of edits.
   (33 + 32 e) P   per pattern: its offset, its kept count, and the first and the last position of its hits in each of the 2 e + 1 length
         slots (16 + 16 (2 e + 1) bytes); per 256 nodes: the two workgroup totals of a level, doubled as the frontiers are, and the
         partial sums of their scan.
      T  the pattern text.
   (19 + 2 e) P + 15 H + T + 2^20  what the pool rounds up: a block of 1 MiB or more to 64 KiB, of 64 MiB or more to 2 MiB, a smaller one to 256 bytes.
  A block of 512 MiB or more is made of whole chunks of 1 GiB (api/context.hip.h): at that size add one chunk per block.
*/
#pragma once

namespace
{
// What the last call of this thread did: nodes expanded (the frontiers' sizes summed over the levels and batches), the largest frontier
// of a batch, the most hits of a batch before max_hits, levels run.
thread_local CallStats t_edit_stats;

EditNodes edit_nodes(const Frontier<4>& f, u64 capacity) { return EditNodes{f.array(0), f.array(1), f.array(2), f.array(3), std::min(capacity, f.cap)}; }

// One batch of patterns: the search, which leaves the hit stream, every pattern's positions in it per length slot and the batch's hit
// offsets on the device, and the gather that brings the kept hits to the caller.
struct EditBatch : PatternBatch
{
  Frontier<4> cur, next;                               // sp, count, pattern, band

  u64 slots() const { return 2 * (u64)max_cost + 1; }
  u64* first() const { return d_slots.as<u64>(); }
  u64* end(u64 nb) const { return d_slots.as<u64>() + slots() * nb; }

  // The patterns first .. first + nb - 1 of the call; hit_offsets[0 .. nb] continue hit_offsets[0] by the kept counts.
  int search(const u8* patterns, const u64* offsets, u64 nb, u64* hit_offsets)
  {
    const char* const who = "bwtm_find_edit_batch";
    const u64 before = hit_offsets[0];
    const IndexView v = x->view();
    TRY(stage(patterns, offsets, nb, 2 * slots() * nb));
    TRY(cur.reserve(nb, who));
    LAUNCH("edit_roots", k_edit_roots, div_up(nb, BLOCK_THREADS), BLOCK_THREADS, d_off.as<const u64>(), nb, x->n, edit_nodes(cur, nb));
    u64 count = nb, peak = nb;
    const u64 levels = std::max<u64>(longest() + max_cost, 1);                                    // a root that is a hit becomes one in the first level
    for(u64 t = 0; t < levels && count > 0; t++)
    {
      const u64 nblocks = div_up(count, BLOCK_THREADS);
      TRY(totals.reserve(2, nblocks));
      LAUNCH("edit_count", (k_edit_level<false>), nblocks, BLOCK_THREADS, v, d_text.as<const u8>(), bytes, d_off.as<const u64>(), nb, max_cost, t,
        (const u64*)cur.array(0), (const u64*)cur.array(1), (const u64*)cur.array(2), (const u64*)cur.array(3), count, nblocks, totals.p(),
        EditNodes{nullptr, nullptr, nullptr, nullptr, 0}, ApproxNodes{nullptr, nullptr, nullptr, 0}, (u64)0);
      TRY(totals.scan_and_read(2, nblocks, 1));                                                 // the next frontier's size, and that plus the level's hits
      const u64 kept = CTX.host_scratch[0], both = CTX.host_scratch[1];
      if(kept > 5 * count || both < kept || both - kept > 6 * count)
      {
        return fail(BWTM_EINVAL, "bwtm_find_edit_batch: level %llu counted %llu children and %llu hits of %llu nodes", (unsigned long long)(t + 1), (unsigned long long)kept,
          (unsigned long long)(both - kept), (unsigned long long)count);
      }
      const u64 found = both - kept;
      t_edit_stats[0] += count; t_edit_stats[3] = std::max(t_edit_stats[3], t + 1);
      if(kept > 0) { TRY(next.reserve(kept, who)); }
      if(found > 0) { TRY(hits.grow_keeping(nhits, nhits + found, who)); }
      if(both > 0)
      {
        LAUNCH("edit_expand", (k_edit_level<true>), nblocks, BLOCK_THREADS, v, d_text.as<const u8>(), bytes, d_off.as<const u64>(), nb, max_cost, t,
          (const u64*)cur.array(0), (const u64*)cur.array(1), (const u64*)cur.array(2), (const u64*)cur.array(3), count, nblocks, totals.p(),
          (kept > 0 ? edit_nodes(next, kept) : EditNodes{nullptr, nullptr, nullptr, nullptr, 0}), hit_nodes(nhits + found), nhits);
      }
      if(found > 0)
      {
        LAUNCH("edit_mark", k_edit_mark, div_up(found, BLOCK_THREADS), BLOCK_THREADS, (const u64*)hits.array(2), nhits, found, d_off.as<const u64>(), nb, max_cost, first(), end(nb));
        nhits += found;
      }
      if(kept > 0) { cur.swap(next); }
      count = kept; peak = std::max(peak, kept);
    }
    t_edit_stats[1] = std::max(t_edit_stats[1], peak); t_edit_stats[2] = std::max(t_edit_stats[2], nhits);
    LAUNCH("edit_cap", k_edit_cap, div_up(nb + 1, BLOCK_THREADS), BLOCK_THREADS, (const u64*)first(), (const u64*)end(nb), nb, max_cost, max_hits, d_base.as<u64>());
    return finish_offsets(who, nb, before, hit_offsets);
  }

  // The kept hits of the batch search() has just seen, in pattern order, into the caller's arrays (any of them null).
  int fill(u64 nb, const PatternHits& out)
  {
    if(kept_total == 0) { return BWTM_OK; }
    if(kept_total > (~0ull) / 24) { return fail(BWTM_ENOMEM, "bwtm_find_edit_batch: %llu hits do not fit", (unsigned long long)kept_total); }
    TRY(d_out.alloc(21 * kept_total));
    u64* o_sp = d_out.as<u64>(); u64* o_cnt = o_sp + kept_total; u32* o_len = (u32*)(o_cnt + kept_total); u8* o_ed = (u8*)(o_len + kept_total);
    LAUNCH("edit_gather", k_edit_gather, div_up(nhits, BLOCK_THREADS), BLOCK_THREADS, (const u64*)hits.array(0), (const u64*)hits.array(1), (const u64*)hits.array(2), nhits,
      d_off.as<const u64>(), nb, max_cost, (const u64*)first(), (const u64*)end(nb), d_base.as<const u64>(), o_sp, o_cnt, o_len, o_ed, kept_total);
    TRY(to_host(out.sp, o_sp, kept_total)); TRY(to_host(out.count, o_cnt, kept_total));
    TRY(to_host(out.lengths, o_len, kept_total)); TRY(to_host(out.cost, o_ed, kept_total));
    HIP_TRY(hipStreamSynchronize(CTX.stream));                                                  // the batch's buffers are reused
    return BWTM_OK;
  }
};

} // namespace

extern "C" int bwtm_find_edit_batch(const bwtm_index* x, const uint8_t* patterns, const uint64_t* offsets, uint64_t count, uint32_t max_edits, uint64_t max_hits,
                                    uint64_t* hit_offsets, uint64_t* out_sp, uint64_t* out_count, uint8_t* out_edits, uint32_t* out_lengths, uint64_t capacity)
{
  if(!x || !hit_offsets || (count > 0 && !offsets)) { return fail(BWTM_EINVAL, "bwtm_find_edit_batch: null argument"); }
  WHOLE_INDEX(x, "bwtm_find_edit_batch");
  ENTER(x->ctx);
  if(max_edits > EDIT_MAX_EDITS)
  {
    return fail(BWTM_EINVAL, "bwtm_find_edit_batch: max_edits = %u is outside 0..%u", (unsigned)max_edits, (unsigned)EDIT_MAX_EDITS);
  }
  t_edit_stats.reset();
  hit_offsets[0] = 0;
  if(count == 0) { return BWTM_OK; }
  TRY(validate_texts("bwtm_find_edit_batch", "pattern", patterns, offsets, count, APPROX_MAX_LEN));
  const int rc = pattern_run<EditBatch>("bwtm_find_edit_batch", &t_edit_stats, x, patterns, offsets, count, max_edits, max_hits, hit_offsets,
    PatternHits{out_sp, out_count, out_edits, out_lengths}, capacity);
  if(rc != BWTM_OK) { (void)hipStreamSynchronize(CTX.stream); }                                 // the half-built state goes back to the pool behind this
  return rc;
}

extern "C" int bwtm_find_edit_stats(uint64_t stats[4]) { return t_edit_stats.get("bwtm_find_edit_stats", stats); }
