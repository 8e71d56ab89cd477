/*
  api/edit.hip.h -- patterns within edit distance e (bwtm_find_edit_batch): the backward search of a batch of patterns as one frontier of
  ranges whose nodes carry a band of the edit-distance matrix, level by level (kernels/edit.hip.h), its hits collected per pattern and
  length.  Part of bwtm_api.hip, behind api/approx.hip.h, whose batch size, hit stream and node views it uses.

  Device memory of the call beyond the index, per batch of bwtm_tune("approx_batch") patterns, with P = the largest frontier of the batch
  (its first one has a root per pattern, so P >= patterns of the batch), H = the hits of the batch before max_hits, T = the bytes of its
  pattern text and e = max_edits (bwtm_find_edit_stats reports P and H):

      peak <= (308 + 34 e) P + 132 H + 2 T + 2^20 bytes                (every block below 512 MiB)

  256 P  two frontiers of 32 bytes per node (range, pattern and band), whose capacities at least double when they grow (api/kmers.hip.h:
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
thread_local u64 t_edit_stats[4] = {0, 0, 0, 0};

// A frontier of the edit search: the three arrays of a KmerFrontier (its code array holds the pattern) and the bands, of the same capacity.
struct EditFrontier
{
  KmerFrontier f; DevBuf band;
  int reserve(u64 need)
  {
    const u64 had = f.cap;
    TRY(f.reserve(need));
    if(f.cap != had || !band.p) { TRY(band.alloc(f.cap * sizeof(u64))); }
    return BWTM_OK;
  }
  EditNodes nodes(u64 capacity) const { return EditNodes{f.sp(), f.cnt(), f.code(), band.as<u64>(), std::min(capacity, f.cap)}; }
  void swap(EditFrontier& o) { f.buf.swap(o.f.buf); std::swap(f.cap, o.f.cap); band.swap(o.band); }
};

// One batch of patterns: the search, which leaves the hit stream, every pattern's positions in it per length slot and the batch's hit
// offsets on the device, and the gather that brings the kept hits to the caller.
struct EditBatch
{
  const bwtm_index* x = nullptr;
  u32 max_edits = 0; u64 max_hits = 0;
  DevBuf d_text, d_off, d_slots, d_base, d_totals, d_out;
  u64 totals_cap = 0;
  EditFrontier cur, next;
  KmerFrontier hits;
  u64 nhits = 0, kept_total = 0;
  std::vector<u64> h_off;

  u64 slots() const { return 2 * (u64)max_edits + 1; }
  u64* first() const { return d_slots.as<u64>(); }
  u64* end(u64 nb) const { return d_slots.as<u64>() + slots() * nb; }

  // The patterns first .. first + nb - 1 of the call; hit_offsets[0 .. nb] continue hit_offsets[0] by the kept counts.
  int search(const u8* patterns, const u64* offsets, u64 nb, u64* hit_offsets)
  {
    const u64 before = hit_offsets[0];
    const u64 base = offsets[0], bytes = offsets[nb] - base;
    const IndexView v = x->view();
    h_off.resize(nb + 1);
    u64 longest = 0;
    for(u64 k = 0; k <= nb; k++) { h_off[k] = offsets[k] - base; }
    for(u64 k = 0; k < nb; k++) { longest = std::max(longest, h_off[k + 1] - h_off[k]); }
    TRY(d_text.alloc(bytes)); TRY(d_off.alloc((nb + 1) * sizeof(u64))); TRY(d_slots.alloc(2 * slots() * nb * sizeof(u64), true)); TRY(d_base.alloc((nb + 1) * sizeof(u64)));
    if(bytes > 0) { HIP_TRY(hipMemcpyAsync(d_text.p, patterns + base, bytes, hipMemcpyHostToDevice, CTX.stream)); }
    HIP_TRY(hipMemcpyAsync(d_off.p, h_off.data(), (nb + 1) * sizeof(u64), hipMemcpyHostToDevice, CTX.stream));
    TRY(cur.reserve(nb));
    LAUNCH("edit_roots", k_edit_roots, div_up(nb, BLOCK_THREADS), BLOCK_THREADS, d_off.as<const u64>(), nb, x->n, cur.nodes(nb));
    u64 count = nb, peak = nb;
    nhits = 0;
    const u64 levels = std::max<u64>(longest + max_edits, 1);                                   // a root that is a hit becomes one in the first level
    for(u64 t = 0; t < levels && count > 0; t++)
    {
      const u64 nblocks = div_up(count, BLOCK_THREADS);
      if(2 * nblocks + 1 > totals_cap)
      {
        totals_cap = std::max<u64>(2 * nblocks + 1, 2 * totals_cap);
        TRY(d_totals.alloc(totals_cap * sizeof(u64)));
      }
      u64* totals = d_totals.as<u64>();
      LAUNCH("edit_count", (k_edit_level<false>), nblocks, BLOCK_THREADS, v, d_text.as<const u8>(), bytes, d_off.as<const u64>(), nb, max_edits, t,
        (const u64*)cur.f.sp(), (const u64*)cur.f.cnt(), (const u64*)cur.f.code(), (const u64*)cur.band.as<u64>(), count, nblocks, totals,
        EditNodes{nullptr, nullptr, nullptr, nullptr, 0}, ApproxNodes{nullptr, nullptr, nullptr, 0}, (u64)0);
      TRY(device_scan<0>(totals, totals, 2 * nblocks + 1));
      TRY(fetch_u64(totals + nblocks, 0)); TRY(fetch_u64(totals + 2 * nblocks, 1));
      HIP_TRY(hipStreamSynchronize(CTX.stream));
      const u64 kept = CTX.host_scratch[0], both = CTX.host_scratch[1];
      if(kept > 5 * count || both < kept || both - kept > 6 * count)
      {
        return fail(BWTM_EINVAL, "bwtm_find_edit_batch: level %llu counted %llu children and %llu hits of %llu nodes", (unsigned long long)(t + 1), (unsigned long long)kept,
          (unsigned long long)(both - kept), (unsigned long long)count);
      }
      const u64 found = both - kept;
      t_edit_stats[0] += count; t_edit_stats[3] = std::max(t_edit_stats[3], t + 1);
      if(kept > 0) { TRY(next.reserve(kept)); }
      if(found > 0) { TRY(approx_keep(hits, nhits, nhits + found)); }
      if(both > 0)
      {
        LAUNCH("edit_expand", (k_edit_level<true>), nblocks, BLOCK_THREADS, v, d_text.as<const u8>(), bytes, d_off.as<const u64>(), nb, max_edits, t,
          (const u64*)cur.f.sp(), (const u64*)cur.f.cnt(), (const u64*)cur.f.code(), (const u64*)cur.band.as<u64>(), count, nblocks, totals,
          (kept > 0 ? next.nodes(kept) : EditNodes{nullptr, nullptr, nullptr, nullptr, 0}), approx_nodes(hits, nhits + found), nhits);
      }
      if(found > 0)
      {
        LAUNCH("edit_mark", k_edit_mark, div_up(found, BLOCK_THREADS), BLOCK_THREADS, (const u64*)hits.code(), nhits, found, d_off.as<const u64>(), nb, max_edits, first(), end(nb));
        nhits += found;
      }
      if(kept > 0) { cur.swap(next); }
      count = kept; peak = std::max(peak, kept);
    }
    t_edit_stats[1] = std::max(t_edit_stats[1], peak); t_edit_stats[2] = std::max(t_edit_stats[2], nhits);
    LAUNCH("edit_cap", k_edit_cap, div_up(nb + 1, BLOCK_THREADS), BLOCK_THREADS, (const u64*)first(), (const u64*)end(nb), nb, max_edits, max_hits, d_base.as<u64>());
    TRY(device_scan<0>(d_base.as<const u64>(), d_base.as<u64>(), nb + 1));
    HIP_TRY(hipMemcpyAsync(hit_offsets, d_base.p, (nb + 1) * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream));
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    kept_total = hit_offsets[nb];
    if(kept_total > nhits) { return fail(BWTM_EINVAL, "bwtm_find_edit_batch: %llu hits kept of %llu found", (unsigned long long)kept_total, (unsigned long long)nhits); }
    if(before != 0) { for(u64 k = 0; k <= nb; k++) { hit_offsets[k] += before; } }              // a later batch of the call
    return BWTM_OK;
  }

  // The kept hits of the batch search() has just seen, in pattern order, into the caller's arrays (any of them null).
  int fill(u64 nb, u64* out_sp, u64* out_count, u8* out_edits, u32* out_lengths)
  {
    if(kept_total == 0) { return BWTM_OK; }
    if(kept_total > (~0ull) / 24) { return fail(BWTM_ENOMEM, "bwtm_find_edit_batch: %llu hits do not fit", (unsigned long long)kept_total); }
    TRY(d_out.alloc(21 * kept_total));
    u64* o_sp = d_out.as<u64>(); u64* o_cnt = o_sp + kept_total; u32* o_len = (u32*)(o_cnt + kept_total); u8* o_ed = (u8*)(o_len + kept_total);
    LAUNCH("edit_gather", k_edit_gather, div_up(nhits, BLOCK_THREADS), BLOCK_THREADS, (const u64*)hits.sp(), (const u64*)hits.cnt(), (const u64*)hits.code(), nhits,
      d_off.as<const u64>(), nb, max_edits, (const u64*)first(), (const u64*)end(nb), d_base.as<const u64>(), o_sp, o_cnt, o_len, o_ed, kept_total);
    if(out_sp) { HIP_TRY(hipMemcpyAsync(out_sp, o_sp, kept_total * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream)); }
    if(out_count) { HIP_TRY(hipMemcpyAsync(out_count, o_cnt, kept_total * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream)); }
    if(out_lengths) { HIP_TRY(hipMemcpyAsync(out_lengths, o_len, kept_total * sizeof(u32), hipMemcpyDeviceToHost, CTX.stream)); }
    if(out_edits) { HIP_TRY(hipMemcpyAsync(out_edits, o_ed, kept_total, hipMemcpyDeviceToHost, CTX.stream)); }
    HIP_TRY(hipStreamSynchronize(CTX.stream));                                                  // the batch's buffers are reused
    return BWTM_OK;
  }
};

// The two rounds of approx_run: every batch is searched, so that hit_offsets is complete and the capacity is checked before anything
// else is written; then the hits are gathered, a call of several batches searching each a second time.
int edit_run(const bwtm_index* x, const u8* patterns, const u64* offsets, u64 count, u32 max_edits, u64 max_hits, u64* hit_offsets,
             u64* out_sp, u64* out_count, u8* out_edits, u32* out_lengths, u64 capacity)
{
  const u64 batch = std::min(approx_batch_size(), count);
  const bool single = (batch >= count);
  EditBatch b;
  b.x = x; b.max_edits = max_edits; b.max_hits = max_hits;
  for(u64 done = 0; done < count; done += batch)
  {
    TRY(b.search(patterns, offsets + done, std::min(batch, count - done), hit_offsets + done));
  }
  const u64 total = hit_offsets[count];
  if((!out_sp && !out_count && !out_edits && !out_lengths) || capacity == 0 || total == 0) { return BWTM_OK; }       // sizes only
  if(capacity < total)
  {
    return fail(BWTM_EINVAL, "bwtm_find_edit_batch: capacity %llu is too small (%llu hits)", (unsigned long long)capacity, (unsigned long long)total);
  }
  const u64 s0 = t_edit_stats[0];
  for(u64 done = 0; done < count; done += batch)
  {
    const u64 nb = std::min(batch, count - done);
    const u64 at = hit_offsets[done];
    if(!single)
    {
      TRY(b.search(patterns, offsets + done, nb, hit_offsets + done));
      t_edit_stats[0] = s0;                                                                     // the same nodes a second time
    }
    TRY(b.fill(nb, (out_sp ? out_sp + at : nullptr), (out_count ? out_count + at : nullptr), (out_edits ? out_edits + at : nullptr), (out_lengths ? out_lengths + at : nullptr)));
  }
  return BWTM_OK;
}

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
  for(u32 j = 0; j < 4; j++) { t_edit_stats[j] = 0; }
  hit_offsets[0] = 0;
  if(count == 0) { return BWTM_OK; }
  for(u64 k = 0; k < count; k++)
  {
    if(offsets[k] > offsets[k + 1]) { return fail(BWTM_EINVAL, "bwtm_find_edit_batch: offsets must not decrease (pattern %llu)", (unsigned long long)k); }
    const u64 len = offsets[k + 1] - offsets[k];
    if(len > APPROX_MAX_LEN)
    {
      return fail(BWTM_EINVAL, "bwtm_find_edit_batch: pattern %llu has %llu symbols (at most %llu)", (unsigned long long)k, (unsigned long long)len, (unsigned long long)APPROX_MAX_LEN);
    }
    if(len > 0 && !patterns) { return fail(BWTM_EINVAL, "bwtm_find_edit_batch: null pattern text"); }
    for(u64 p = offsets[k]; p < offsets[k + 1]; p++)
    {
      if(patterns[p] < 1 || patterns[p] > 5)
      {
        return fail(BWTM_EINVAL, "bwtm_find_edit_batch: pattern %llu holds the symbol %u at offset %llu (comp values 1..5)", (unsigned long long)k, (unsigned)patterns[p],
          (unsigned long long)(p - offsets[k]));
      }
    }
  }
  const int rc = edit_run(x, patterns, offsets, count, max_edits, max_hits, hit_offsets, out_sp, out_count, out_edits, out_lengths, capacity);
  if(rc != BWTM_OK) { (void)hipStreamSynchronize(CTX.stream); }                                 // the half-built state goes back to the pool behind this
  return rc;
}

extern "C" int bwtm_find_edit_stats(uint64_t stats[4])
{
  if(!stats) { return fail(BWTM_EINVAL, "bwtm_find_edit_stats: null argument"); }
  for(u32 j = 0; j < 4; j++) { stats[j] = t_edit_stats[j]; }
  return BWTM_OK;
}
