/*
  api/frontier.hip.h -- the host side of the level scheme of kernels/level.hip.h, stated once for api/kmers.hip.h, api/kmer_join.hip.h,
  api/approx.hip.h and api/edit.hip.h: the frontier of parallel u64 arrays, the totals of a level with their scan and read-back, and what
  the two pattern searches share of a batch and of a call.  Part of bwtm_api.hip.

  The memory argument behind every bound of those four files.  A level's size is known only after its count pass, and a block the pool
  has handed out and taken back stays with the pool: a frontier that grew by a little every level would leave a block per level behind.
  So a frontier's capacity AT LEAST DOUBLES when it grows: the blocks one frontier ever had hold fewer than 4 P nodes together, P the
  most nodes it ever held (the last block fewer than 2 P, the earlier ones a geometric series below it).  Two ping-pong frontiers of
  8 ARRAYS bytes per node are therefore 64 ARRAYS P bytes.  A stream that keeps its contents while it grows (grow_keeping) doubles the
  same way, the block being copied from included.  The totals of a level (8 STREAMS bytes per workgroup of nodes) double as well.
*/
#pragma once

namespace
{

// ARRAYS parallel arrays of `cap` u64 each in one block: a frontier, a hit stream, or a result.  `who` is the entry point for the error text.
template<u32 ARRAYS>
struct Frontier
{
  DevBuf buf; u64 cap = 0;
  u64* array(u32 w) const { return buf.as<u64>() + w * cap; }
  void swap(Frontier& o) { buf.swap(o.buf); std::swap(cap, o.cap); }
  // room for `need` nodes; the old contents are not kept
  int reserve(u64 need, const char* who)
  {
    if(need <= cap && buf.p) { return BWTM_OK; }
    const u64 want = std::max<u64>(std::max<u64>(need, 2 * cap), 1);
    if(want > (~0ull) / (8 * ARRAYS)) { return fail(BWTM_ENOMEM, "%s: a frontier of %llu nodes does not fit", who, (unsigned long long)want); }
    TRY(buf.alloc(ARRAYS * want * sizeof(u64)));
    cap = want;
    return BWTM_OK;
  }
  // room for `need` nodes, of which the first `used` are kept; the old block returns to the pool (stream ordered)
  int grow_keeping(u64 used, u64 need, const char* who)
  {
    if(need <= cap && buf.p) { return BWTM_OK; }
    Frontier grown;
    grown.cap = cap;                                                                            // reserve() at least doubles this
    TRY(grown.reserve(need, who));
    return move_into(grown, used);
  }
  // the first `count` >= 1 nodes in a block of exactly that size
  int shrink_to(u64 count, const char* who)
  {
    if(cap == count) { return BWTM_OK; }
    Frontier exact;
    TRY(exact.reserve(count, who));
    return move_into(exact, count);
  }
private:
  int move_into(Frontier& other, u64 count)
  {
    for(u32 w = 0; w < ARRAYS && count > 0; w++)
    {
      HIP_TRY(hipMemcpyAsync(other.array(w), array(w), count * sizeof(u64), hipMemcpyDeviceToDevice, CTX.stream));
    }
    swap(other);
    return BWTM_OK;
  }
};

// The per-workgroup totals of a level: `streams` runs of `nblocks` entries and one more (kernels/level.hip.h).
struct LevelTotals
{
  DevBuf buf; u64 cap = 0;
  u64* p() const { return buf.as<u64>(); }
  int reserve(u32 streams, u64 nblocks)
  {
    const u64 need = streams * nblocks + 1;
    if(need <= cap) { return BWTM_OK; }
    const u64 want = std::max<u64>(need, 2 * cap);
    TRY(buf.alloc(want * sizeof(u64)));
    cap = want;
    return BWTM_OK;
  }
  // Behind the count pass: the scan, and CTX.host_scratch[i] = the end of stream first_stream_read + i - 1, up to the last one.
  int scan_and_read(u32 streams, u64 nblocks, u32 first_stream_read)
  {
    TRY(device_scan<0>(p(), p(), streams * nblocks + 1));
    for(u32 s = first_stream_read; s <= streams; s++) { TRY(fetch_u64(p() + s * nblocks, s - first_stream_read)); }
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    return BWTM_OK;
  }
};

u64 pattern_batch_size() { return std::min<u64>((u64)g_tune.approx_batch, WALK_BATCH_LIMIT); }

// Where a pattern search's hits go: the caller's arrays, any of them null.  cost = mismatches or edits; lengths only for the edit search.
struct PatternHits
{
  u64* sp; u64* count; u8* cost; u32* lengths;
  bool any() const { return sp || count || cost || lengths; }
  PatternHits at(u64 i) const { return PatternHits{sp ? sp + i : nullptr, count ? count + i : nullptr, cost ? cost + i : nullptr, lengths ? lengths + i : nullptr}; }
};

// What one batch of patterns is to both searches: its text and offsets on the device, the hit stream (sp, count, meta) of its levels,
// every pattern's slots in it, and the batch's hit offsets.
struct PatternBatch
{
  const bwtm_index* x = nullptr;
  u32 max_cost = 0; u64 max_hits = 0;                   // the search's budget of mismatches or edits; hits kept per pattern (0: all)
  DevBuf d_text, d_off, d_slots, d_base, d_out;
  LevelTotals totals;
  Frontier<3> hits;
  u64 nhits = 0, kept_total = 0;
  u64 bytes = 0, longest = 0;                           // of the staged batch: its text, its longest pattern
  std::vector<u64> h_off;

  ApproxNodes hit_nodes(u64 capacity) const { return ApproxNodes{hits.array(0), hits.array(1), hits.array(2), std::min(capacity, hits.cap)}; }

  // The patterns of offsets[0 .. nb] to the device, `slot_words` zeroed u64 for the marks, and an empty hit stream.
  int stage(const u8* patterns, const u64* offsets, u64 nb, u64 slot_words)
  {
    const u64 base = offsets[0];
    bytes = offsets[nb] - base; longest = 0; nhits = 0;
    h_off.resize(nb + 1);
    for(u64 k = 0; k <= nb; k++) { h_off[k] = offsets[k] - base; }
    for(u64 k = 0; k < nb; k++) { longest = std::max(longest, h_off[k + 1] - h_off[k]); }
    TRY(d_text.alloc(bytes)); TRY(d_off.alloc((nb + 1) * sizeof(u64))); TRY(d_slots.alloc(slot_words * sizeof(u64), true)); TRY(d_base.alloc((nb + 1) * sizeof(u64)));
    if(bytes > 0) { HIP_TRY(hipMemcpyAsync(d_text.p, patterns + base, bytes, hipMemcpyHostToDevice, CTX.stream)); }
    HIP_TRY(hipMemcpyAsync(d_off.p, h_off.data(), (nb + 1) * sizeof(u64), hipMemcpyHostToDevice, CTX.stream));
    return BWTM_OK;
  }

  // d_base[0 .. nb] holds the capped counts: hit_offsets[0 .. nb] = their scan, continuing `before`, the hits of the call's earlier batches.
  int finish_offsets(const char* who, u64 nb, u64 before, u64* hit_offsets)
  {
    TRY(device_scan<0>(d_base.as<const u64>(), d_base.as<u64>(), nb + 1));
    HIP_TRY(hipMemcpyAsync(hit_offsets, d_base.p, (nb + 1) * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream));
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    kept_total = hit_offsets[nb];
    if(kept_total > nhits) { return fail(BWTM_EINVAL, "%s: %llu hits kept of %llu found", who, (unsigned long long)kept_total, (unsigned long long)nhits); }
    if(before != 0) { for(u64 k = 0; k <= nb; k++) { hit_offsets[k] += before; } }
    return BWTM_OK;
  }
};

// A call of a pattern search, over a Batch with search() and fill().  First every batch is searched, so that hit_offsets is complete and
// the capacity is checked before anything else is written; then the hits are gathered.  A call of one batch keeps its hit stream between
// the two; a call of several searches every batch a second time (the streams of all batches do not stay anywhere: the memory is that of
// one batch).  stats[0] counts the nodes expanded, once.
template<class Batch>
int pattern_run(const char* who, u64* stats, const bwtm_index* x, const u8* patterns, const u64* offsets, u64 count, u32 max_cost, u64 max_hits, u64* hit_offsets,
                const PatternHits& out, u64 capacity)
{
  const u64 batch = std::min(pattern_batch_size(), count);
  const bool single = (batch >= count);
  Batch b;
  b.x = x; b.max_cost = max_cost; b.max_hits = max_hits;
  for(u64 done = 0; done < count; done += batch)
  {
    TRY(b.search(patterns, offsets + done, std::min(batch, count - done), hit_offsets + done));
  }
  const u64 total = hit_offsets[count];
  if(!out.any() || capacity == 0 || total == 0) { return BWTM_OK; }                             // sizes only
  if(capacity < total) { return fail(BWTM_EINVAL, "%s: capacity %llu is too small (%llu hits)", who, (unsigned long long)capacity, (unsigned long long)total); }
  const u64 s0 = stats[0];
  for(u64 done = 0; done < count; done += batch)
  {
    const u64 nb = std::min(batch, count - done);
    const u64 at = hit_offsets[done];
    if(!single)
    {
      TRY(b.search(patterns, offsets + done, nb, hit_offsets + done));
      stats[0] = s0;                                                                            // the same nodes a second time
    }
    TRY(b.fill(nb, out.at(at)));
  }
  return BWTM_OK;
}

// The patterns of a call: offsets that do not decrease, lengths the nodes can hold, comp values 1..5.
int validate_patterns(const char* who, const u8* patterns, const u64* offsets, u64 count)
{
  for(u64 k = 0; k < count; k++)
  {
    if(offsets[k] > offsets[k + 1]) { return fail(BWTM_EINVAL, "%s: offsets must not decrease (pattern %llu)", who, (unsigned long long)k); }
    const u64 len = offsets[k + 1] - offsets[k];
    if(len > APPROX_MAX_LEN)
    {
      return fail(BWTM_EINVAL, "%s: pattern %llu has %llu symbols (at most %llu)", who, (unsigned long long)k, (unsigned long long)len, (unsigned long long)APPROX_MAX_LEN);
    }
    if(len > 0 && !patterns) { return fail(BWTM_EINVAL, "%s: null pattern text", who); }
    for(u64 p = offsets[k]; p < offsets[k + 1]; p++)
    {
      if(patterns[p] < 1 || patterns[p] > 5)
      {
        return fail(BWTM_EINVAL, "%s: pattern %llu holds the symbol %u at offset %llu (comp values 1..5)", who, (unsigned long long)k, (unsigned)patterns[p],
          (unsigned long long)(p - offsets[k]));
      }
    }
  }
  return BWTM_OK;
}

} // namespace
