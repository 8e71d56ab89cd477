/*
  api/overlap.hip.h -- suffix-prefix overlaps of a batch of queries against the collection (bwtm_overlap_batch, bwtm_overlap_sequences):
  one backward search per query, its rank(., 0) pairs looked up in the locator's table (kernels/overlap.hip.h).  Part of bwtm_api.hip.
  Batches: see api/batches.hip.h.
*/
#pragma once

namespace
{
u64 overlap_batch_size() { return std::min<u64>((u64)g_tune.overlap_batch, WALK_BATCH_LIMIT); }

// One batch of queries whose text and offsets are on the device: the count pass, two scans on the device that turn its counts into the
// first record and the first hit slot of every query, the emit pass and the expansion in hit batches of locate_batch.  Of the counts only
// the batch's hit offsets travel, straight into the caller's hit_offsets.  Device memory: 24 bytes per query, 32 per interval record (at
// most one per symbol of the batch's text, allocated at the exact number) and 16 per hit of one hit batch.
struct OverlapBatch
{
  const bwtm_locator* loc = nullptr;
  u64 min_overlap = 0, max_hits = 0;
  DevBuf d_rbase;       // batch + 1: intervals per query, scanned in place into the first record of every query
  DevBuf d_nhits;       // batch: hits per query before max_hits
  DevBuf d_hbase;       // batch + 1: hits kept per query, scanned in place into the first hit slot of every query
  DevBuf d_recs, d_ids, d_len;
  StatusCell status;
  u64 nrecs = 0, kept_total = 0;

  int alloc(u64 batch)
  {
    TRY(d_rbase.alloc((batch + 1) * sizeof(u64))); TRY(d_nhits.alloc(batch * sizeof(u64))); TRY(d_hbase.alloc((batch + 1) * sizeof(u64)));
    TRY(status.alloc());
    return BWTM_OK;
  }
  OverlapRecs recs() const
  {
    OverlapRecs r;
    r.first = d_recs.as<u64>(); r.z0 = r.first + nrecs; r.cnt = r.z0 + nrecs; r.len = r.cnt + nrecs;
    return r;
  }
  // One pass of the search over the batch: the count pass, or the emit pass into recs().
  int scan(bool emit, const u8* d_text, const u64* d_off, u64 nb)
  {
    const OverlapRecs r = (emit ? recs() : OverlapRecs());
    const IndexView v = loc->index->view();
#ifdef BWTM_DIAGNOSTICS
    if(g_tune.overlap_kernel == 1)                                                              // the A/B partner: one lane per query
    {
      const u64 lane_grid = div_up(nb, BLOCK_THREADS);
      if(emit) { LAUNCH("overlap_scan", (k_overlap_scan_lane<true>), lane_grid, BLOCK_THREADS, v, d_text, d_off, nb, min_overlap, max_hits, d_rbase.as<u64>(), d_nhits.as<u64>(), d_hbase.as<u64>(), r); }
      else { LAUNCH("overlap_scan", (k_overlap_scan_lane<false>), lane_grid, BLOCK_THREADS, v, d_text, d_off, nb, min_overlap, max_hits, d_rbase.as<u64>(), d_nhits.as<u64>(), d_hbase.as<u64>(), r); }
      return BWTM_OK;
    }
#endif
    const u64 grid = div_up(4 * nb, BLOCK_THREADS);
    if(emit) { LAUNCH("overlap_scan", (k_overlap_scan<true>), grid, BLOCK_THREADS, v, d_text, d_off, nb, min_overlap, max_hits, d_rbase.as<u64>(), d_nhits.as<u64>(), d_hbase.as<u64>(), r); }
    else { LAUNCH("overlap_scan", (k_overlap_scan<false>), grid, BLOCK_THREADS, v, d_text, d_off, nb, min_overlap, max_hits, d_rbase.as<u64>(), d_nhits.as<u64>(), d_hbase.as<u64>(), r); }
    return BWTM_OK;
  }
  // The count pass over nb queries: hit_offsets[1 .. nb] continue hit_offsets[0] by the kept counts; the bases of the emit pass stay on the device.
  int count(const u8* d_text, const u64* d_off, u64 nb, u64* hit_offsets)
  {
    const u64 before = hit_offsets[0];
    TRY(scan(false, d_text, d_off, nb));
    TRY(device_scan<0>(d_rbase.as<const u64>(), d_rbase.as<u64>(), nb + 1));
    TRY(device_scan<0>(d_hbase.as<const u64>(), d_hbase.as<u64>(), nb + 1));
    TRY(fetch_u64(d_rbase.as<u64>() + nb, 1));
    TRY(to_host(hit_offsets, d_hbase.as<const u64>(), nb + 1));
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    nrecs = CTX.host_scratch[1]; kept_total = hit_offsets[nb];
    if(before != 0) { for(u64 k = 0; k <= nb; k++) { hit_offsets[k] += before; } }              // a later batch of the call
    return BWTM_OK;
  }
  // The emit pass over the batch count() has just seen, then its kept_total hits, locate_batch at a time, into out_ids / out_lengths.
  // *bad = the first hit of the batch that failed, or SEQ_STATUS_NONE.
  int expand(const u8* d_text, const u64* d_off, u64 nb, u64* out_ids, u64* out_lengths, u64* bad)
  {
    *bad = SEQ_STATUS_NONE;
    if(kept_total == 0) { return BWTM_OK; }
    TRY(d_recs.alloc(4 * nrecs * sizeof(u64)));
    TRY(scan(true, d_text, d_off, nb));
    const u64 batch = std::min(locate_batch_size(), kept_total);
    TRY(d_ids.alloc(batch * sizeof(u64))); TRY(d_len.alloc(batch * sizeof(u64)));
    for(u64 done = 0; done < kept_total; done += batch)
    {
      const u64 nh = std::min(batch, kept_total - done);
      TRY(status.arm());
      LAUNCH("overlap_expand", k_overlap_expand, div_up(nh, BLOCK_THREADS), BLOCK_THREADS, loc->table.as<const u64>(), loc->index->m, recs(), nrecs, done, nh,
        d_ids.as<u64>(), d_len.as<u64>(), status.word());
      u64 slot = 0;
      TRY(status.read(&slot));
      if(slot != SEQ_STATUS_NONE) { *bad = done + slot; return BWTM_OK; }                         // nothing of a failed batch reaches the caller
      TRY(to_host(out_ids + done, d_ids.as<const u64>(), nh)); TRY(to_host(out_lengths + done, d_len.as<const u64>(), nh));
      HIP_TRY(hipStreamSynchronize(CTX.stream));                                                // the batch's buffers are reused
    }
    return BWTM_OK;
  }
};

// Both calls: prepare(done, nb, &d_text, &d_off) puts the text and the nb + 1 batch-local offsets of the queries done .. done + nb - 1 on
// the device.  Batches of overlap_batch_size() in the two rounds of api/batches.hip.h: counted, then emitted and expanded.
template<class Prepare>
int overlap_run(const char* who, const bwtm_locator* loc, u64 count, u64 min_overlap, u64 max_hits, u64* hit_offsets, u64* out_ids, u64* out_lengths,
                u64 capacity, Prepare&& prepare)
{
  const u64 batch = std::min(overlap_batch_size(), count);
  OverlapBatch b;
  b.loc = loc; b.min_overlap = min_overlap; b.max_hits = max_hits;
  TRY(b.alloc(batch));
  const u8* d_text = nullptr; const u64* d_off = nullptr;
  auto size = [&](u64 done, u64 nb, u64* batch_offsets) -> int
  {
    TRY(prepare(done, nb, &d_text, &d_off));
    TRY(b.count(d_text, d_off, nb, batch_offsets));
    // A call that will fill needs both arrays, and says so before the capacity is looked at.  "Will fill" is two_round_call's own condition
    // for going past "sizes only" (an array wanted, a capacity, something found), known here with the last batch's count: the two change together.
    if(done + nb == count && out_ids && capacity > 0 && batch_offsets[nb] > 0 && !out_lengths) { return fail(BWTM_EINVAL, "%s: null argument", who); }
    return BWTM_OK;
  };
  auto fill = [&](u64, u64 nb, u64 at) -> int
  {
    u64 bad = 0;
    TRY(b.expand(d_text, d_off, nb, out_ids + at, out_lengths + at, &bad));
    if(bad == SEQ_STATUS_NONE) { return BWTM_OK; }
    return fail(BWTM_EINVAL, "%s: hit %llu has no sequence in the locator's table (the index or the table is damaged)", who, (unsigned long long)(at + bad));
  };
  return two_round_call(who, "hits", count, hit_offsets, out_ids != nullptr, capacity, nullptr, [&](u64 done) { return std::min(batch, count - done); }, size, fill);
}

} // namespace

extern "C" int bwtm_overlap_batch(const bwtm_locator* loc, const uint8_t* queries, const uint64_t* offsets, uint64_t count, uint64_t min_overlap, uint64_t max_hits,
                                  uint64_t* hit_offsets, uint64_t* out_ids, uint64_t* out_lengths, uint64_t capacity)
{
  if(!loc || !hit_offsets || (count > 0 && !offsets)) { return fail(BWTM_EINVAL, "bwtm_overlap_batch: null argument"); }
  ENTER(loc->ctx);
  if(min_overlap == 0) { return fail(BWTM_EINVAL, "bwtm_overlap_batch: min_overlap must be at least 1"); }
  hit_offsets[0] = 0;
  if(count == 0) { return BWTM_OK; }
  TRY(validate_texts("bwtm_overlap_batch", "query", queries, offsets, count, 0));
  StagedTexts t;
  auto prepare = [&](u64 done, u64 nb, const u8** text_out, const u64** off_out) -> int
  {
    TRY(t.stage(queries, offsets + done, nb));
    *text_out = t.d_text.as<const u8>(); *off_out = t.d_off.as<const u64>();
    return BWTM_OK;
  };
  return overlap_run("bwtm_overlap_batch", loc, count, min_overlap, max_hits, hit_offsets, out_ids, out_lengths, capacity, prepare);
}

// The queries are extracted on the device, batch by batch (the stage of bwtm_sequences_extract), and searched where they are.
extern "C" int bwtm_overlap_sequences(const bwtm_locator* loc, const uint64_t* ids, uint64_t first_id, uint64_t count, uint64_t min_overlap, uint64_t max_hits,
                                      uint64_t* hit_offsets, uint64_t* out_ids, uint64_t* out_lengths, uint64_t capacity)
{
  if(!loc || !hit_offsets) { return fail(BWTM_EINVAL, "bwtm_overlap_sequences: null argument"); }
  ENTER(loc->ctx);
  const bwtm_index* x = loc->index;
  if(min_overlap == 0) { return fail(BWTM_EINVAL, "bwtm_overlap_sequences: min_overlap must be at least 1"); }
  hit_offsets[0] = 0;
  if(count == 0) { return BWTM_OK; }
  TRY(check_sequence_ids("bwtm_overlap_sequences", x, ids, first_id, count));
  SeqBatch s;
  TRY(s.alloc(std::min(overlap_batch_size(), count), ids != nullptr, true, false));           // lengths and offsets stay on the device
  auto prepare = [&](u64 done, u64 nb, const u8** text_out, const u64** off_out) -> int
  {
    TRY(s.offsets_on_device("bwtm_overlap_sequences", "the locator's max_len", x, at_or_null(ids, done), first_id + done, nb, loc->max_len));
    TRY(fetch_u64(s.d_off.as<u64>() + nb, 1));
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    TRY(s.emit(x, at_or_null(ids, done), first_id + done, nb, CTX.host_scratch[1]));      // the text at its exact size
    *text_out = s.d_text.as<const u8>(); *off_out = s.d_off.as<const u64>();
    return BWTM_OK;
  };
  return overlap_run("bwtm_overlap_sequences", loc, count, min_overlap, max_hits, hit_offsets, out_ids, out_lengths, capacity, prepare);
}
