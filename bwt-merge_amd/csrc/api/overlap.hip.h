/*
  api/overlap.hip.h -- suffix-prefix overlaps of a batch of queries against the collection (bwtm_overlap_batch, bwtm_overlap_sequences):
  one backward search per query, its rank(., 0) pairs looked up in the locator's table (kernels/overlap.hip.h).  Part of bwtm_api.hip.
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
    HIP_TRY(hipMemcpyAsync(hit_offsets, d_hbase.p, (nb + 1) * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream));
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
      HIP_TRY(hipMemcpyAsync(out_ids + done, d_ids.p, nh * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream));
      HIP_TRY(hipMemcpyAsync(out_lengths + done, d_len.p, nh * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream));
      HIP_TRY(hipStreamSynchronize(CTX.stream));                                                // the batch's buffers are reused
    }
    return BWTM_OK;
  }
};

// Both calls: prepare(done, nb, &d_text, &d_off) puts the text and the nb + 1 batch-local offsets of the queries done .. done + nb - 1 on
// the device.  First every batch is counted, so that hit_offsets is complete and the capacity is checked before anything else is written;
// then every batch is emitted and expanded.  A call of one batch keeps its text and counts between the two; a call of several prepares
// and counts every batch a second time (the counts of all batches do not stay anywhere: the memory is that of one batch).
template<class Prepare>
int overlap_run(const char* who, const bwtm_locator* loc, u64 count, u64 min_overlap, u64 max_hits, u64* hit_offsets, u64* out_ids, u64* out_lengths,
                u64 capacity, Prepare&& prepare)
{
  const u64 batch = std::min(overlap_batch_size(), count);
  const bool single = (batch >= count);
  OverlapBatch b;
  b.loc = loc; b.min_overlap = min_overlap; b.max_hits = max_hits;
  TRY(b.alloc(batch));
  const u8* d_text = nullptr; const u64* d_off = nullptr;
  for(u64 done = 0; done < count; done += batch)
  {
    const u64 nb = std::min(batch, count - done);
    TRY(prepare(done, nb, &d_text, &d_off));
    TRY(b.count(d_text, d_off, nb, hit_offsets + done));
  }
  const u64 total = hit_offsets[count];
  if(!out_ids || capacity == 0 || total == 0) { return BWTM_OK; }                               // sizes only
  if(!out_lengths) { return fail(BWTM_EINVAL, "%s: null argument", who); }
  if(capacity < total) { return fail(BWTM_EINVAL, "%s: capacity %llu is too small (%llu hits)", who, (unsigned long long)capacity, (unsigned long long)total); }
  for(u64 done = 0; done < count; done += batch)
  {
    const u64 nb = std::min(batch, count - done);
    if(!single)
    {
      TRY(prepare(done, nb, &d_text, &d_off));
      TRY(b.count(d_text, d_off, nb, hit_offsets + done));
    }
    u64 bad = 0;
    TRY(b.expand(d_text, d_off, nb, out_ids + hit_offsets[done], out_lengths + hit_offsets[done], &bad));
    if(bad != SEQ_STATUS_NONE)
    {
      return fail(BWTM_EINVAL, "%s: hit %llu has no sequence in the locator's table (the index or the table is damaged)", who, (unsigned long long)(hit_offsets[done] + bad));
    }
  }
  return BWTM_OK;
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
  for(u64 k = 0; k < count; k++)
  {
    if(offsets[k] > offsets[k + 1]) { return fail(BWTM_EINVAL, "bwtm_overlap_batch: offsets must not decrease (query %llu)", (unsigned long long)k); }
  }
  if(offsets[count] > offsets[0] && !queries) { return fail(BWTM_EINVAL, "bwtm_overlap_batch: null query text"); }
  for(u64 k = 0; k < count; k++)
  {
    for(u64 p = offsets[k]; p < offsets[k + 1]; p++)
    {
      if(queries[p] < 1 || queries[p] > 5)
      {
        return fail(BWTM_EINVAL, "bwtm_overlap_batch: query %llu holds the symbol %u at offset %llu (comp values 1..5)", (unsigned long long)k, (unsigned)queries[p],
          (unsigned long long)(p - offsets[k]));
      }
    }
  }
  DevBuf d_text, d_off;
  std::vector<u64> h_off;
  auto prepare = [&](u64 done, u64 nb, const u8** text_out, const u64** off_out) -> int
  {
    const u64 base = offsets[done], bytes = offsets[done + nb] - base;
    h_off.resize(nb + 1);
    for(u64 k = 0; k <= nb; k++) { h_off[k] = offsets[done + k] - base; }
    TRY(d_text.alloc(bytes)); TRY(d_off.alloc((nb + 1) * sizeof(u64)));
    if(bytes > 0) { HIP_TRY(hipMemcpyAsync(d_text.p, queries + base, bytes, hipMemcpyHostToDevice, CTX.stream)); }
    HIP_TRY(hipMemcpyAsync(d_off.p, h_off.data(), (nb + 1) * sizeof(u64), hipMemcpyHostToDevice, CTX.stream));
    HIP_TRY(hipStreamSynchronize(CTX.stream));                                                  // h_off is reused
    *text_out = d_text.as<const u8>(); *off_out = d_off.as<const u64>();
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
    u64 bad = 0;
    TRY(s.lengths(x, (ids ? ids + done : nullptr), first_id + done, nb, loc->max_len, &bad));
    if(bad != SEQ_STATUS_NONE)
    {
      bad += done;
      return fail(BWTM_EINVAL, "bwtm_overlap_sequences: sequence %llu is longer than the locator's max_len = %llu (or the index is damaged)",
        (unsigned long long)(ids ? ids[bad] : first_id + bad), (unsigned long long)loc->max_len);
    }
    LAUNCH("overlap_widen", k_overlap_widen, div_up(nb + 1, BLOCK_THREADS), BLOCK_THREADS, s.d_len.as<const u32>(), nb, s.d_off.as<u64>());
    TRY(device_scan<0>(s.d_off.as<const u64>(), s.d_off.as<u64>(), nb + 1));
    TRY(fetch_u64(s.d_off.as<u64>() + nb, 1));
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    TRY(s.emit(x, (ids ? ids + done : nullptr), first_id + done, nb, CTX.host_scratch[1]));    // the text at its exact size
    *text_out = s.d_text.as<const u8>(); *off_out = s.d_off.as<const u64>();
    return BWTM_OK;
  };
  return overlap_run("bwtm_overlap_sequences", loc, count, min_overlap, max_hits, hit_offsets, out_ids, out_lengths, capacity, prepare);
}
