/*
  api/locate.hip.h -- from BWT positions to (sequence id, offset): the locator of an index (bwtm_locator_*), positions and ranges located
  batch by batch (bwtm_locate_batch, bwtm_locate_ranges).  Part of bwtm_api.hip.
*/
#pragma once

// The table start_to_id of one index (kernels/locate.hip.h).  It borrows the index: the index outlives it and is not consumed meanwhile.
struct bwtm_locator
{
  bwtm_context* ctx = nullptr;
  bwtm_locator() : ctx(t_ctx) { if(ctx) { ctx->live_handles++; } }
  ~bwtm_locator() { if(ctx) { ctx->live_handles--; } }
  bwtm_locator(const bwtm_locator&) = delete; bwtm_locator& operator=(const bwtm_locator&) = delete;
  const bwtm_index* index = nullptr;
  DevBuf table;                       // m u64: id of the sequence whose whole-sequence suffix is the k-th in BWT order
  u64 max_len = 0;                    // no sequence is longer (checked by the build), so no walk of a locate call is
};

namespace
{
u64 locate_batch_size() { return std::min<u64>((u64)g_tune.locate_batch, WALK_BATCH_LIMIT); }

// The table of `loc`: filled with LOCATE_UNSET, one k_locate_build per batch of sequences, then the count of entries nobody claimed.
int locator_build(bwtm_locator* loc)
{
  const bwtm_index* x = loc->index;
  const u64 m = x->m;
  TRY(loc->table.alloc(m * sizeof(u64)));
  if(m == 0) { return BWTM_OK; }
  StatusCell status;
  DevBuf d_unclaimed;                                                                           // the check's count
  TRY(status.alloc()); TRY(d_unclaimed.alloc(sizeof(u64)));
  HIP_TRY(hipMemsetAsync(loc->table.p, 0xFF, m * sizeof(u64), CTX.stream));                     // LOCATE_UNSET
  const u64 batch = std::min(locate_batch_size(), m);
  for(u64 done = 0; done < m; done += batch)
  {
    const u64 nb = std::min(batch, m - done);
    TRY(status.arm());
    LAUNCH("locate_build", k_locate_build, div_up(4 * nb, BLOCK_THREADS), BLOCK_THREADS, x->view(), done, nb, (u32)loc->max_len, loc->table.as<u64>(),
      status.word());
    u64 bad = 0;
    TRY(status.read(&bad));
    if(bad != SEQ_STATUS_NONE)
    {
      return fail(BWTM_EINVAL, "bwtm_locator_create: sequence %llu is longer than max_len = %llu (or the index is damaged)",
        (unsigned long long)(done + bad), (unsigned long long)loc->max_len);
    }
  }
  HIP_TRY(hipMemsetAsync(d_unclaimed.p, 0, sizeof(u64), CTX.stream));
  LAUNCH("locate_check", k_locate_check, std::min<u64>(div_up(m, BLOCK_THREADS), 1024), BLOCK_THREADS, loc->table.as<const u64>(), m, d_unclaimed.as<unsigned long long>());
  TRY(fetch_u64(d_unclaimed.as<u64>(), 0));
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  if(CTX.host_scratch[0] != 0)
  {
    return fail(BWTM_EINVAL, "bwtm_locator_create: the index is damaged (%llu of its %llu sequences have no start of their own)", (unsigned long long)CTX.host_scratch[0],
      (unsigned long long)m);
  }
  return BWTM_OK;
}

// The device buffers of one batch of hits, and its launch.
struct LocateBatch
{
  DevBuf d_pos, d_start, d_first, d_ids, d_offs;
  StatusCell status;
  int alloc(u64 batch, bool positions)
  {
    if(positions) { TRY(d_pos.alloc(batch * sizeof(u64))); }
    else { TRY(d_start.alloc(batch * sizeof(u64))); TRY(d_first.alloc(batch * sizeof(u64))); }
    TRY(d_ids.alloc(batch * sizeof(u64))); TRY(d_offs.alloc(batch * sizeof(u64))); TRY(status.alloc());
    return BWTM_OK;
  }
  // nb hits (positions in d_pos, or `nranges` ranges in d_start / d_first) -> out_ids / out_offsets; *bad = the first slot that failed, or SEQ_STATUS_NONE
  int run(const bwtm_locator* loc, bool positions, u64 nranges, u64 nb, u64* out_ids, u64* out_offsets, u64* bad)
  {
    TRY(status.arm());
    LAUNCH("locate", k_locate, div_up(4 * nb, BLOCK_THREADS), BLOCK_THREADS, loc->index->view(), loc->table.as<const u64>(),
      (positions ? d_pos.as<const u64>() : (const u64*)nullptr), d_start.as<const u64>(), d_first.as<const u64>(), nranges, nb, (u32)loc->max_len,
      d_ids.as<u64>(), d_offs.as<u64>(), status.word());
    TRY(status.read(bad));
    if(*bad != SEQ_STATUS_NONE) { return BWTM_OK; }                                             // nothing of a failed batch reaches the caller
    HIP_TRY(hipMemcpyAsync(out_ids, d_ids.p, nb * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream));
    HIP_TRY(hipMemcpyAsync(out_offsets, d_offs.p, nb * sizeof(u64), hipMemcpyDeviceToHost, CTX.stream));
    HIP_TRY(hipStreamSynchronize(CTX.stream));                                                  // the batch's buffers are reused
    return BWTM_OK;
  }
};

} // namespace

extern "C" int bwtm_locator_create(const bwtm_index* x, uint64_t max_len, bwtm_locator** out)
{
  if(!x || !out) { return fail(BWTM_EINVAL, "bwtm_locator_create: null argument"); }
  WHOLE_INDEX(x, "bwtm_locator_create");
  ENTER(x->ctx);
  TRY(check_max_len("bwtm_locator_create", &max_len));
  bwtm_locator* loc = new bwtm_locator();
  loc->index = x; loc->max_len = max_len;
  const int rc = locator_build(loc);
  if(rc != BWTM_OK) { (void)hipStreamSynchronize(CTX.stream); delete loc; return rc; }
  *out = loc;
  return BWTM_OK;
}

extern "C" void bwtm_locator_free(bwtm_locator* locator)
{
  if(!locator) { return; }
  Scope scope(locator->ctx);
  delete locator;                                     // the table returns to the pool (stream ordered)
}

extern "C" uint64_t bwtm_locator_bytes(const bwtm_locator* locator) { return locator ? locator->index->m * sizeof(u64) : 0; }

extern "C" int bwtm_locate_batch(const bwtm_locator* loc, const uint64_t* positions, uint64_t count, uint64_t* out_ids, uint64_t* out_offsets)
{
  if(!loc || (count > 0 && (!positions || !out_ids || !out_offsets))) { return fail(BWTM_EINVAL, "bwtm_locate_batch: null argument"); }
  ENTER(loc->ctx);
  const u64 n = loc->index->n;
  for(u64 k = 0; k < count; k++)
  {
    if(positions[k] >= n) { return fail(BWTM_EINVAL, "bwtm_locate_batch: position %llu out of range (%llu positions)", (unsigned long long)positions[k], (unsigned long long)n); }
  }
  if(count == 0) { return BWTM_OK; }
  const u64 batch = std::min(locate_batch_size(), count);
  LocateBatch b;
  TRY(b.alloc(batch, true));
  for(u64 done = 0; done < count; done += batch)
  {
    const u64 nb = std::min(batch, count - done);
    HIP_TRY(hipMemcpyAsync(b.d_pos.p, positions + done, nb * sizeof(u64), hipMemcpyHostToDevice, CTX.stream));
    u64 bad = 0;
    TRY(b.run(loc, true, 0, nb, out_ids + done, out_offsets + done, &bad));
    if(bad != SEQ_STATUS_NONE)
    {
      return fail(BWTM_EINVAL, "bwtm_locate_batch: position %llu reaches no start of a sequence (the index is damaged)", (unsigned long long)positions[done + bad]);
    }
  }
  return BWTM_OK;
}

// The hits are numbered through all ranges; a batch is `locate_batch` consecutive hits.  The host walks the ranges once and hands every
// batch the ranges that have hits in it -- the start position of the first of its hits and the batch-local number of that hit, at most one
// pair per hit -- and the device turns hit numbers into positions: no position exists on the host.
extern "C" int bwtm_locate_ranges(const bwtm_locator* loc, const uint64_t* sp, const uint64_t* ep, uint64_t count, uint64_t max_hits, uint64_t* hit_offsets,
                                  uint64_t* out_ids, uint64_t* out_offsets, uint64_t capacity)
{
  if(!loc || !hit_offsets || (count > 0 && (!sp || !ep))) { return fail(BWTM_EINVAL, "bwtm_locate_ranges: null argument"); }
  ENTER(loc->ctx);
  const u64 n = loc->index->n;
  auto kept = [&](u64 r) -> u64
  {
    if(sp[r] > ep[r]) { return 0; }
    const u64 all = ep[r] - sp[r] + 1;
    return (max_hits > 0 && all > max_hits ? max_hits : all);
  };
  hit_offsets[0] = 0;
  for(u64 r = 0; r < count; r++)
  {
    if(sp[r] <= ep[r] && ep[r] >= n)
    {
      return fail(BWTM_EINVAL, "bwtm_locate_ranges: range %llu ends at position %llu (%llu positions)", (unsigned long long)r, (unsigned long long)ep[r], (unsigned long long)n);
    }
    hit_offsets[r + 1] = hit_offsets[r] + kept(r);
  }
  const u64 total = hit_offsets[count];
  if(!out_ids || capacity == 0 || total == 0) { return BWTM_OK; }                               // sizes only
  if(!out_offsets) { return fail(BWTM_EINVAL, "bwtm_locate_ranges: null argument"); }
  if(capacity < total) { return fail(BWTM_EINVAL, "bwtm_locate_ranges: capacity %llu is too small (%llu hits)", (unsigned long long)capacity, (unsigned long long)total); }
  const u64 batch = std::min(locate_batch_size(), total);
  LocateBatch b;
  TRY(b.alloc(batch, false));
  std::vector<u64> h_start, h_first;
  h_start.reserve(std::min<u64>(batch, count)); h_first.reserve(std::min<u64>(batch, count));
  u64 r = 0;                                                                                    // the range of the next hit
  for(u64 done = 0; done < total; done += batch)
  {
    const u64 nb = std::min(batch, total - done);
    h_start.clear(); h_first.clear();
    while(r < count && hit_offsets[r] < done + nb)
    {
      const u64 first = std::max(hit_offsets[r], done);
      if(hit_offsets[r + 1] > first)                                                            // it has hits in this batch
      {
        h_start.push_back(sp[r] + (first - hit_offsets[r])); h_first.push_back(first - done);
      }
      if(hit_offsets[r + 1] > done + nb) { break; }                                             // the next batch goes on inside this range
      r++;
    }
    HIP_TRY(hipMemcpyAsync(b.d_start.p, h_start.data(), h_start.size() * sizeof(u64), hipMemcpyHostToDevice, CTX.stream));
    HIP_TRY(hipMemcpyAsync(b.d_first.p, h_first.data(), h_first.size() * sizeof(u64), hipMemcpyHostToDevice, CTX.stream));
    u64 bad = 0;
    TRY(b.run(loc, false, h_start.size(), nb, out_ids + done, out_offsets + done, &bad));      // synchronises: the host vectors are free again
    if(bad != SEQ_STATUS_NONE)
    {
      return fail(BWTM_EINVAL, "bwtm_locate_ranges: hit %llu reaches no start of a sequence (the index is damaged)", (unsigned long long)(done + bad));
    }
  }
  return BWTM_OK;
}
