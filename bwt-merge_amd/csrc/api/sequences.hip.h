/*
  api/sequences.hip.h -- sequences of the collection by id (bwtm_sequences_extract): lengths, offsets and text, batch by batch.
  Part of bwtm_api.hip.
*/
#pragma once

namespace
{
constexpr u64 SEQ_MAX_LEN_DEFAULT = 1ull << 16, SEQ_MAX_LEN_LIMIT = 1ull << 24;
// four lanes per sequence and fewer than 2^32 threads per grid (the note at LAUNCH_CFG): a batch is one launch
constexpr u64 SEQ_BATCH_LIMIT = 1ull << 28;
} // namespace

// Every batch of at most extract_batch sequences: ids up (when given), k_seq_lengths, lengths down, prefix sums on the host into the
// caller's offsets, the batch's text allocated at its exact size, batch-local offsets up, k_seq_emit, text down at the running offset.
// The device buffers of the call are those of one batch, whatever the collection holds.
extern "C" int bwtm_sequences_extract(const bwtm_index* x, const uint64_t* ids, uint64_t first_id, uint64_t count, uint64_t max_len,
                                      uint64_t* offsets, uint8_t* text, uint64_t capacity)
{
  if(!x || !offsets) { return fail(BWTM_EINVAL, "bwtm_sequences_extract: null argument"); }
  WHOLE_INDEX(x, "bwtm_sequences_extract");
  ENTER(x->ctx);
  if(max_len == 0) { max_len = SEQ_MAX_LEN_DEFAULT; }
  if(max_len > SEQ_MAX_LEN_LIMIT) { return fail(BWTM_EINVAL, "bwtm_sequences_extract: max_len %llu is above 2^24", (unsigned long long)max_len); }
  offsets[0] = 0;
  if(count == 0) { return BWTM_OK; }
  if(!ids)
  {
    if(first_id >= x->m || count > x->m - first_id)
    {
      return fail(BWTM_EINVAL, "bwtm_sequences_extract: sequence %llu out of range (%llu sequences)", (unsigned long long)std::max<u64>(first_id, x->m), (unsigned long long)x->m);
    }
  }
  else
  {
    for(u64 k = 0; k < count; k++)
    {
      if(ids[k] >= x->m) { return fail(BWTM_EINVAL, "bwtm_sequences_extract: sequence %llu out of range (%llu sequences)", (unsigned long long)ids[k], (unsigned long long)x->m); }
    }
  }
  const bool sizes_only = (!text || capacity == 0);
  const u64 batch = std::min<u64>(std::min<u64>((u64)g_tune.extract_batch, SEQ_BATCH_LIMIT), count);
  DevBuf d_ids, d_len, d_off, d_status, d_text;
  if(ids) { TRY(d_ids.alloc(batch * sizeof(u64))); }
  TRY(d_len.alloc(batch * sizeof(u32))); TRY(d_status.alloc(sizeof(u64)));
  if(!sizes_only) { TRY(d_off.alloc(batch * sizeof(u64))); }
  std::vector<u32> h_len(batch);
  std::vector<u64> h_off(sizes_only ? 0 : batch);
  u64 running = 0;
  for(u64 done = 0; done < count; done += batch)
  {
    const u64 nb = std::min(batch, count - done);
    const u64 grid = div_up(4 * nb, BLOCK_THREADS);
    if(ids) { HIP_TRY(hipMemcpyAsync(d_ids.p, ids + done, nb * sizeof(u64), hipMemcpyHostToDevice, CTX.stream)); }
    HIP_TRY(hipMemsetAsync(d_status.p, 0xFF, sizeof(u64), CTX.stream));                       // SEQ_STATUS_NONE
    LAUNCH("seq_lengths", k_seq_lengths, grid, BLOCK_THREADS, x->view(), (ids ? d_ids.as<const u64>() : (const u64*)nullptr), first_id + done, nb, (u32)max_len,
      d_len.as<u32>(), d_status.as<unsigned long long>());
    HIP_TRY(hipMemcpyAsync(h_len.data(), d_len.p, nb * sizeof(u32), hipMemcpyDeviceToHost, CTX.stream));
    TRY(fetch_u64(d_status.as<u64>(), 0));
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    if(CTX.host_scratch[0] != SEQ_STATUS_NONE)
    {
      const u64 bad = done + CTX.host_scratch[0];
      return fail(BWTM_EINVAL, "bwtm_sequences_extract: sequence %llu is longer than max_len = %llu (or the index is damaged)",
        (unsigned long long)(ids ? ids[bad] : first_id + bad), (unsigned long long)max_len);
    }
    u64 local = 0;
    for(u64 k = 0; k < nb; k++)
    {
      if(!sizes_only) { h_off[k] = local; }
      local += h_len[k];
      offsets[done + k + 1] = running + local;
    }
    if(!sizes_only && local > 0)
    {
      if(running + local > capacity)
      {
        return fail(BWTM_EINVAL, "bwtm_sequences_extract: capacity %llu is too small (the first %llu sequences take %llu bytes)", (unsigned long long)capacity,
          (unsigned long long)(done + nb), (unsigned long long)(running + local));
      }
      TRY(d_text.alloc(local));
      HIP_TRY(hipMemcpyAsync(d_off.p, h_off.data(), nb * sizeof(u64), hipMemcpyHostToDevice, CTX.stream));
      LAUNCH("seq_emit", k_seq_emit, grid, BLOCK_THREADS, x->view(), (ids ? d_ids.as<const u64>() : (const u64*)nullptr), first_id + done, nb, d_off.as<const u64>(),
        d_len.as<const u32>(), d_text.as<u8>());
      HIP_TRY(hipMemcpyAsync(text + running, d_text.p, local, hipMemcpyDeviceToHost, CTX.stream));
      HIP_TRY(hipStreamSynchronize(CTX.stream));                                              // the batch's buffers are reused
    }
    running += local;
  }
  return BWTM_OK;
}
