/*
  api/sequences.hip.h -- sequences of the collection by id (bwtm_sequences_extract): lengths, offsets and text, batch by batch.
  Part of bwtm_api.hip.
*/
#pragma once

namespace
{
// What the per-chain queries share on the host (this file, api/locate.hip.h, api/overlap.hip.h; their kernels: kernels/quad.hip.h).

constexpr u64 SEQ_MAX_LEN_DEFAULT = 1ull << 16, SEQ_MAX_LEN_LIMIT = 1ull << 24;
// four lanes per sequence, walk or query and fewer than 2^32 threads per grid (the note at LAUNCH_CFG): a batch is one launch
constexpr u64 WALK_BATCH_LIMIT = 1ull << 28;

// The status word of a launch: its kernel lowers it (atomicMin) to the first slot of the batch that failed.  arm() fills it with 0xFF
// bytes, which is SEQ_STATUS_NONE; read() queues its copy into slot 0 of the host scratch behind whatever the caller has queued since the
// launch, awaits the stream and hands the word out.
struct StatusCell
{
  static_assert(SEQ_STATUS_NONE == 0xFFFFFFFFFFFFFFFFull, "arm() fills the word with 0xFF bytes");
  DevBuf d;
  int alloc() { return d.alloc(sizeof(u64)); }
  unsigned long long* word() const { return d.as<unsigned long long>(); }
  int arm()
  {
    HIP_TRY(hipMemsetAsync(d.p, 0xFF, sizeof(u64), CTX.stream));
    return BWTM_OK;
  }
  int read(u64* first_bad)
  {
    TRY(fetch_u64(d.as<u64>(), 0));
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    *first_bad = CTX.host_scratch[0];
    return BWTM_OK;
  }
};

// max_len of a call: 0 stands for the default, and no walk is allowed more than 2^24 steps.
int check_max_len(const char* who, u64* max_len)
{
  if(*max_len == 0) { *max_len = SEQ_MAX_LEN_DEFAULT; }
  if(*max_len > SEQ_MAX_LEN_LIMIT) { return fail(BWTM_EINVAL, "%s: max_len %llu is above 2^24", who, (unsigned long long)*max_len); }
  return BWTM_OK;
}

// The sequences of a call, count >= 1 of them: ids[0 .. count), or first_id .. first_id + count - 1 (ids == nullptr), are all below m.
int check_sequence_ids(const char* who, const bwtm_index* x, const u64* ids, u64 first_id, u64 count)
{
  if(!ids)
  {
    if(first_id >= x->m || count > x->m - first_id)
    {
      return fail(BWTM_EINVAL, "%s: sequence %llu out of range (%llu sequences)", who, (unsigned long long)std::max<u64>(first_id, x->m), (unsigned long long)x->m);
    }
    return BWTM_OK;
  }
  for(u64 k = 0; k < count; k++)
  {
    if(ids[k] >= x->m) { return fail(BWTM_EINVAL, "%s: sequence %llu out of range (%llu sequences)", who, (unsigned long long)ids[k], (unsigned long long)x->m); }
  }
  return BWTM_OK;
}

// The per-batch stage of reading sequences by id, shared by bwtm_sequences_extract (which brings the text to the host),
// bwtm_overlap_sequences and bwtm_correct_sequences (which work on it where it is): the device buffers of one batch and its two launches.
struct SeqBatch
{
  DevBuf d_ids, d_len, d_off, d_text;
  StatusCell status;
  std::vector<u32> h_len;               // the batch's lengths, after lengths()
  std::vector<u64> h_off;               // batch-local offsets (nb + 1 entries), filled by the caller between lengths() and emit()
  bool on_host = true;                  // false: the lengths stay in d_len, and the caller leaves the nb + 1 offsets in d_off before emit()
  int alloc(u64 batch, bool with_ids, bool with_text, bool host_side = true)
  {
    on_host = host_side;
    if(with_ids) { TRY(d_ids.alloc(batch * sizeof(u64))); }
    TRY(d_len.alloc(batch * sizeof(u32))); TRY(status.alloc());
    if(with_text) { TRY(d_off.alloc((batch + 1) * sizeof(u64))); }
    h_len.assign(on_host ? batch : 0, 0);
    h_off.assign(on_host && with_text ? batch + 1 : 0, 0);
    return BWTM_OK;
  }
  const u64* ids_or_null(const u64* ids) const { return (ids ? d_ids.as<const u64>() : (const u64*)nullptr); }
  // ids up (when given), k_seq_lengths, lengths down into h_len (on_host); *bad = the first sequence of the batch that failed, or SEQ_STATUS_NONE
  int lengths(const bwtm_index* x, const u64* ids, u64 first_id, u64 nb, u64 max_len, u64* bad)
  {
    if(ids) { HIP_TRY(hipMemcpyAsync(d_ids.p, ids, nb * sizeof(u64), hipMemcpyHostToDevice, CTX.stream)); }
    TRY(status.arm());
    LAUNCH("seq_lengths", k_seq_lengths, div_up(4 * nb, BLOCK_THREADS), BLOCK_THREADS, x->view(), ids_or_null(ids), first_id, nb, (u32)max_len,
      d_len.as<u32>(), status.word());
    if(on_host) { HIP_TRY(hipMemcpyAsync(h_len.data(), d_len.p, nb * sizeof(u32), hipMemcpyDeviceToHost, CTX.stream)); }
    return status.read(bad);
  }
  // For a batch whose lengths stay on the device (!on_host): lengths(), refused in the name of `who` if a sequence is longer than max_len
  // (`limit` is what the message calls it), then the nb + 1 batch-local offsets into d_off: the lengths widened and scanned.  ids and
  // first_id are those of the batch's first sequence.
  int offsets_on_device(const char* who, const char* limit, const bwtm_index* x, const u64* ids, u64 first_id, u64 nb, u64 max_len)
  {
    u64 bad = 0;
    TRY(lengths(x, ids, first_id, nb, max_len, &bad));
    if(bad != SEQ_STATUS_NONE)
    {
      return fail(BWTM_EINVAL, "%s: sequence %llu is longer than %s = %llu (or the index is damaged)", who, (unsigned long long)(ids ? ids[bad] : first_id + bad), limit,
        (unsigned long long)max_len);
    }
    LAUNCH("overlap_widen", k_overlap_widen, div_up(nb + 1, BLOCK_THREADS), BLOCK_THREADS, d_len.as<const u32>(), nb, d_off.as<u64>());
    return device_scan<0>(d_off.as<const u64>(), d_off.as<u64>(), nb + 1);
  }
  // the batch's text allocated at its exact size `local`, h_off up (on_host), k_seq_emit (not launched for an empty text); nothing is awaited
  int emit(const bwtm_index* x, const u64* ids, u64 first_id, u64 nb, u64 local)
  {
    TRY(d_text.alloc(local));
    if(on_host) { HIP_TRY(hipMemcpyAsync(d_off.p, h_off.data(), (nb + 1) * sizeof(u64), hipMemcpyHostToDevice, CTX.stream)); }
    if(local == 0) { return BWTM_OK; }
    LAUNCH("seq_emit", k_seq_emit, div_up(4 * nb, BLOCK_THREADS), BLOCK_THREADS, x->view(), ids_or_null(ids), first_id, nb, d_off.as<const u64>(),
      d_len.as<const u32>(), d_text.as<u8>());
    return BWTM_OK;
  }
};
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
  TRY(check_max_len("bwtm_sequences_extract", &max_len));
  offsets[0] = 0;
  if(count == 0) { return BWTM_OK; }
  TRY(check_sequence_ids("bwtm_sequences_extract", x, ids, first_id, count));
  const bool sizes_only = (!text || capacity == 0);
  const u64 batch = std::min<u64>(std::min<u64>((u64)g_tune.extract_batch, WALK_BATCH_LIMIT), count);
  SeqBatch b;
  TRY(b.alloc(batch, ids != nullptr, !sizes_only));
  u64 running = 0;
  for(u64 done = 0; done < count; done += batch)
  {
    const u64 nb = std::min(batch, count - done);
    u64 bad = 0;
    TRY(b.lengths(x, (ids ? ids + done : nullptr), first_id + done, nb, max_len, &bad));
    if(bad != SEQ_STATUS_NONE)
    {
      bad += done;
      return fail(BWTM_EINVAL, "bwtm_sequences_extract: sequence %llu is longer than max_len = %llu (or the index is damaged)",
        (unsigned long long)(ids ? ids[bad] : first_id + bad), (unsigned long long)max_len);
    }
    u64 local = 0;
    for(u64 k = 0; k < nb; k++)
    {
      if(!sizes_only) { b.h_off[k] = local; }
      local += b.h_len[k];
      offsets[done + k + 1] = running + local;
    }
    if(!sizes_only && local > 0)
    {
      if(running + local > capacity)
      {
        return fail(BWTM_EINVAL, "bwtm_sequences_extract: capacity %llu is too small (the first %llu sequences take %llu bytes)", (unsigned long long)capacity,
          (unsigned long long)(done + nb), (unsigned long long)(running + local));
      }
      b.h_off[nb] = local;
      TRY(b.emit(x, (ids ? ids + done : nullptr), first_id + done, nb, local));
      HIP_TRY(hipMemcpyAsync(text + running, b.d_text.p, local, hipMemcpyDeviceToHost, CTX.stream));
      HIP_TRY(hipStreamSynchronize(CTX.stream));                                              // the batch's buffers are reused
    }
    running += local;
  }
  return BWTM_OK;
}
