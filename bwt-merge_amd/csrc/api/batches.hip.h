/*
  api/batches.hip.h -- the batch scheme of the calls that take a batch of texts (patterns, queries or reads) from the host, stated once for
  api/overlap.hip.h, api/approx.hip.h, api/edit.hip.h, api/correct.hip.h and api/mem.hip.h: what is checked of the texts, how a batch of
  them reaches the device, the two rounds of a call that sizes before it fills, how optional arrays travel back, and the statistics of a
  call.  Part of bwtm_api.hip.  Nothing here knows of the level scheme (api/frontier.hip.h).

  The first three pieces are plain C++ over fail() and TRY, so that csrc/host/host_cpu_test.cpp runs them without a device; the pieces
  behind them need the context.
*/
#pragma once

namespace
{

// The texts of a call, count >= 1 of them, `noun` what the call's header names them ("pattern", "query").  First every offset, so that no
// text is read through a bad one; then each text's length (max_len == 0: no limit) and its comp values 1..5.
int validate_texts(const char* who, const char* noun, const u8* text, const u64* offsets, u64 count, u64 max_len)
{
  for(u64 k = 0; k < count; k++)
  {
    if(offsets[k] > offsets[k + 1]) { return fail(BWTM_EINVAL, "%s: offsets must not decrease (%s %llu)", who, noun, (unsigned long long)k); }
  }
  if(offsets[count] > offsets[0] && !text) { return fail(BWTM_EINVAL, "%s: null %s text", who, noun); }
  for(u64 k = 0; k < count; k++)
  {
    const u64 len = offsets[k + 1] - offsets[k];
    if(max_len != 0 && len > max_len)
    {
      return fail(BWTM_EINVAL, "%s: %s %llu has %llu symbols (at most %llu)", who, noun, (unsigned long long)k, (unsigned long long)len, (unsigned long long)max_len);
    }
    for(u64 p = offsets[k]; p < offsets[k + 1]; p++)
    {
      if(text[p] < 1 || text[p] > 5)
      {
        return fail(BWTM_EINVAL, "%s: %s %llu holds the symbol %u at offset %llu (comp values 1..5)", who, noun, (unsigned long long)k, (unsigned)text[p],
          (unsigned long long)(p - offsets[k]));
      }
    }
  }
  return BWTM_OK;
}

// What the last call of a family did on this thread: four counters whose meaning the family's file states.
struct CallStats
{
  u64 v[4] = {0, 0, 0, 0};
  u64& operator[](u32 j) { return v[j]; }
  void reset() { for(u32 j = 0; j < 4; j++) { v[j] = 0; } }
  int get(const char* who, u64* out) const
  {
    if(!out) { return fail(BWTM_EINVAL, "%s: null argument", who); }
    for(u32 j = 0; j < 4; j++) { out[j] = v[j]; }
    return BWTM_OK;
  }
};

// A call that sizes before it fills, over the batches batch_at(done) cuts (the patterns done .. done + batch_at(done) - 1).  First
// size(done, nb, hit_offsets + done) runs for every batch: it continues hit_offsets[done] by the batch's counts, so that hit_offsets is
// complete.  Only sizes are wanted if no output array is given (`wanted`), the capacity is 0 or nothing was found.  Otherwise the capacity
// is checked before anything else is written, and fill(done, nb, at) brings every batch's results to slot at = hit_offsets[done] of the
// caller's arrays.  A call whose first batch covers it keeps the batch's state between the two rounds; a call of several batches sizes each
// a second time (the state of all batches does not stay anywhere: the memory is that of one batch), and `stats`, if given, counts that
// work once.  `things` names what the capacity counts ("hits", "MEMs").
template<class BatchAt, class Size, class Fill>
int two_round_call(const char* who, const char* things, u64 count, u64* hit_offsets, bool wanted, u64 capacity, CallStats* stats, BatchAt&& batch_at, Size&& size, Fill&& fill)
{
  const bool single = (batch_at(0) >= count);
  for(u64 done = 0, nb = 0; done < count; done += nb)
  {
    nb = batch_at(done);
    TRY(size(done, nb, hit_offsets + done));
  }
  const u64 total = hit_offsets[count];
  if(!wanted || capacity == 0 || total == 0) { return BWTM_OK; }                                  // sizes only (overlap_run's `size` restates this condition)
  if(capacity < total) { return fail(BWTM_EINVAL, "%s: capacity %llu is too small (%llu %s)", who, (unsigned long long)capacity, (unsigned long long)total, things); }
  const CallStats once = (stats ? *stats : CallStats());
  for(u64 done = 0, nb = 0; done < count; done += nb)
  {
    nb = batch_at(done);
    const u64 at = hit_offsets[done];
    if(!single)
    {
      TRY(size(done, nb, hit_offsets + done));
      if(stats) { *stats = once; }                                                                // the same work a second time
    }
    TRY(fill(done, nb, at));
  }
  return BWTM_OK;
}

template<class T> T* at_or_null(T* p, u64 i) { return (p ? p + i : nullptr); }

#ifdef __HIPCC__

// A batch of texts from the host on the device: the text of offsets[0 .. nb] and its nb + 1 batch-local offsets.
// stage() awaits nothing, and the copy of h_off may still be queued when it returns.  The invariant that makes this safe: every user's
// batch ends in a synchronise of the stream before the next stage() rewrites h_off (PatternBatch::finish_offsets, MemBatch::search and
// the loop of the matching statistics, OverlapBatch::count, CorrectBatch::run).
struct StagedTexts
{
  DevBuf d_text, d_off;
  std::vector<u64> h_off;
  u64 bytes = 0;                                        // of the staged batch: its text
  u64 longest() const                                   // its longest text
  {
    u64 most = 0;
    for(size_t k = 0; k + 1 < h_off.size(); k++) { most = std::max(most, h_off[k + 1] - h_off[k]); }
    return most;
  }

  int stage(const u8* text, const u64* offsets, u64 nb)
  {
    const u64 base = offsets[0];
    bytes = offsets[nb] - base;
    h_off.resize(nb + 1);
    for(u64 k = 0; k <= nb; k++) { h_off[k] = offsets[k] - base; }
    TRY(d_text.alloc(bytes)); TRY(d_off.alloc((nb + 1) * sizeof(u64)));
    if(bytes > 0) { HIP_TRY(hipMemcpyAsync(d_text.p, text + base, bytes, hipMemcpyHostToDevice, CTX.stream)); }
    HIP_TRY(hipMemcpyAsync(d_off.p, h_off.data(), (nb + 1) * sizeof(u64), hipMemcpyHostToDevice, CTX.stream));
    return BWTM_OK;
  }
};

// n entries of a result to an array of the caller's that may be null; queued, not awaited.
template<class T>
int to_host(T* dst, const T* src, u64 n)
{
  if(dst && n > 0) { HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, CTX.stream)); }
  return BWTM_OK;
}

#endif // __HIPCC__

} // namespace
