/*
  api/mem.hip.h -- matching statistics and maximal exact matches of a batch of patterns (bwtm_matching_stats_batch, bwtm_mem_batch): one
  backward search per symbol of the text for the statistics; for the MEMs one quad per pattern that searches its ends downwards and
  flags those that give a MEM, two scans, one emit (kernels/mem.hip.h).  Part of bwtm_api.hip.

  Device memory of a call beyond the index, per batch of B = bwtm_tune("mem_batch") patterns, with T = the symbols of the batch's text
  (a batch also ends before T reaches 2^29: one launch holds its 4 T lanes) and M = its MEMs of at least min_length symbols (M <= T):

      bwtm_matching_stats_batch   peak <= 21 T +  8 B + 2^24 bytes
      bwtm_mem_batch              peak <= 29 T + 28 M + 16 B + 2^25 bytes

        T  the text.
      8 B  the batch-local offsets, B + 1 of them.
     20 T  the matching statistics: length (4), sp (8), count (8) per symbol; bwtm_matching_stats_batch leaves out an array the caller
           does not ask for, and bwtm_mem_batch fills in the entries of the ends that give a MEM only.
      8 T  bwtm_mem_batch: the flags of the ends, scanned in place into the MEMs' slots (T + 1 words; the scan adds 8 bytes per 2048).
      8 B  bwtm_mem_batch: the MEMs per pattern, scanned in place into the batch's hit offsets.
     28 M  bwtm_mem_batch, filling call: begin (4), length (4), sp (8), count (8) per MEM before they travel.
     2^24 / 2^25  what the pool rounds up: a block of 1 MiB or more to 64 KiB, of 64 MiB or more to 2 MiB, a smaller one to 256 bytes.
  A block of 512 MiB or more is made of whole chunks of 1 GiB (api/context.hip.h): at that size add one chunk per block.

  Batches: see api/batches.hip.h.
*/
#pragma once

namespace
{
// What the last call of this thread (either of the two) did: LF steps taken (rank pairs), tasks run (symbols for the statistics, patterns
// for the MEMs), MEMs before min_length, batches.
thread_local CallStats t_mem_stats;

// A batch of the statistics is one launch of four lanes per symbol, and a grid holds fewer than 2^32 threads: a batch (of either call)
// also ends before its text reaches 2^29 symbols (a pattern has fewer than 2^16, so every batch holds a pattern).
constexpr u64 MEM_BATCH_SYMBOLS = 1ull << 29;

// The patterns of the batch that starts at pattern `done`: at most bwtm_tune("mem_batch") of them, cut at a pattern boundary.
u64 mem_batch_patterns(const u64* offsets, u64 done, u64 count)
{
  const u64 most = std::min(std::min<u64>((u64)g_tune.mem_batch, WALK_BATCH_LIMIT), count - done);
  if(offsets[done + most] - offsets[done] <= MEM_BATCH_SYMBOLS) { return most; }
  const u64* cut = std::upper_bound(offsets + done, offsets + done + most + 1, offsets[done] + MEM_BATCH_SYMBOLS);
  return std::max<u64>((u64)(cut - (offsets + done)) - 1, 1);
}

// One batch of patterns: its staged text and offsets, the matching statistics, and for the MEMs the flags, slots and hit offsets.
struct MemBatch : StagedTexts
{
  const bwtm_index* x = nullptr;
  u32 min_length = 1;
  DevBuf d_len, d_sp, d_cnt, d_flags, d_per, d_counters, d_out;
  u64 kept_total = 0;                                   // of the staged batch: its MEMs kept

  // The patterns of offsets[0 .. nb] to the device, and the two zeroed counters (steps, MEMs of any length).
  int stage(const u8* patterns, const u64* offsets, u64 nb)
  {
    TRY(d_counters.alloc(2 * sizeof(u64), true));                                               // zeroed on the stream before the copies, as it always was
    return StagedTexts::stage(patterns, offsets, nb);
  }
  unsigned long long* counter(u32 j) const { return d_counters.as<unsigned long long>() + j; }

  // The matching statistics of the staged batch into the arrays asked for.
  int stats_scan(u64 nb, bool want_len, bool want_sp, bool want_cnt)
  {
    if(want_len) { TRY(d_len.alloc(bytes * sizeof(u32))); }
    if(want_sp) { TRY(d_sp.alloc(bytes * sizeof(u64))); }
    if(want_cnt) { TRY(d_cnt.alloc(bytes * sizeof(u64))); }
    LAUNCH("ms_scan", k_ms_scan, div_up(4 * bytes, BLOCK_THREADS), BLOCK_THREADS, x->view(), d_text.as<const u8>(), d_off.as<const u64>(), nb, bytes,
      (want_len ? d_len.as<u32>() : nullptr), (want_sp ? d_sp.as<u64>() : nullptr), (want_cnt ? d_cnt.as<u64>() : nullptr), counter(0));
    return BWTM_OK;
  }

  // The patterns first .. first + nb - 1 of a bwtm_mem_batch call; hit_offsets[0 .. nb] continue hit_offsets[0] by the MEMs kept.
  int search(const char* who, const u8* patterns, const u64* offsets, u64 nb, u64* hit_offsets)
  {
    const u64 before = hit_offsets[0];
    TRY(stage(patterns, offsets, nb));
    kept_total = 0;
    t_mem_stats[3]++;
    if(bytes == 0)
    {
      HIP_TRY(hipStreamSynchronize(CTX.stream));                                                // h_off is reused
      for(u64 k = 1; k <= nb; k++) { hit_offsets[k] = before; }
      return BWTM_OK;
    }
    TRY(d_flags.alloc((bytes + 1) * sizeof(u64)));
    u64 tasks = nb;
#ifdef BWTM_DIAGNOSTICS
    if(g_tune.mem_kernel == 1)                                                                  // the A/B partner: one quad per end, then the rule on the lengths
    {
      TRY(d_per.alloc((nb + 1) * sizeof(u64), true));
      TRY(stats_scan(nb, true, true, true));
      LAUNCH("mem_flag", k_mem_flag, div_up(bytes + 1, BLOCK_THREADS), BLOCK_THREADS, d_len.as<const u32>(), d_off.as<const u64>(), nb, bytes, min_length,
        d_flags.as<u64>(), d_per.as<u64>(), counter(1));
      tasks = bytes;
    }
    else
#endif
    {
      TRY(d_len.alloc(bytes * sizeof(u32))); TRY(d_sp.alloc(bytes * sizeof(u64))); TRY(d_cnt.alloc(bytes * sizeof(u64)));
      TRY(d_per.alloc((nb + 1) * sizeof(u64)));
      LAUNCH("mem_pattern", k_mem_pattern, div_up(4 * nb, BLOCK_THREADS), BLOCK_THREADS, x->view(), d_text.as<const u8>(), d_off.as<const u64>(), nb, bytes, min_length,
        d_len.as<u32>(), d_sp.as<u64>(), d_cnt.as<u64>(), d_flags.as<u64>(), d_per.as<u64>(), counter(0), counter(1));
    }
    TRY(device_scan<0>(d_flags.as<const u64>(), d_flags.as<u64>(), bytes + 1));
    TRY(device_scan<0>(d_per.as<const u64>(), d_per.as<u64>(), nb + 1));
    TRY(fetch_u64(d_flags.as<u64>() + bytes, 0));
    TRY(fetch_u64(d_counters.as<u64>(), 1, 2));
    TRY(to_host(hit_offsets, d_per.as<const u64>(), nb + 1));
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    kept_total = hit_offsets[nb];
    t_mem_stats[0] += CTX.host_scratch[1]; t_mem_stats[1] += tasks; t_mem_stats[2] += CTX.host_scratch[2];
    if(kept_total != CTX.host_scratch[0] || kept_total > bytes)
    {
      return fail(BWTM_EINVAL, "%s: %llu MEMs counted per pattern, %llu flagged, of %llu symbols", who, (unsigned long long)kept_total, (unsigned long long)CTX.host_scratch[0],
        (unsigned long long)bytes);
    }
    if(before != 0) { for(u64 k = 0; k <= nb; k++) { hit_offsets[k] += before; } }              // a later batch of the call
    return BWTM_OK;
  }

  // The MEMs of the batch search() has just seen into the caller's arrays (any of them null), which begin at the batch's first MEM.
  int fill(u64 nb, u32* out_begin, u32* out_length, u64* out_sp, u64* out_count)
  {
    if(kept_total == 0) { return BWTM_OK; }
    TRY(d_out.alloc(28 * kept_total));
    u64* o_sp = d_out.as<u64>(); u64* o_cnt = o_sp + kept_total; u32* o_begin = (u32*)(o_cnt + kept_total); u32* o_len = o_begin + kept_total;
    LAUNCH("mem_emit", k_mem_emit, div_up(bytes, BLOCK_THREADS), BLOCK_THREADS, d_len.as<const u32>(), d_sp.as<const u64>(), d_cnt.as<const u64>(), d_off.as<const u64>(), nb, bytes,
      d_flags.as<const u64>(), kept_total, (out_begin ? o_begin : nullptr), (out_length ? o_len : nullptr), (out_sp ? o_sp : nullptr), (out_count ? o_cnt : nullptr));
    TRY(to_host(out_begin, o_begin, kept_total)); TRY(to_host(out_length, o_len, kept_total)); TRY(to_host(out_sp, o_sp, kept_total)); TRY(to_host(out_count, o_cnt, kept_total));
    HIP_TRY(hipStreamSynchronize(CTX.stream));                                                  // the batch's buffers are reused
    return BWTM_OK;
  }
};

// The batches of a bwtm_mem_batch call in the two rounds of api/batches.hip.h.
int mem_run(const char* who, const bwtm_index* x, const u8* patterns, const u64* offsets, u64 count, u32 min_length, u64* hit_offsets,
            u32* out_begin, u32* out_length, u64* out_sp, u64* out_count, u64 capacity)
{
  MemBatch b;
  b.x = x; b.min_length = min_length;
  return two_round_call(who, "MEMs", count, hit_offsets, out_begin || out_length || out_sp || out_count, capacity, &t_mem_stats,
    [&](u64 done) { return mem_batch_patterns(offsets, done, count); },
    [&](u64 done, u64 nb, u64* batch_offsets) { return b.search(who, patterns, offsets + done, nb, batch_offsets); },
    [&](u64, u64 nb, u64 at) { return b.fill(nb, at_or_null(out_begin, at), at_or_null(out_length, at), at_or_null(out_sp, at), at_or_null(out_count, at)); });
}

// Every batch of a bwtm_matching_stats_batch call: staged, scanned, and the arrays asked for brought to the caller at the batch's first symbol.
int matching_stats_run(const bwtm_index* x, const u8* patterns, const u64* offsets, u64 count, u32* out_lengths, u64* out_sp, u64* out_count)
{
  MemBatch b;
  b.x = x;
  for(u64 done = 0, nb = 0; done < count; done += nb)
  {
    nb = mem_batch_patterns(offsets, done, count);
    const u64 at = offsets[done] - offsets[0];
    TRY(b.stage(patterns, offsets + done, nb));
    t_mem_stats[3]++;
    if(b.bytes > 0)
    {
      TRY(b.stats_scan(nb, out_lengths != nullptr, out_sp != nullptr, out_count != nullptr));
      TRY(fetch_u64(b.d_counters.as<u64>(), 0));
      TRY(to_host(at_or_null(out_lengths, at), b.d_len.as<const u32>(), b.bytes));
      TRY(to_host(at_or_null(out_sp, at), b.d_sp.as<const u64>(), b.bytes));
      TRY(to_host(at_or_null(out_count, at), b.d_cnt.as<const u64>(), b.bytes));
    }
    HIP_TRY(hipStreamSynchronize(CTX.stream));                                                  // the batch's buffers and h_off are reused
    if(b.bytes > 0) { t_mem_stats[0] += CTX.host_scratch[0]; t_mem_stats[1] += b.bytes; }
  }
  return BWTM_OK;
}

} // namespace

extern "C" int bwtm_matching_stats_batch(const bwtm_index* x, const uint8_t* patterns, const uint64_t* offsets, uint64_t count,
                                         uint32_t* out_lengths, uint64_t* out_sp, uint64_t* out_count)
{
  if(!x || (count > 0 && !offsets) || !(out_lengths || out_sp || out_count)) { return fail(BWTM_EINVAL, "bwtm_matching_stats_batch: null argument"); }
  WHOLE_INDEX(x, "bwtm_matching_stats_batch");
  ENTER(x->ctx);
  t_mem_stats.reset();
  if(count == 0) { return BWTM_OK; }
  TRY(validate_texts("bwtm_matching_stats_batch", "pattern", patterns, offsets, count, APPROX_MAX_LEN));
  const int rc = matching_stats_run(x, patterns, offsets, count, out_lengths, out_sp, out_count);
  if(rc != BWTM_OK) { (void)hipStreamSynchronize(CTX.stream); }                                 // the half-built state goes back to the pool behind this
  return rc;
}

extern "C" int bwtm_mem_batch(const bwtm_index* x, const uint8_t* patterns, const uint64_t* offsets, uint64_t count, uint32_t min_length,
                              uint64_t* hit_offsets, uint32_t* out_begin, uint32_t* out_length, uint64_t* out_sp, uint64_t* out_count, uint64_t capacity)
{
  if(!x || !hit_offsets || (count > 0 && !offsets)) { return fail(BWTM_EINVAL, "bwtm_mem_batch: null argument"); }
  WHOLE_INDEX(x, "bwtm_mem_batch");
  ENTER(x->ctx);
  if(min_length == 0) { return fail(BWTM_EINVAL, "bwtm_mem_batch: min_length must be at least 1"); }
  t_mem_stats.reset();
  hit_offsets[0] = 0;
  if(count == 0) { return BWTM_OK; }
  TRY(validate_texts("bwtm_mem_batch", "pattern", patterns, offsets, count, APPROX_MAX_LEN));
  const int rc = mem_run("bwtm_mem_batch", x, patterns, offsets, count, min_length, hit_offsets, out_begin, out_length, out_sp, out_count, capacity);
  if(rc != BWTM_OK) { (void)hipStreamSynchronize(CTX.stream); }                                 // the half-built state goes back to the pool behind this
  return rc;
}

extern "C" int bwtm_mem_stats(uint64_t stats[4]) { return t_mem_stats.get("bwtm_mem_stats", stats); }
