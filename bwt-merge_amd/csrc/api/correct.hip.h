/*
  api/correct.hip.h -- k-mer error correction of reads (bwtm_corrector_*, bwtm_correct_batch, bwtm_correct_sequences): the solid k-mers of
  a spectrum as a sorted table with a bucket directory, and one wave per read that substitutes a symbol per round (kernels/correct.hip.h).
  Part of bwtm_api.hip.

  The handle, with S = the k-mers of count >= threshold and D = min(2 k, 24, max(1, ceil(log2 S))):

      bytes = 8 max(S, 1) + 8 (2^D + 1), each of the two blocks rounded up by the pool

  bwtm_corrector_create needs 8 (n + 1) bytes more while it runs, n = the k-mers of the k-mer handle: the flags whose scan gives every
  solid code its slot (and the partial sums of that scan, 8 bytes per 2048 flags).

  Device memory of a correct call beyond the table (and the index), per batch of B = bwtm_tune("correct_batch") reads with T bytes of text:

      peak <= 17/8 T + 27 (B + 1) + 2^16 bytes                          (every block below 512 MiB)

      T  the batch's input text: uploaded (bwtm_correct_batch) or extracted (bwtm_correct_sequences, the stage of bwtm_sequences_extract).
      T  the working copy the kernel corrects; a FAILED read is restored from the input text.
    8 (B + 1)  the batch-local offsets.
    5 B  one byte of status and four of edits per read.
   12 B  bwtm_correct_sequences only: the ids of the batch (when ids are given) and the 32-bit lengths of the extract stage.
         Then 8 bytes per 2048 reads for the partial sums of the offsets' scan, and three small cells (statistics, the extract stage's status).
  1/8 T + 2 (B + 1) + 2^16  what the pool rounds up: a block of 1 MiB or more to 64 KiB, of 64 MiB or more to 2 MiB (a sixteenth of the
         block at the most), a smaller one to 256 bytes, nine blocks.
  A block of 512 MiB or more is made of whole chunks of 1 GiB (api/context.hip.h): at that size add one chunk per block.
  bwtm_correct_sequences first takes the lengths of every batch into offsets of its own (8 (count + 1) bytes of host memory), so that max_len
  and the capacity are checked before anything is written: the caller's offsets, text, status and edit counts are untouched by a refused
  call.  A call of one batch keeps those lengths, a call of several walks every batch a second time.  Its second round runs whether or not
  text is wanted, so it is not a two_round_call.  Batches: see api/batches.hip.h.
*/
#pragma once

struct bwtm_corrector
{
  bwtm_context* ctx = nullptr;
  bwtm_corrector() : ctx(t_ctx) { if(ctx) { ctx->live_handles++; } }
  ~bwtm_corrector() { if(ctx) { ctx->live_handles--; } }
  bwtm_corrector(const bwtm_corrector&) = delete; bwtm_corrector& operator=(const bwtm_corrector&) = delete;
  DevBuf codes;                       // the solid codes, ascending
  DevBuf dir;                         // 2^dir_bits + 1 first entries of the buckets
  u64 solid = 0, threshold = 0;
  u32 k = 0, skip = 0, dir_bits = 0;
  CorrectTable table() const { return CorrectTable{codes.as<const u64>(), dir.as<const u64>(), solid, k, skip, dir_bits}; }
};

namespace
{
// What the last correct call of this thread did: table lookups, rounds run over all reads, the most edits in one read, batches.
thread_local CallStats t_correct_stats;

constexpr u64 CORRECT_MAX_ROUNDS = 65535;
constexpr u64 CORRECT_LAUNCH_READS = 1ull << 25;        // a wave per read: 2^31 threads per launch

u64 correct_batch_size() { return std::min<u64>((u64)g_tune.correct_batch, WALK_BATCH_LIMIT); }

int corrector_build(bwtm_corrector* c, const bwtm_kmers* km, u32 skip, u64 threshold)
{
  const u64 n = km->distinct;
  c->k = km->k; c->skip = skip; c->threshold = threshold;
  auto alloc_codes = [&]() -> int { return c->codes.alloc(std::max<u64>(c->solid, 1) * sizeof(u64)); };   // 8 max(S, 1), as stated above
  if(n > 0)
  {
    DevBuf flags;
    TRY(flags.alloc((n + 1) * sizeof(u64)));
    LAUNCH("correct_flag", k_correct_flag, div_up(n + 1, BLOCK_THREADS), BLOCK_THREADS, km->cnt(), n, threshold, flags.as<u64>());
    TRY(device_scan<0>(flags.as<const u64>(), flags.as<u64>(), n + 1));
    TRY(fetch_u64(flags.as<u64>() + n, 0));
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    c->solid = CTX.host_scratch[0];
    if(c->solid > n) { return fail(BWTM_EINVAL, "bwtm_corrector_create: %llu of %llu k-mers counted as solid", (unsigned long long)c->solid, (unsigned long long)n); }
    TRY(alloc_codes());
    if(c->solid > 0)
    {
      LAUNCH("correct_compact", k_correct_compact, div_up(n, BLOCK_THREADS), BLOCK_THREADS, km->code(), km->cnt(), flags.as<const u64>(), n, threshold, c->codes.as<u64>(), c->solid);
    }
  }
  else { TRY(alloc_codes()); }
  c->dir_bits = correct_dir_bits(c->k, c->solid);
  const u64 buckets = 1ull << c->dir_bits;
  TRY(c->dir.alloc((buckets + 1) * sizeof(u64)));
  LAUNCH("correct_dir", k_correct_dir, div_up(c->solid + 1, BLOCK_THREADS), BLOCK_THREADS, c->codes.as<const u64>(), c->solid, 2 * c->k - c->dir_bits, buckets, c->dir.as<u64>());
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  return BWTM_OK;
}

// The buffers of one batch behind its text and offsets, and the launch: the working copy, status and edits, brought to the caller.
struct CorrectBatch
{
  const bwtm_corrector* c = nullptr;
  u32 max_rounds = 0;
  DevBuf d_work, d_status, d_edits, d_stats;
  int alloc(u64 batch)
  {
    TRY(d_status.alloc(batch)); TRY(d_edits.alloc(batch * sizeof(u32))); TRY(d_stats.alloc(4 * sizeof(u64), true));
    return BWTM_OK;
  }
  // nb reads whose input text (bytes of it) and nb + 1 batch-local offsets are on the device; any of the three outputs may be null
  int run(const u8* d_text, const u64* d_off, u64 nb, u64 bytes, u8* out_text, u8* out_status, u32* out_edits)
  {
    TRY(d_work.alloc(bytes));
#ifdef BWTM_DIAGNOSTICS
    if(g_tune.correct_kernel == 1)                                                              // the A/B partner: one lane per read
    {
      LAUNCH("correct", k_correct_lane, div_up(nb, BLOCK_THREADS), BLOCK_THREADS, c->table(), d_text, d_work.as<u8>(), d_off, nb, max_rounds, d_status.as<u8>(),
        d_edits.as<u32>(), d_stats.as<unsigned long long>());
    }
    else
#endif
    for(u64 first = 0; first < nb; first += CORRECT_LAUNCH_READS)
    {
      const u64 part = std::min(CORRECT_LAUNCH_READS, nb - first);
      LAUNCH("correct", k_correct_wave, div_up(part, CORRECT_WAVES), BLOCK_THREADS, c->table(), d_text, d_work.as<u8>(), d_off + first, part, max_rounds,
        d_status.as<u8>() + first, d_edits.as<u32>() + first, d_stats.as<unsigned long long>());
    }
    TRY(to_host(out_text, d_work.as<const u8>(), bytes)); TRY(to_host(out_status, d_status.as<const u8>(), nb)); TRY(to_host(out_edits, d_edits.as<const u32>(), nb));
    HIP_TRY(hipStreamSynchronize(CTX.stream));                                                  // the batch's buffers, and a staged batch's h_off, are reused
    t_correct_stats[3]++;
    return BWTM_OK;
  }
  int finish()
  {
    TRY(fetch_u64(d_stats.as<u64>(), 0, 3));
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    for(u32 j = 0; j < 3; j++) { t_correct_stats[j] = CTX.host_scratch[j]; }
    return BWTM_OK;
  }
};

} // namespace

extern "C" int bwtm_corrector_create(const bwtm_kmers* kmers, uint32_t skip, uint64_t threshold, bwtm_corrector** out)
{
  if(!kmers || !out) { return fail(BWTM_EINVAL, "bwtm_corrector_create: null argument"); }
  ENTER(kmers->ctx);
  if(skip < 1 || skip > 5) { return fail(BWTM_EINVAL, "bwtm_corrector_create: skip = %u is no comp value 1..5", (unsigned)skip); }
  if(kmers->k == 0 || kmers->k > KMER_MAX_K) { return fail(BWTM_EINVAL, "bwtm_corrector_create: the k-mer handle has k = %u", (unsigned)kmers->k); }
  if(threshold == 0) { threshold = 1; }
  bwtm_corrector* c = new bwtm_corrector();
  const int rc = corrector_build(c, kmers, skip, threshold);
  if(rc != BWTM_OK) { (void)hipStreamSynchronize(CTX.stream); delete c; return rc; }
  *out = c;
  return BWTM_OK;
}

extern "C" void bwtm_corrector_free(bwtm_corrector* corrector)
{
  if(!corrector) { return; }
  Scope scope(corrector->ctx);
  delete corrector;                                   // the table returns to the pool (stream ordered)
}

extern "C" uint64_t bwtm_corrector_solid(const bwtm_corrector* corrector) { return corrector ? corrector->solid : 0; }
extern "C" uint64_t bwtm_corrector_bytes(const bwtm_corrector* corrector) { return corrector ? corrector->codes.bytes + corrector->dir.bytes : 0; }
extern "C" uint32_t bwtm_corrector_k(const bwtm_corrector* corrector) { return corrector ? corrector->k : 0; }

extern "C" int bwtm_correct_stats(uint64_t stats[4]) { return t_correct_stats.get("bwtm_correct_stats", stats); }

extern "C" int bwtm_correct_batch(const bwtm_corrector* corrector, const uint8_t* patterns, const uint64_t* offsets, uint64_t count, uint32_t max_rounds,
                                  uint8_t* out_text, uint8_t* out_status, uint32_t* out_edits)
{
  if(!corrector || (count > 0 && !offsets)) { return fail(BWTM_EINVAL, "bwtm_correct_batch: null argument"); }
  ENTER(corrector->ctx);
  if(max_rounds > CORRECT_MAX_ROUNDS) { return fail(BWTM_EINVAL, "bwtm_correct_batch: max_rounds = %u is above 65535", (unsigned)max_rounds); }
  t_correct_stats.reset();
  if(count == 0) { return BWTM_OK; }
  TRY(validate_texts("bwtm_correct_batch", "pattern", patterns, offsets, count, 0));
  const u64 batch = std::min(correct_batch_size(), count);
  CorrectBatch b;
  b.c = corrector; b.max_rounds = max_rounds;
  TRY(b.alloc(batch));
  StagedTexts t;
  for(u64 done = 0; done < count; done += batch)
  {
    const u64 nb = std::min(batch, count - done);
    TRY(t.stage(patterns, offsets + done, nb));
    TRY(b.run(t.d_text.as<const u8>(), t.d_off.as<const u64>(), nb, t.bytes, at_or_null(out_text, offsets[done]), at_or_null(out_status, done), at_or_null(out_edits, done)));
  }
  return b.finish();
}

// The reads are extracted on the device, batch by batch (the stage of bwtm_sequences_extract), corrected there and brought to the caller.
extern "C" int bwtm_correct_sequences(const bwtm_corrector* corrector, const bwtm_index* x, const uint64_t* ids, uint64_t first_id, uint64_t count,
                                      uint64_t max_len, uint32_t max_rounds, uint64_t* offsets, uint8_t* text, uint64_t capacity,
                                      uint8_t* out_status, uint32_t* out_edits)
{
  const char* const who = "bwtm_correct_sequences";
  if(!corrector || !x) { return fail(BWTM_EINVAL, "bwtm_correct_sequences: null argument"); }
  WHOLE_INDEX(x, "bwtm_correct_sequences");
  if(corrector->ctx != x->ctx) { return fail(BWTM_EINVAL, "bwtm_correct_sequences: the corrector and the index belong to different contexts"); }
  ENTER(corrector->ctx);
  if(max_rounds > CORRECT_MAX_ROUNDS) { return fail(BWTM_EINVAL, "bwtm_correct_sequences: max_rounds = %u is above 65535", (unsigned)max_rounds); }
  TRY(check_max_len(who, &max_len));
  t_correct_stats.reset();
  if(count == 0) { if(offsets) { offsets[0] = 0; } return BWTM_OK; }
  TRY(check_sequence_ids(who, x, ids, first_id, count));
  std::vector<u64> own(count + 1, 0);                                                           // the caller's offsets are written after the last check
  u64* const out_offsets = offsets;
  offsets = own.data();
  const u64 batch = std::min(correct_batch_size(), count);
  const bool single = (batch >= count);
  SeqBatch s;
  TRY(s.alloc(batch, ids != nullptr, true, false));                                             // lengths and offsets stay on the device
  std::vector<u64> h_off(batch + 1, 0);
  // lengths -> batch-local offsets in s.d_off; fill: they continue the caller's offsets behind offsets[done]
  auto sizes = [&](u64 done, u64 nb, bool fill) -> int
  {
    TRY(s.offsets_on_device(who, "max_len", x, at_or_null(ids, done), first_id + done, nb, max_len));
    if(!fill) { return BWTM_OK; }
    TRY(to_host(h_off.data(), s.d_off.as<const u64>(), nb + 1));
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    for(u64 k = 1; k <= nb; k++) { offsets[done + k] = offsets[done] + h_off[k]; }
    return BWTM_OK;
  };
  for(u64 done = 0; done < count; done += batch) { TRY(sizes(done, std::min(batch, count - done), true)); }
  const u64 total = offsets[count];
  const bool want_text = (text && capacity > 0);
  if(want_text && capacity < total) { return fail(BWTM_EINVAL, "bwtm_correct_sequences: capacity %llu is too small (%llu bytes of text)", (unsigned long long)capacity, (unsigned long long)total); }
  if(out_offsets) { std::copy(own.begin(), own.end(), out_offsets); }
  CorrectBatch b;
  b.c = corrector; b.max_rounds = max_rounds;
  TRY(b.alloc(batch));
  for(u64 done = 0; done < count; done += batch)
  {
    const u64 nb = std::min(batch, count - done);
    if(!single) { TRY(sizes(done, nb, false)); }
    const u64 local = offsets[done + nb] - offsets[done];
    TRY(s.emit(x, at_or_null(ids, done), first_id + done, nb, local));                          // the text at its exact size
    TRY(b.run(s.d_text.as<const u8>(), s.d_off.as<const u64>(), nb, local, (want_text ? text + offsets[done] : nullptr), at_or_null(out_status, done), at_or_null(out_edits, done)));
  }
  return b.finish();
}
