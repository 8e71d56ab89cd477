/*
  api/upload_stream.hip.h -- the chunked upload: native bytes -> records + super table without the stream ever being resident as a whole
  (BlockArray::clearUntil on the way IN: the reference never holds more of an input than it is consuming).  Part of bwtm_api.hip.

  The stream travels in chunks of whole 62-block groups (the upload_chunk knob) through a ring of at most three chunk buffers.  Chunk k's copy
  (copy stream) carries the next 128 bytes as well: the two lookahead blocks of its last group.  Its kernels (compute stream: k_block_len over
  the chunk's own bytes, k_chunk_carry, k_build_sup_chunk, k_build_recs_chunk; kernels/transcode.hip.h) run while chunk k + 1 is on the link,
  and a ring slot is copied into again only after the kernels of its previous chunk have finished.  What one chunk hands to the next -- the
  position, the six symbol counts, the error word, k_block_len's flags -- stays on the device: no host round trip per chunk.  After the last
  chunk the totals come back once and the header is validated exactly as upload_validate does for the one-shot upload.
*/
#pragma once

namespace
{

struct ChunkedUpload
{
  static constexpr int SLOTS = 3;
  DevBuf bytes[SLOTS];                  // chunk + 128 bytes of lookahead + 16 of padding
  DevBuf blen, gtab;                    // the chunk's block lengths and group tables: one set, the chunks' kernels run one after the other
  DevBuf state[2];                      // UP_STATE_WORDS u64 per input (kernels/transcode.hip.h)
  hipEvent_t copied[SLOTS] = {}, done[SLOTS] = {};
  bool used[SLOTS] = {};
  int nslots = 0, inputs = 0;
  u64 groups_per_chunk = 0, seq = 0, chunks = 0, peak = 0;

  ChunkedUpload() {}
  ChunkedUpload(const ChunkedUpload&) = delete; ChunkedUpload& operator=(const ChunkedUpload&) = delete;
  ~ChunkedUpload()
  {
    // queued copies read the caller's bytes and write the ring: both streams are joined before anything is released
    (void)hipStreamSynchronize(CTX.copy_stream); (void)hipStreamSynchronize(CTX.stream);
    for(int k = 0; k < SLOTS; k++)
    {
      if(copied[k]) { (void)hipEventDestroy(copied[k]); }
      if(done[k]) { (void)hipEventDestroy(done[k]); }
    }
  }

  static u64 groups_of(u64 nbytes) { return std::max<u64>(1, div_up(div_up(nbytes, RLE_BLOCK), (u64)GROUP)); }
  u64 chunk_bytes() const { return groups_per_chunk * GROUP * RLE_BLOCK; }

  // The ring for streams of at most `max_nbytes` bytes: chunks of upload_chunk bytes in whole groups, no larger than the longest stream.
  int prepare(u64 max_nbytes)
  {
    const u64 max_groups = groups_of(max_nbytes);
    groups_per_chunk = std::min(max_groups, std::max<u64>(1, (u64)g_tune.upload_chunk / ((u64)GROUP * RLE_BLOCK)));
    nslots = (int)std::min<u64>(SLOTS, div_up(max_groups, groups_per_chunk));
    for(int k = 0; k < nslots; k++)
    {
      TRY(bytes[k].alloc(chunk_bytes() + 2 * RLE_BLOCK + 16));
      HIP_TRY(hipEventCreateWithFlags(&copied[k], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
    }
    TRY(blen.alloc((groups_per_chunk * GROUP + 2) * sizeof(u64)));
    TRY(gtab.alloc(7 * (groups_per_chunk + 1) * sizeof(u64)));
    note();
    TRY(fork_copy_stream());                                         // the ring may be recycled blocks with queued users
    return BWTM_OK;
  }

  // counted the way Streamer::note() counts the slices: what the call holds besides the records and the super table
  void note()
  {
    u64 total = blen.bytes + gtab.bytes + state[0].bytes + state[1].bytes;
    for(const DevBuf& b : bytes) { total += b.bytes; }
    peak = std::max(peak, total);
  }

  // Queues the whole upload of one input (x->n = the header's bases); its totals travel to host_scratch[slot .. slot + 6].
  int queue(bwtm_index* x, const u8* src, u64 nbytes, u32 slot)
  {
    if(inputs >= 2) { return fail(BWTM_EINVAL, "chunked upload: more than two inputs in one ring"); }
    DevBuf& st = state[inputs++];
    TRY(st.alloc(UP_STATE_WORDS * sizeof(u64), true));
    note();
    const u64 bases = x->n;
    x->nrecs = num_records(bases); x->nsup = num_supers(bases);
    TRY(x->recs.alloc(x->nrecs * 64));
    TRY(x->sup.alloc(x->nsup * SUP_STRIDE * sizeof(u64)));
    const u64 nblocks = div_up(nbytes, RLE_BLOCK), ngroups = groups_of(nbytes), group_bytes = (u64)GROUP * RLE_BLOCK;
    const u64 nchunks = div_up(ngroups, groups_per_chunk);
    // the window of k_build_recs_chunk by the header's density (build_records: by the stream's own, which is the same after validation)
    const u64 per_group = bases / ngroups;
    const bool long_runs = (nblocks > 0 && bases / nblocks > 400);
    const u64 window = (g_tune.recs_window != 0 ? (u64)g_tune.recs_window : (per_group <= 6500 ? 8192 : (per_group <= 14000 ? 16384 : 32768)));
    const bool uniform = (g_tune.recs_uniform != 0 ? g_tune.recs_uniform > 0 : window == 32768);
    u64* state_p = st.as<u64>();
    for(u64 k = 0; k < nchunks; k++, seq++, chunks++)
    {
      const int s = (int)(seq % (u64)nslots);
      const u64 g0 = k * groups_per_chunk, g1 = std::min(ngroups, g0 + groups_per_chunk), ngl = g1 - g0;
      const u32 last = (k + 1 == nchunks ? 1u : 0u);
      const u64 from = g0 * group_bytes, own_to = std::min(nbytes, g1 * group_bytes), to = std::min(nbytes, own_to + 2 * RLE_BLOCK);
      const u64 local_bytes = to - from, local_blocks = div_up(local_bytes, RLE_BLOCK);
      u8* dst = bytes[s].as<u8>();
      hipError_t e = hipSuccess;
      // the stream ends in this chunk: alloc_native's padding behind its last byte.  On the compute stream (behind the kernels of the slot's previous
      // chunk, and the copy does not touch these bytes): the copy stream carries nothing but copies, as in the one-shot upload
      if(to == nbytes) { e = hipMemsetAsync(dst + local_bytes, 0, 16, CTX.stream); }
      if(e == hipSuccess && used[s]) { e = hipStreamWaitEvent(CTX.copy_stream, done[s], 0); }  // the kernels of the slot's previous chunk
      if(e == hipSuccess && local_bytes > 0) { e = hipMemcpyAsync(dst, src + from, local_bytes, hipMemcpyHostToDevice, CTX.copy_stream); }
      if(e == hipSuccess) { e = hipEventRecord(copied[s], CTX.copy_stream); }
      if(e == hipSuccess) { e = hipStreamWaitEvent(CTX.stream, copied[s], 0); }
      if(e != hipSuccess) { return fail(BWTM_ENODEV, "H2D copy failed: %s", hipGetErrorString(e)); }
      used[s] = true;
      const u64 gstride = ngl + 1;
      // block lengths of the chunk's blocks and of its lookahead blocks (the group behind the chunk's own: its counts are overwritten by the carry)
      LAUNCH("block_len", k_block_len, div_up(ngl + (last ? 0 : 1), BLOCK_THREADS / WAVE), BLOCK_THREADS,
        (const u8*)dst, local_bytes, local_blocks, (u64)0, ngl + (last ? 0 : 1), blen.as<u64>(), gtab.as<u64>(), gstride, (u32*)(state_p + UP_STATE_FLAGS));
      LAUNCH("chunk_carry", k_chunk_carry, 1, BLOCK_THREADS, gtab.as<u64>(), gstride, ngl, state_p, bases, last);
      LAUNCH("build_sup", k_build_sup_chunk, div_up(x->nsup * WAVE, BLOCK_THREADS), BLOCK_THREADS,
        (const u8*)dst, local_bytes, blen.as<const u64>(), gtab.as<const u64>(), gstride, local_blocks, ngl, bases, x->sup.as<u64>(), x->nsup,
        (const u64*)state_p, last);
#define BUILD_RECS_CHUNK(W, WAVES, FILL, UNIFORM) do { CTX.transcode_forms[transcode_form(1, W, FILL, UNIFORM)]++; \
        LAUNCH("build_recs", (k_build_recs_chunk<W, WAVES, FILL, UNIFORM>), div_up(ngl, WAVES), WAVES * WAVE, \
        (const u8*)dst, local_bytes, blen.as<const u64>(), gtab.as<const u64>(), gstride, local_blocks, ngl, bases, \
        x->sup.as<const u64>(), x->recs.as<uint4>(), x->nrecs, (const u64*)state_p, last); } while(0)
      if(window == 8192) { if(uniform) { BUILD_RECS_CHUNK(8192, 4, false, true); } else { BUILD_RECS_CHUNK(8192, 4, false, false); } }
      else if(window == 16384) { if(uniform) { BUILD_RECS_CHUNK(16384, 4, false, true); } else { BUILD_RECS_CHUNK(16384, 4, false, false); } }
      else if(!long_runs) { if(uniform) { BUILD_RECS_CHUNK(32768, 2, false, true); } else { BUILD_RECS_CHUNK(32768, 2, false, false); } }
      else { if(uniform) { BUILD_RECS_CHUNK(32768, 2, true, true); } else { BUILD_RECS_CHUNK(32768, 2, true, false); } }
#undef BUILD_RECS_CHUNK
      HIP_TRY(hipEventRecord(done[s], CTX.stream));
    }
    TRY(fetch_u64(state_p, slot, 7));                                 // six totals and the flags: upload_validate's layout
    return BWTM_OK;
  }

  // The one synchronisation: the caller's buffers are free again, the totals are on the host.
  int join() { return join_streams("upload"); }

  // After join(): the header against the stream, with upload_validate's verdicts.  The index keeps records and super table only.
  static int validate(bwtm_index* x, u64 sequences, u64 bases, const u64* C, u32 slot)
  {
    CTX.host_scratch[slot + 6] &= 0xFFFFFFFFull;
    TRY(upload_validate(x, sequences, bases, C, slot));
    x->has_native = false; x->nbytes = 0; x->nblocks = 0; x->ngroups = 0;
    return BWTM_OK;
  }
};

// A new index of the current context from host bytes through the chunked upload: queued only (join and validate follow).
int chunked_index(ChunkedUpload& up, const u8* data, u64 nbytes, u64 sequences, u64 bases, u32 slot, bwtm_index** out)
{
  bwtm_index* x = new bwtm_index();
  *out = x;                                                          // owned by the caller from here on, also on failure
  x->ctx = t_ctx; x->n = bases; x->m = sequences;
  return up.queue(x, data, nbytes, slot);                            // (an empty stream queues no copy: `data` is never read)
}

} // namespace

extern "C" int bwtm_index_upload_streamed(const uint8_t* data, uint64_t nbytes, uint64_t sequences, uint64_t bases,
  const uint64_t* C, bwtm_index** out, bwtm_upload_stats* stats)
{
  ENTER(nullptr);
  if(!out || (nbytes > 0 && !data)) { return fail(BWTM_EINVAL, "bwtm_index_upload_streamed: null argument"); }
  const double t0 = now_ms();
  bwtm_index* x = nullptr;
  int rc = BWTM_OK;
  u64 chunks = 0, chunk_bytes = 0, peak = 0;
  {
    ChunkedUpload up;
    rc = up.prepare(nbytes);
    if(rc == BWTM_OK) { rc = chunked_index(up, data, nbytes, sequences, bases, 0, &x); }
    const int rj = up.join();                                        // also on failure: the caller's buffer is free again
    if(rc == BWTM_OK) { rc = rj; }
    if(rc == BWTM_OK) { rc = ChunkedUpload::validate(x, sequences, bases, C, 0); }
    chunks = up.chunks; chunk_bytes = up.chunk_bytes(); peak = up.peak;
  }
  if(rc != BWTM_OK) { delete x; return rc; }                         // the half-built index
  if(stats) { stats->chunks = chunks; stats->chunk_bytes = chunk_bytes; stats->staging_bytes_peak = peak; stats->ms_total = now_ms() - t0; }
  *out = x;
  return BWTM_OK;
}
