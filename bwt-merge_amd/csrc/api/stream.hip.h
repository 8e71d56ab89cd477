/*
  api/stream.hip.h -- bwtm_merge_host_streamed: host-resident inputs -> the merged BWT handed to the caller in PIECES, in bounded device
  memory.  Upload and search as bwtm_merge_host; the second half is mergeBWT's own shape (bwt.cpp:215-282: consume, emit, free what
  was consumed): the output-range slices of api/slices.hip.h one after the other on one GPU, at most two alive.  Part of bwtm_api.hip.

  Per slice g:  interleave_range, last head, size table, encode (+ cum32), samples (k_piece_fields), D2H of bytes and samples on the copy
                stream into staging set g & 1 | then piece g - 1: wait for its copies, sink, release.
  So the copies of slice g run under the interleave AND the encoder of slice g + 1 (the copy stream never waits for a slice's three
  small synchronisations), and the sink of piece g runs while the copies of slice g + 1 are in flight.  Slice g + 2 is interleaved
  only after slice g has been released.
*/
#pragma once

namespace
{

// One of the two staging sets: the slice whose piece is on its way, its device-side samples, the page-locked arrays the sink reads.
struct StreamSet
{
  bwtm_slice* slice = nullptr;
  DevBuf dsamp, cumabs;                 // samples as the piece delivers them (+ the longest block); counts of the rank-query form
  u8* host_data = nullptr; u64 host_data_cap = 0;
  u8* host_samp = nullptr; u64 host_samp_cap = 0;
  hipEvent_t ready = nullptr, copied = nullptr;
  bool pending = false;                 // a piece is queued
  PieceSrc src;
  u64 nbytes = 0, g0 = 0, ns = 0, anchor_first = 0, nanch = 0;
  int width = 0, carry_out = 0;
  bool last = false;
};

inline u64 align8(u64 x) { return (x + 7) & ~7ull; }
constexpr int CARRY_RING = 4;

struct Streamer
{
  bwtm_index* a = nullptr; bwtm_index* b = nullptr; bwtm_ra* ra = nullptr;
  int want = 0; bool by_query = false;
  bwtm_piece_fn sink = nullptr; void* user = nullptr;
  StreamSet set[2];
  DevBuf carry;                         // CARRY_RING x 6 u64: the open block, written by one piece's kernel and read by the next one's; a ring,
                                        // because the kernel of piece g - 1 may run again (another width) after the kernel of piece g has run
  int carry_idx = 0; bool has_carry = false;
  u64 head_carry = 0, byte_off = 0, n = 0;
  u64 tail[6] = {};
  int width_guess = 1;
  u64 pieces = 0, peak = 0;
  u64* host_words = nullptr; u64* host_words_dev = nullptr;          // 72 page-locked u64 and their device-visible address (bwtm_slice::host_direct)

  Streamer()
  {
    // the page-locked staging of the context's previous streamed call, if it is still there
    for(int k = 0; k < 2; k++)
    {
      set[k].host_data = (u8*)CTX.stream_stage[2 * k]; set[k].host_data_cap = CTX.stream_stage_cap[2 * k];
      set[k].host_samp = (u8*)CTX.stream_stage[2 * k + 1]; set[k].host_samp_cap = CTX.stream_stage_cap[2 * k + 1];
      CTX.stream_stage[2 * k] = CTX.stream_stage[2 * k + 1] = nullptr; CTX.stream_stage_cap[2 * k] = CTX.stream_stage_cap[2 * k + 1] = 0;
    }
  }
  Streamer(const Streamer&) = delete; Streamer& operator=(const Streamer&) = delete;
  ~Streamer()
  {
    // nothing may touch the staging or a slice's buffers after this: both streams are joined before anything is released
    (void)hipStreamSynchronize(CTX.copy_stream); (void)hipStreamSynchronize(CTX.stream);
    for(int k = 0; k < 2; k++)
    {
      StreamSet& s = set[k];
      delete s.slice;
      CTX.stream_stage[2 * k] = s.host_data; CTX.stream_stage_cap[2 * k] = s.host_data_cap;          // kept for the next call (bwtm_trim returns them)
      CTX.stream_stage[2 * k + 1] = s.host_samp; CTX.stream_stage_cap[2 * k + 1] = s.host_samp_cap;
      if(s.ready) { (void)hipEventDestroy(s.ready); }
      if(s.copied) { (void)hipEventDestroy(s.copied); }
    }
    delete ra; delete a; delete b;
    if(host_words) { (void)hipHostFree(host_words); }
  }

  // What the live slices and the call's device staging hold right now (a slice's own high-water mark since the last look counts:
  // its size tables are gone again when bwtm_slice_encode returns).
  void note()
  {
    u64 total = carry.bytes;
    for(StreamSet& s : set)
    {
      total += s.dsamp.bytes + s.cumabs.bytes;
      if(s.slice) { total += std::max(s.slice->device_bytes(), s.slice->bytes_high); s.slice->bytes_high = 0; }
    }
    peak = std::max(peak, total);
  }

  int host_reserve(u8*& p, u64& cap, u64 need)
  {
    if(need <= cap) { return BWTM_OK; }
    if(p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
    const u64 want_bytes = need + need / 4 + 64;
    hipError_t e = hipHostMalloc((void**)&p, want_bytes, hipHostMallocDefault);
    if(e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return fail(BWTM_ENOMEM, "bwtm_merge_host_streamed: hipHostMalloc(%llu bytes) failed: %s", (unsigned long long)want_bytes, hipGetErrorString(e)); }
    cap = want_bytes;
    return BWTM_OK;
  }

  static u64 samp_a_bytes(u64 ns, int width) { return align8(6 * ns * (u64)width); }
  static u64 samp_b_bytes(u64 ns, u64 nanch, int width) { return (width == 8 ? ns : 6 * nanch) * sizeof(u64); }

  // Queues the piece's samples in the given width (the kernel, then the copy into the set's page-locked staging).
  int queue_samples(StreamSet& S, int width)
  {
    S.width = width;
    const u64 bytes_a = samp_a_bytes(S.ns, width), bytes_b = samp_b_bytes(S.ns, S.nanch, width), total = bytes_a + bytes_b + sizeof(u64);
    TRY(S.dsamp.alloc(total));
    u8* d = S.dsamp.as<u8>();
    u64* part_b = (u64*)(d + bytes_a);
    unsigned long long* mx = (unsigned long long*)(d + bytes_a + bytes_b);
    HIP_TRY(hipMemsetAsync(mx, 0, sizeof(u64), CTX.stream));
    u64* cout_ptr = carry.as<u64>() + 6 * S.carry_out;
    const u64 grid = div_up(std::max<u64>(S.ns, 1), BLOCK_THREADS);
    if(width == 1) { LAUNCH("piece_fields", k_piece_fields<u8>, grid, BLOCK_THREADS, S.src, S.ns, S.g0, (u8*)d, part_b, S.anchor_first, S.nanch, cout_ptr, mx); }
    else if(width == 2) { LAUNCH("piece_fields", k_piece_fields<unsigned short>, grid, BLOCK_THREADS, S.src, S.ns, S.g0, (unsigned short*)d, part_b, S.anchor_first, S.nanch, cout_ptr, mx); }
    else if(width == 4) { LAUNCH("piece_fields", k_piece_fields<u32>, grid, BLOCK_THREADS, S.src, S.ns, S.g0, (u32*)d, part_b, S.anchor_first, S.nanch, cout_ptr, mx); }
    else { LAUNCH("piece_fields", k_piece_fields<u64>, grid, BLOCK_THREADS, S.src, S.ns, S.g0, (u64*)d, part_b, S.anchor_first, S.nanch, cout_ptr, mx); }
    TRY(host_reserve(S.host_samp, S.host_samp_cap, total));
    HIP_TRY(hipEventRecord(S.ready, CTX.stream));
    HIP_TRY(hipStreamWaitEvent(CTX.copy_stream, S.ready, 0));
    HIP_TRY(hipMemcpyAsync(S.host_samp, d, total, hipMemcpyDeviceToHost, CTX.copy_stream));
    return BWTM_OK;
  }

  // Slice g has been interleaved into S.slice: the rest of its device work, and its copies.
  int process(StreamSet& S, bool is_last)
  {
    bwtm_slice* s = S.slice;
    s->host_direct = host_words_dev;
    u64 lh = 0, table[64];
    TRY(bwtm_slice_lasthead(s, &lh));                        // the carry is the running maximum over the slices before
    TRY(bwtm_slice_size_table(s, head_carry, table));
    note();
    // the byte offset is known from the slice before: no fold across slices
    const u64 expect_end = byte_off + table[byte_off & 63];
    TRY(slice_encode(s, byte_off, want != BWTM_SAMPLES_NONE && !by_query));
    if(s->byte_end != expect_end) { return fail(BWTM_ENODEV, "bwtm_merge_host_streamed: a slice wrote %llu bytes, its size table says %llu", (unsigned long long)(s->byte_end - byte_off), (unsigned long long)(expect_end - byte_off)); }
    if(lh > head_carry) { head_carry = lh; }
    S.nbytes = s->byte_end - s->byte_first;
    byte_off = s->byte_end;
    S.last = is_last;
    const u64 nb = s->nblocks;
    const u64 entries = (want != BWTM_SAMPLES_NONE ? (has_carry ? 1 : 0) + nb + (is_last ? 1 : 0) : 0);
    S.ns = (entries > 0 ? entries - 1 : 0);
    S.g0 = s->block_first - (has_carry ? 1 : 0);
    S.anchor_first = div_up(S.g0, 64);
    S.nanch = (S.ns > 0 && S.anchor_first * 64 < S.g0 + S.ns ? (S.g0 + S.ns - 1) / 64 - S.anchor_first + 1 : 0);
    S.width = (want == BWTM_SAMPLES_FULL ? 8 : (want == BWTM_SAMPLES_COMPACT ? 1 : 0));
    if(S.nbytes == 0 && entries <= (has_carry ? 1u : 0u) && !is_last)
    {
      // inside one run: no head, no byte, no block -- no piece
      note();
      delete S.slice; S.slice = nullptr;
      return BWTM_OK;
    }
    if(S.nbytes > 0)
    {
      TRY(host_reserve(S.host_data, S.host_data_cap, S.nbytes));
      HIP_TRY(hipEventRecord(S.ready, CTX.stream));
      HIP_TRY(hipStreamWaitEvent(CTX.copy_stream, S.ready, 0));
      HIP_TRY(hipMemcpyAsync(S.host_data, s->stream_byte(s->byte_first), S.nbytes, hipMemcpyDeviceToHost, CTX.copy_stream));
    }
    if(entries > 0 && (S.ns > 0 || nb > 0))
    {
      if(by_query && nb > 0)
      {
        TRY(S.cumabs.alloc(6 * nb * sizeof(u64)));
        TRY(slice_block_cum(s, S.cumabs.as<u64>()));
      }
      S.src.block_start = s->block_start.as<const u64>();
      S.src.cum32 = (by_query ? (const u32*)nullptr : s->cum32.as<const u32>());
      S.src.cum = (by_query ? S.cumabs.as<const u64>() : (const u64*)nullptr);
      S.src.sup = s->sup.as<const u64>();
      S.src.carry = carry.as<const u64>() + 6 * carry_idx;
      S.src.nb = nb; S.src.has_carry = (has_carry ? 1u : 0u); S.src.has_tail = (is_last ? 1u : 0u);
      for(int c = 0; c < 6; c++) { S.src.tail[c] = tail[c]; }
      S.carry_out = (carry_idx + 1) % CARRY_RING;
      TRY(queue_samples(S, want == BWTM_SAMPLES_FULL ? 8 : width_guess));
      if(nb > 0) { carry_idx = S.carry_out; has_carry = true; }         // (without a block of its own the kernel rewrote nothing: the carry stays)
    }
    HIP_TRY(hipEventRecord(S.copied, CTX.copy_stream));
    S.pending = true;
    note();
    return BWTM_OK;
  }

  // Waits for the piece's copies, hands it to the sink, releases the slice.
  int finish(StreamSet& S)
  {
    if(!S.pending) { return BWTM_OK; }
    S.pending = false;
    HIP_TRY(hipEventSynchronize(S.copied));
    if(want == BWTM_SAMPLES_COMPACT && S.ns > 0)
    {
      // the narrowest width that holds the piece's longest block (samples_width's rule): the guess was the width of the piece before
      const u64 mx = *(const u64*)(S.host_samp + samp_a_bytes(S.ns, S.width) + samp_b_bytes(S.ns, S.nanch, S.width));
      const int need = (mx < 0xFFull ? 1 : (mx < 0xFFFFull ? 2 : (mx < 0xFFFFFFFFull ? 4 : 8)));
      if(need != S.width)
      {
        TRY(queue_samples(S, need));
        HIP_TRY(hipStreamSynchronize(CTX.copy_stream));
        note();
      }
      width_guess = (need == 8 ? 4 : need);
    }
    bwtm_piece pc;
    std::memset(&pc, 0, sizeof(pc));
    pc.byte_first = S.slice->byte_first; pc.nbytes = S.nbytes; pc.data = (S.nbytes > 0 ? S.host_data : nullptr);
    if(S.ns == 0) { S.width = (want == BWTM_SAMPLES_FULL ? 8 : (want == BWTM_SAMPLES_COMPACT ? 1 : 0)); }
    pc.sample_block_first = S.g0; pc.sample_blocks = S.ns; pc.sample_width = S.width;
    pc.last = (S.last ? 1 : 0);
    if(S.ns > 0 && S.width == 8)
    {
      pc.cum = (const u64*)S.host_samp; pc.block_end = (const u64*)(S.host_samp + samp_a_bytes(S.ns, 8));
    }
    else if(S.ns > 0)
    {
      pc.fields = S.host_samp; pc.anchors = (S.nanch > 0 ? (const u64*)(S.host_samp + samp_a_bytes(S.ns, S.width)) : nullptr);
      pc.anchor_first = S.anchor_first; pc.nanchors = S.nanch;
    }
    pieces++;
    const int stop = sink(user, &pc);
    S.dsamp.release(); S.cumabs.release();
    delete S.slice; S.slice = nullptr;
    if(stop != 0) { return fail(BWTM_EINVAL, "bwtm_merge_host_streamed: the sink returned %d for piece %llu and stopped the merge", stop, (unsigned long long)(pieces - 1)); }
    return BWTM_OK;
  }
};

// Two slices within a fixed share (a quarter) of the free device memory at 256 bytes per record (the bound on a live slice: records 64,
// bytes <= 128, block starts + cum32 <= 56, size tables 0.5), in whole segments, and no more than 2^20 records: measured at config 2
//  the second half is fastest with slices of 2^18 .. 2^20 records -- the first slice's device work and the last
// slice's copy are the only parts of the pipeline nothing runs under, and both grow with the slice -- and 2^20 keeps the number of
// pieces (and of per-slice synchronisations) four times smaller.
u64 auto_slice_records()
{
  size_t free_bytes = 0, total_bytes = 0;
  if(hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) { (void)hipGetLastError(); free_bytes = 0; }
  const u64 avail = (u64)free_bytes + CTX.cached_bytes;
  u64 recs = avail / 4 / 2 / 256;
  recs = std::min<u64>(recs, 1ull << 20);
  recs = recs / SLICE_ALIGN * SLICE_ALIGN;
  return std::max<u64>(recs, SLICE_ALIGN);
}

int merge_host_streamed_impl(bwtm_index* a_dev, const bwtm_host_input* a_host, const bwtm_host_input* b_host, u64 slice_records, int want_samples,
  bwtm_piece_fn sink, void* user, bwtm_host_output* out, bwtm_stream_stats* stats)
{
  const double t0 = now_ms();
  Streamer st;                                                       // owns a, b, ra, the slices and the staging: released on every path
  st.a = a_dev; st.want = want_samples; st.sink = sink; st.user = user; st.by_query = (g_tune.stream_samples_query != 0);
  std::memset(out, 0, sizeof(*out));
  // Upload and transcode as merge_host_impl does (upload_pipelined) -- but b's native bytes go as soon as b is transcoded, not after a.
  if(g_tune.stream_upload)
  {
    // The chunked upload: b's chunks, then a's, through one ring; neither stream is ever resident as a whole.  One synchronisation for both.
    ChunkedUpload up;
    TRY(up.prepare(std::max<u64>(b_host->nbytes, a_host ? a_host->nbytes : 0)));
    int rc = chunked_index(up, b_host->data, b_host->nbytes, b_host->sequences, b_host->bases, 8, &st.b);
    if(rc == BWTM_OK && a_host) { rc = chunked_index(up, a_host->data, a_host->nbytes, a_host->sequences, a_host->bases, 16, &st.a); }
    const int rj = up.join();                                        // also on failure: the caller's buffers are free again
    TRY(rc); TRY(rj);
    TRY(ChunkedUpload::validate(st.b, b_host->sequences, b_host->bases, b_host->C, 8));
    if(a_host) { TRY(ChunkedUpload::validate(st.a, a_host->sequences, a_host->bases, a_host->C, 16)); }
    st.peak = std::max(st.peak, up.peak);
  }
  else
  {
    UploadEvents ev_a, ev_b;
    TRY(upload_pipelined({a_host, &st.a, &ev_a}, {b_host, &st.b, &ev_b}, {}, true));
  }
  if(st.a->ctx != t_ctx) { return fail(BWTM_EINVAL, "bwtm_merge_host_streamed: the index lives in another context"); }
  WHOLE_INDEX(st.a, "bwtm_merge_host_streamed");
  TRY(bwtm_index_drop_native(st.a));
  const double t1 = now_ms();
  out->ms_upload = t1 - t0;

  bwtm_index* a = st.a; bwtm_index* b = st.b;
  TRY(ra_make(a, b, &st.ra));
  if(b->m > 0) { TRY(bwtm_search(a, b, 0, b->m - 1, st.ra)); }
  TRY(ra_finalize(st.ra));
  TRY(check_interleave_args(a, b, st.ra));
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  const double t2 = now_ms();
  out->ms_search = t2 - t1;

  const u64 n = st.ra->n_out, nrecs = st.ra->nrecs_out;
  merged_header(a, b, &out->bases, &out->sequences, out->C, 7);
  st.n = n;
  st.tail[0] = n;
  for(int c = 1; c < 6; c++) { st.tail[c] = out->C[c + 1] - out->C[c]; }
  if(slice_records == 0) { slice_records = auto_slice_records(); }
  slice_records = std::min(slice_records, div_up(nrecs, SLICE_ALIGN) * SLICE_ALIGN);

  if(n == 0)
  {
    // the empty result: no byte, no block; the final piece is delivered all the same
    bwtm_piece pc; std::memset(&pc, 0, sizeof(pc));
    pc.last = 1; pc.sample_width = (want_samples == BWTM_SAMPLES_FULL ? 8 : (want_samples == BWTM_SAMPLES_COMPACT ? 1 : 0));
    st.pieces = 1;
    const int stop = sink(user, &pc);
    if(stop != 0) { return fail(BWTM_EINVAL, "bwtm_merge_host_streamed: the sink returned %d for piece 0 and stopped the merge", stop); }
  }
  else
  {
    TRY(st.carry.alloc(CARRY_RING * 6 * sizeof(u64), true));
    HIP_TRY(hipHostMalloc((void**)&st.host_words, 72 * sizeof(u64), hipHostMallocDefault));
    HIP_TRY(hipHostGetDevicePointer((void**)&st.host_words_dev, st.host_words, 0));
    for(StreamSet& S : st.set)
    {
      HIP_TRY(hipEventCreateWithFlags(&S.ready, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&S.copied, hipEventDisableTiming));
    }
    const u64 nslices = div_up(nrecs, slice_records);
    for(u64 g = 0; g < nslices; g++)
    {
      StreamSet& S = st.set[g & 1];
      const u64 r0 = g * slice_records, r1 = std::min(nrecs, r0 + slice_records);
      TRY(bwtm_interleave_range(a, b, st.ra, r0, r1, &S.slice));
      st.note();
      TRY(st.process(S, g + 1 == nslices));
      if(g > 0) { TRY(st.finish(st.set[(g - 1) & 1])); }
    }
    TRY(st.finish(st.set[(nslices - 1) & 1]));
  }
  HIP_TRY(hipStreamSynchronize(CTX.copy_stream));
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  const double t3 = now_ms();
  out->nbytes = st.byte_off; out->blocks = div_up(st.byte_off, RLE_BLOCK);
  out->sample_width = 0;
  out->ms_encode_download = t3 - t2; out->ms_total = t3 - t0;
  if(stats)
  {
    stats->pieces = st.pieces; stats->slice_records = slice_records; stats->slice_bytes_peak = st.peak;
    stats->ms_upload = out->ms_upload; stats->ms_search = out->ms_search; stats->ms_second_half = t3 - t2; stats->ms_total = t3 - t0;
  }
  return BWTM_OK;
}

} // namespace

extern "C" int bwtm_merge_host_streamed(bwtm_index* a_device, const bwtm_host_input* a_host, const bwtm_host_input* b_host,
  uint64_t slice_records, int want_samples, bwtm_piece_fn sink, void* user, bwtm_host_output* out, bwtm_stream_stats* stats)
{
  const bool bad = (!b_host || !sink || !out || ((a_device != nullptr) == (a_host != nullptr)) || (a_host && a_host->nbytes > 0 && !a_host->data) ||
    (b_host->nbytes > 0 && !b_host->data) || slice_records % SLICE_ALIGN != 0 ||
    (want_samples != BWTM_SAMPLES_NONE && want_samples != BWTM_SAMPLES_FULL && want_samples != BWTM_SAMPLES_COMPACT));
  if(bad)
  {
    bwtm_index_free(a_device);
    return fail(BWTM_EINVAL, "bwtm_merge_host_streamed: exactly one form of a, b, a sink, slice_records a multiple of %llu and samples NONE / FULL / COMPACT are required", (unsigned long long)SLICE_ALIGN);
  }
  Scope scope_(a_device ? a_device->ctx : nullptr);
  if(scope_.rc != BWTM_OK) { bwtm_index_free(a_device); return scope_.rc; }      // consumed on every exit path
  return merge_host_streamed_impl(a_device, a_host, b_host, slice_records, want_samples, sink, user, out, stats);
}
