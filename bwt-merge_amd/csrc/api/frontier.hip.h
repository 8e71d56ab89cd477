/*
  api/frontier.hip.h -- the host side of the level scheme of kernels/level.hip.h, stated once for api/kmers.hip.h, api/kmer_join.hip.h,
  api/approx.hip.h and api/edit.hip.h: the frontier of parallel u64 arrays, and the totals of a level with their scan and read-back.
  Part of bwtm_api.hip.

  The memory argument behind every bound of those four files.  A level's size is known only after its count pass, and a block the pool
  has handed out and taken back stays with the pool: a frontier that grew by a little every level would leave a block per level behind.
  So a frontier's capacity AT LEAST DOUBLES when it grows: the blocks one frontier ever had hold fewer than 4 P nodes together, P the
  most nodes it ever held (the last block fewer than 2 P, the earlier ones a geometric series below it).  Two ping-pong frontiers of
  8 ARRAYS bytes per node are therefore 64 ARRAYS P bytes.  A stream that keeps its contents while it grows (grow_keeping) doubles the
  same way, the block being copied from included.  The totals of a level (8 STREAMS bytes per workgroup of nodes) double as well.
*/
#pragma once

namespace
{

// ARRAYS parallel arrays of `cap` u64 each in one block: a frontier, a hit stream, or a result.  `who` is the entry point for the error text.
template<u32 ARRAYS>
struct Frontier
{
  DevBuf buf; u64 cap = 0;
  u64* array(u32 w) const { return buf.as<u64>() + w * cap; }
  void swap(Frontier& o) { buf.swap(o.buf); std::swap(cap, o.cap); }
  // room for `need` nodes; the old contents are not kept
  int reserve(u64 need, const char* who)
  {
    if(need <= cap && buf.p) { return BWTM_OK; }
    const u64 want = std::max<u64>(std::max<u64>(need, 2 * cap), 1);
    if(want > (~0ull) / (8 * ARRAYS)) { return fail(BWTM_ENOMEM, "%s: a frontier of %llu nodes does not fit", who, (unsigned long long)want); }
    TRY(buf.alloc(ARRAYS * want * sizeof(u64)));
    cap = want;
    return BWTM_OK;
  }
  // room for `need` nodes, of which the first `used` are kept; the old block returns to the pool (stream ordered)
  int grow_keeping(u64 used, u64 need, const char* who)
  {
    if(need <= cap && buf.p) { return BWTM_OK; }
    Frontier grown;
    grown.cap = cap;                                                                            // reserve() at least doubles this
    TRY(grown.reserve(need, who));
    return move_into(grown, used);
  }
  // the first `count` >= 1 nodes in a block of exactly that size
  int shrink_to(u64 count, const char* who)
  {
    if(cap == count) { return BWTM_OK; }
    Frontier exact;
    TRY(exact.reserve(count, who));
    return move_into(exact, count);
  }
private:
  int move_into(Frontier& other, u64 count)
  {
    for(u32 w = 0; w < ARRAYS && count > 0; w++)
    {
      HIP_TRY(hipMemcpyAsync(other.array(w), array(w), count * sizeof(u64), hipMemcpyDeviceToDevice, CTX.stream));
    }
    swap(other);
    return BWTM_OK;
  }
};

// The per-workgroup totals of a level: `streams` runs of `nblocks` entries and one more (kernels/level.hip.h).
struct LevelTotals
{
  DevBuf buf; u64 cap = 0;
  u64* p() const { return buf.as<u64>(); }
  int reserve(u32 streams, u64 nblocks)
  {
    const u64 need = streams * nblocks + 1;
    if(need <= cap) { return BWTM_OK; }
    const u64 want = std::max<u64>(need, 2 * cap);
    TRY(buf.alloc(want * sizeof(u64)));
    cap = want;
    return BWTM_OK;
  }
  // Behind the count pass: the scan, and CTX.host_scratch[i] = the end of stream first_stream_read + i - 1, up to the last one.
  int scan_and_read(u32 streams, u64 nblocks, u32 first_stream_read)
  {
    TRY(device_scan<0>(p(), p(), streams * nblocks + 1));
    for(u32 s = first_stream_read; s <= streams; s++) { TRY(fetch_u64(p() + s * nblocks, s - first_stream_read)); }
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    return BWTM_OK;
  }
};

} // namespace
