/*
  kernels/level.hip.h -- what the level-wise trie walks share (no kernel): the ranks of a node's range, and the stable placement of a
  level's children without atomics.  k_kmer_level, k_kmer_join_level, k_approx_level and k_edit_level are built on it.
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm, in front of kernels/kmers.hip.h); gfx950 only.
*/
#pragma once

//------------------------------------------------------------------------------
// A LEVEL takes a frontier of nodes to the next one, and possibly to further output streams, in two launches over the same frontier with
// one exclusive scan between them:
//   the count pass    computes every node's children and leaves totals[s * nblocks + b] = the children of stream s from workgroup b, and
//                     totals[STREAMS * nblocks] = 0.  ONE scan over these STREAMS * nblocks + 1 entries gives every workgroup its first
//                     slot in every stream and, at s * nblocks, the end of stream s - 1, which the host reads back and allocates from.
//   the expand pass   computes the same children again (the ranks are not stored: 64 more bytes per node would be written and read where
//                     one or two records are re-read in order) and stores each at
//                         totals[s * nblocks + b] + the wave totals of the waves before + the children of the lanes before this one.
// Both passes take the ranks the same way, so the second finds what the first counted, and no atomic decides a position: a stream holds
// its children in workgroup, wave, lane and then bit order.  A store is still checked against the capacity by the kernel that makes it.

// rank(sp, .) and rank(e, .) of one lane, sp <= e <= n.  sp == 0: no load.  e == n: from C.  Same record: one load.
__device__ inline void level_lane_ranks(const IndexView& x, const u64* sC, u64 sp, u64 e, u64 rs[6], u64 re[6])
{
  u32 w[16];
  const bool at_end = (e == x.n);
  u64 loaded = ~0ull;
#pragma unroll
  for(u32 c = 1; c < 6; c++) { rs[c] = 0; }
  if(sp > 0)
  {
    loaded = sp >> REC_SHIFT;
    load_record(x.recs, loaded, w);
    const u64* s = x.sup + (sp >> SUPER_SHIFT) * SUP_STRIDE;
    const u32 js = (u32)(sp & (REC_POS - 1));
#pragma unroll
    for(u32 c = 1; c < 6; c++) { rs[c] = s[c] + rec_header(w, c) + rec_count(w, c, js); }
  }
  if(at_end)
  {
#pragma unroll
    for(u32 c = 1; c < 6; c++) { re[c] = sC[c + 1] - sC[c]; }
    return;
  }
  if((e >> REC_SHIFT) != loaded) { load_record(x.recs, e >> REC_SHIFT, w); }
  const u64* s = x.sup + (e >> SUPER_SHIFT) * SUP_STRIDE;
  const u32 je = (u32)(e & (REC_POS - 1));
#pragma unroll
  for(u32 c = 1; c < 6; c++) { re[c] = s[c] + rec_header(w, c) + rec_count(w, c, je); }
}

// One stream within a wave: bit j < BITS of `mask` is a child of this lane, and a lane that does not stand for its node (the other three
// of a quad) brings none.  *wave_total = the children of the wave, *before = those of the lanes in `below`; a lane's own children follow
// in bit order.  Every lane of the wave has to call it.
template<u32 BITS>
__device__ inline void level_place(u32 mask, bool stands, u64 below, u32* wave_total, u32* before)
{
  u32 total = 0, lower = 0;
#pragma unroll
  for(u32 j = 0; j < BITS; j++)
  {
    const u64 ballot = __ballot(stands && ((mask >> j) & 1u));
    total += (u32)__builtin_popcountll(ballot);
    lower += (u32)__builtin_popcountll(ballot & below);
  }
  *wave_total = total; *before = lower;
}

// The end of a count pass, behind the barrier that follows s_wave[wave][s] = the wave's total of stream s: the workgroup's totals, and
// the cell the scan turns into the grand total.
template<u32 STREAMS>
__device__ inline void level_publish(const u32 (*s_wave)[STREAMS], u64* totals, u64 nblocks)
{
  if(threadIdx.x < STREAMS)
  {
    u32 sum = 0;
#pragma unroll
    for(u32 w = 0; w < BLOCK_THREADS / WAVE; w++) { sum += s_wave[w][threadIdx.x]; }
    totals[(u64)threadIdx.x * nblocks + blockIdx.x] = sum;
  }
  if(blockIdx.x == 0 && threadIdx.x == 0) { totals[STREAMS * nblocks] = 0; }
}

// In an expand pass, behind the same barrier: the slot in `stream` of the first child of wave `wave` of this workgroup.
template<u32 STREAMS>
__device__ inline u64 level_slot(const u32 (*s_wave)[STREAMS], const u64* totals, u64 nblocks, u32 stream, u32 wave)
{
  u64 slot = totals[(u64)stream * nblocks + blockIdx.x];
#pragma unroll
  for(u32 w = 0; w < BLOCK_THREADS / WAVE; w++) { if(w < wave) { slot += s_wave[w][stream]; } }
  return slot;
}
