/*
  kernels/kmer_join.hip.h -- the k-mers of TWO collections side by side: one joint walk down the suffix tries of two indexes, one level per step.
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm, behind kernels/kmers.hip.h whose code it uses); gfx950 only.
*/
#pragma once

//------------------------------------------------------------------------------
// A NODE is (sp_a, cnt_a, sp_b, cnt_b, code), 40 bytes, kept as five arrays: the string of t symbols that `code` holds (kernels/kmers.hip.h)
// and, per index x, the range [sp_x, sp_x + cnt_x) of the suffixes of x that start with it.  When cnt_x == 0 the string does not occur in x
// and sp_x is its INSERTION POINT: the number of suffixes of x that are smaller than the string.  The LF formula gives both alike,
//     sp_x' = C_x[c] + rank_x(sp_x, c),   cnt_x' = rank_x(sp_x + cnt_x, c) - rank_x(sp_x, c)
// (the suffixes smaller than cX are those that start with a smaller symbol and those cY with Y < X), so a side whose count has fallen to 0
// is walked on like the other one: there sp == e, level_lane_ranks loads one record, every lane of a wave still does the same thing, and
// the result says where the k-mer would stand in that index -- which makes sp_a + sp_b its position in the merged index.
//
// A child is kept when cnt_a >= min_a, cnt_b >= min_b and cnt_a + cnt_b >= min_sum (min_sum >= 1: a string neither index holds is never
// a node), and cnt_a <= max_a, cnt_b <= max_b.  A count never exceeds its parent's, so the lower bounds prune every level exactly; the upper
// bounds say nothing about a node's children, so the host passes ~0 for them above the last level.
//
// A level is k_kmer_level's two launches over the same frontier with one scan between them (symbol-major totals, the stable split by
// symbol; see there): the frontier stays sorted by code, by sp_a and by sp_b at once, all non-strictly on a dead side.  One lane per node,
// 256 nodes per workgroup: four lanes per node took twice the time on sorted frontiers and are not built here.
// Within a lane A's ranks are taken first, then B's, through the same 16 record words.
//
// No load leaves either index: sp and sp + cnt are clamped to that index's own n before anything is loaded, and rank(n, c) comes from
// that index's C.  There is no loop whose length depends on data.

struct KmerJoinBounds { u64 min_a, max_a, min_b, max_b, min_sum; };
struct KmerJoinNodes { u64* sp_a; u64* cnt_a; u64* sp_b; u64* cnt_b; u64* code; };

constexpr u32 KMER_JOIN_STATS = 7;

// The four children of (sp, cnt) in one index: csp[j], ccnt[j] for the j-th kept symbol.
__device__ inline void kmer_join_side(const IndexView& x, const u64* sC, u32 skip, u64 sp, u64 cnt, u64 csp[4], u64 ccnt[4])
{
  if(sp > x.n) { sp = x.n; }
  if(cnt > x.n - sp) { cnt = x.n - sp; }
  u64 rs[6], re[6];
  level_lane_ranks(x, sC, sp, sp + cnt, rs, re);
#pragma unroll
  for(u32 j = 0; j < 4; j++)
  {
    const bool up = (j + 1 >= skip);                                        // the j-th kept symbol is j + 2, not j + 1
    const u64 a = (up ? rs[j + 2] : rs[j + 1]), b = (up ? re[j + 2] : re[j + 1]);
    csp[j] = sC[kmer_comp(j, skip)] + a; ccnt[j] = (b >= a ? b - a : 0);
  }
}

// EMIT == false: totals[j * nblocks + blockIdx.x] = kept children of symbol j among this workgroup's nodes, and totals[4 * nblocks] = 0.
// EMIT == true:  totals as the exclusive scan left them; the kept children go to out.*[..], never at or beyond `capacity`.
// t = symbols of a node of the frontier `in` (1 <= t < 32), count = its nodes, nblocks = gridDim.x.
template<bool EMIT>
__global__ void __launch_bounds__(BLOCK_THREADS) k_kmer_join_level(IndexView xa, IndexView xb, u32 skip, KmerJoinBounds bd, u32 t, KmerJoinNodes in,
  u64 count, u64 nblocks, u64* totals, KmerJoinNodes out, u64 capacity)
{
  __shared__ u64 sCa[8];
  __shared__ u64 sCb[8];
  __shared__ u32 s_wave[BLOCK_THREADS / WAVE][4];
  if(threadIdx.x < 8) { sCa[threadIdx.x] = xa.C[threadIdx.x]; sCb[threadIdx.x] = xb.C[threadIdx.x]; }
  __syncthreads();
  const u64 k = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  u64 aspc[4] = {0, 0, 0, 0}, acnt[4] = {0, 0, 0, 0}, bspc[4] = {0, 0, 0, 0}, bcnt[4] = {0, 0, 0, 0}, code = 0;
  u32 keep = 0;                                                             // bit j: this lane stores the child of the j-th kept symbol
  if(k < count)
  {
    code = in.code[k];
    kmer_join_side(xa, sCa, skip, in.sp_a[k], in.cnt_a[k], aspc, acnt);
    kmer_join_side(xb, sCb, skip, in.sp_b[k], in.cnt_b[k], bspc, bcnt);
#pragma unroll
    for(u32 j = 0; j < 4; j++)
    {
      const u64 ca = acnt[j], cb = bcnt[j];                                 // each at most its index's n < 2^63: the sum does not wrap
      if(ca >= bd.min_a && ca <= bd.max_a && cb >= bd.min_b && cb <= bd.max_b && ca + cb >= bd.min_sum) { keep |= 1u << j; }
    }
  }
  // the stable split of k_kmer_level: one stream per symbol (kernels/level.hip.h)
  const u32 wave = threadIdx.x >> 6;
  const u64 below = (1ull << lane_id()) - 1ull;
  u32 before[4];
#pragma unroll
  for(u32 j = 0; j < 4; j++)
  {
    u32 wave_total;
    level_place<1>(keep >> j, true, below, &wave_total, &before[j]);
    if(lane_id() == 0) { s_wave[wave][j] = wave_total; }
  }
  __syncthreads();
  if(!EMIT) { level_publish<4>(s_wave, totals, nblocks); return; }
#pragma unroll
  for(u32 j = 0; j < 4; j++)
  {
    if((keep >> j) & 1u)
    {
      const u64 slot = level_slot<4>(s_wave, totals, nblocks, j, wave) + before[j];
      if(slot < capacity)
      {
        nt_store(out.sp_a + slot, aspc[j]); nt_store(out.cnt_a + slot, acnt[j]);
        nt_store(out.sp_b + slot, bspc[j]); nt_store(out.cnt_b + slot, bcnt[j]);
        nt_store(out.code + slot, ((u64)j << (2 * t)) | code);
      }
    }
  }
}

// stats[0..2] += the entries only in a (cnt_b == 0), only in b (cnt_a == 0), in both; stats[3] += the occurrences in a of the first class,
// stats[4] += those in b of the second, stats[5], stats[6] += those in a and in b of the third.  One atomic per workgroup and value.
__global__ void __launch_bounds__(BLOCK_THREADS) k_kmer_join_summary(const u64* cnt_a, const u64* cnt_b, u64 count, unsigned long long* stats)
{
  __shared__ u64 lds[BLOCK_THREADS / WAVE];
  u64 acc[KMER_JOIN_STATS] = {0, 0, 0, 0, 0, 0, 0};
  for(u64 k = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x; k < count; k += (u64)gridDim.x * BLOCK_THREADS)
  {
    const u64 a = cnt_a[k], b = cnt_b[k];
    const bool in_a = (a != 0), in_b = (b != 0);
    acc[0] += (in_a && !in_b ? 1 : 0); acc[1] += (!in_a && in_b ? 1 : 0); acc[2] += (in_a && in_b ? 1 : 0);
    acc[3] += (in_b ? 0 : a); acc[4] += (in_a ? 0 : b);
    acc[5] += (in_b ? a : 0); acc[6] += (in_a ? b : 0);
  }
#pragma unroll
  for(u32 s = 0; s < KMER_JOIN_STATS; s++)
  {
    const u64 total = block_reduce<0>(acc[s], lds);
    if(threadIdx.x == 0 && total != 0) { atomicAdd(stats + s, (unsigned long long)total); }
  }
}
