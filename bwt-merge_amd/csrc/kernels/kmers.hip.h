/*
  kernels/kmers.hip.h -- the k-mers of a collection with their counts: the suffix trie of the index down to depth k, one level per step.
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm, behind kernels/quad.hip.h whose record reader it uses); gfx950 only.
*/
#pragma once

//------------------------------------------------------------------------------
// A NODE is (sp, count, code): the BWT range [sp, sp + count) of the suffixes that start with a string of t symbols, none of them the
// endmarker or `skip` (the comp of N), and the string itself, two bits per symbol (the rank of the symbol among the four kept comp values),
// first symbol in the highest used bits.  The nodes of one level are a FRONTIER, kept as three arrays, sorted by sp and by code at once.
//
// From level t to t + 1, for every node and every kept symbol c of rank j:
//     sp' = C[c] + rank(sp, c),  count' = rank(sp + count, c) - rank(sp, c),  code' = (j << 2 t) | code
// and the child is kept when count' >= min_count (>= 1).  A node's count never exceeds its parent's, so dropping a child drops exactly the
// k-mers below it that the threshold drops anyway.  The next frontier is the STABLE SPLIT by c: the kept children of the first symbol in
// parent order, then those of the second, ...  LF is monotone per symbol, so it is sorted again, and the parents' records are read in
// ascending order.
//
// A level is the count pass, the scan and the expand pass of kernels/level.hip.h with one stream per symbol (symbol-major totals): the last
// entry of the scan is the size of the next frontier, which the host reads once per level and allocates from.
//
// QUAD = false: one lane per node, the whole record in its registers (index_ranks' way, k_find_batch's shape); 256 nodes per workgroup.
//               The default: a frontier is sorted by sp, so neighbouring lanes read the same or the next record and the loads of a wave
//               fall into few lines, which is what the quads buy a walk whose positions are scattered.
// QUAD = true:  four lanes per node on the record reader of kernels/quad.hip.h: lane q loads chunk q, every rank is a quad sum, and lane q
//               keeps the child of the q-th kept symbol; 64 nodes per workgroup.  Twice the time of the lanes on the 3 Gbase index of
//               tools/kmer_bench.py: instantiated in the diagnostics build only (bwtm_tune("kmers_kernel", 1)),
//               as the partner of that comparison.
// When sp and sp + count lie in the same record -- the common case in the deep levels of a read collection -- it is loaded once.
//
// No load leaves the index, whatever the records hold: sp is clamped to n and sp + count to n before anything is loaded (records and
// super rows exist for the positions 0 .. n, bwtm_device.h), and rank(n, c) is C[c + 1] - C[c], not a load.  There is no loop whose
// length depends on data.

constexpr u32 KMER_MAX_K = 32;
constexpr u32 KMER_HIST_LDS = 4096;               // bins a workgroup of k_kmer_hist keeps in LDS

template<bool QUAD> constexpr u32 kmer_block_nodes() { return (QUAD ? BLOCK_THREADS / 4 : BLOCK_THREADS); }

// The comp value of the j-th kept symbol (j = 0..3): 1..5 without skip, ascending.
__host__ __device__ inline u32 kmer_comp(u32 j, u32 skip) { return j + 1 + (j + 1 >= skip ? 1u : 0u); }

// EMIT == false: totals[j * nblocks + blockIdx.x] = kept children of symbol j among this workgroup's nodes, and totals[4 * nblocks] = 0.
// EMIT == true:  totals as the exclusive scan left them; the kept children go to out_*[..], never at or beyond `capacity`.
// t = symbols of a node of the frontier in_* (1 <= t < 32), count = its nodes, nblocks = gridDim.x.
template<bool QUAD, bool EMIT>
__global__ void __launch_bounds__(BLOCK_THREADS) k_kmer_level(IndexView x, u32 skip, u64 min_count, u32 t, const u64* in_sp, const u64* in_cnt, const u64* in_code,
  u64 count, u64 nblocks, u64* totals, u64* out_sp, u64* out_cnt, u64* out_code, u64 capacity)
{
  __shared__ u64 sC[8];
  __shared__ u32 s_wave[BLOCK_THREADS / WAVE][4];
  load_C(sC, x);
  const u32 q = threadIdx.x & 3;
  const u64 k = (QUAD ? ((u64)blockIdx.x * BLOCK_THREADS + threadIdx.x) >> 2 : (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x);
  u64 csp[4] = {0, 0, 0, 0}, ccnt[4] = {0, 0, 0, 0}, code = 0;
  u32 keep = 0;                                                             // bit j: this lane stores the child of the j-th kept symbol
  if(k < count)                                                             // quad-uniform
  {
    u64 sp = in_sp[k], cnt = in_cnt[k];
    code = in_code[k];
    if(sp > x.n) { sp = x.n; }
    if(cnt > x.n - sp) { cnt = x.n - sp; }
    const u64 e = sp + cnt;
    if(QUAD)
    {
      const bool at_end = (e == x.n);
      const bool one = (at_end || (e >> REC_SHIFT) == (sp >> REC_SHIFT));   // quad-uniform
      QuadRec ra, rb;
      if(one) { quad_load(x, sp, q, ra); rb = ra; }
      else { quad_load(x, sp, e, q, ra, rb); }
#pragma unroll
      for(u32 j = 0; j < 4; j++)
      {
        const u32 c = kmer_comp(j, skip);
        const u64 a = quad_rank(ra, q, c, sp);
        const u64 b = (at_end ? sC[c + 1] - sC[c] : quad_rank(rb, q, c, e));
        csp[j] = sC[c] + a; ccnt[j] = b - a;
        if(j == q && b >= a && b - a >= min_count) { keep = 1u << j; }
      }
    }
    else
    {
      u64 rs[6], re[6];
      level_lane_ranks(x, sC, sp, e, rs, re);
#pragma unroll
      for(u32 j = 0; j < 4; j++)
      {
        const bool up = (j + 1 >= skip);                                    // the j-th kept symbol is j + 2, not j + 1
        const u64 a = (up ? rs[j + 2] : rs[j + 1]), b = (up ? re[j + 2] : re[j + 1]);
        csp[j] = sC[kmer_comp(j, skip)] + a; ccnt[j] = b - a;
        if(b >= a && b - a >= min_count) { keep |= 1u << j; }
      }
    }
  }
  // the stable split: one stream per symbol (kernels/level.hip.h)
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
        nt_store(out_sp + slot, csp[j]); nt_store(out_cnt + slot, ccnt[j]); nt_store(out_code + slot, ((u64)j << (2 * t)) | code);
      }
    }
  }
}

// *out += the sum of cnt[0 .. count): one atomic per workgroup.
__global__ void __launch_bounds__(BLOCK_THREADS) k_kmer_sum(const u64* cnt, u64 count, unsigned long long* out)
{
  __shared__ u64 lds[BLOCK_THREADS / WAVE];
  u64 acc = 0;
  for(u64 k = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x; k < count; k += (u64)gridDim.x * BLOCK_THREADS) { acc += cnt[k]; }
  const u64 total = block_reduce<0>(acc, lds);
  if(threadIdx.x == 0 && total != 0) { atomicAdd(out, (unsigned long long)total); }
}

// hist[min(cnt[k], bins - 1)]++ for k < count.  The first KMER_HIST_LDS bins -- where a spectrum has its mass -- are counted in LDS and
// flushed once per workgroup; a count beyond them (the spectrum's tail, when the caller asks for more bins than that) goes to its bin directly.
__global__ void __launch_bounds__(BLOCK_THREADS) k_kmer_hist(const u64* cnt, u64 count, u64 bins, unsigned long long* hist)
{
  __shared__ u32 s_bins[KMER_HIST_LDS];
  const u32 local = (u32)(bins < KMER_HIST_LDS ? bins : KMER_HIST_LDS);
  for(u32 b = threadIdx.x; b < local; b += BLOCK_THREADS) { s_bins[b] = 0; }
  __syncthreads();
  for(u64 k = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x; k < count; k += (u64)gridDim.x * BLOCK_THREADS)
  {
    const u64 c = cnt[k];
    const u64 b = (c < bins - 1 ? c : bins - 1);
    if(b < local) { atomicAdd(&s_bins[(u32)b], 1u); }
    else { atomicAdd(hist + b, 1ull); }
  }
  __syncthreads();
  for(u32 b = threadIdx.x; b < local; b += BLOCK_THREADS)
  {
    const u32 v = s_bins[b];
    if(v != 0) { atomicAdd(hist + b, (unsigned long long)v); }
  }
}
