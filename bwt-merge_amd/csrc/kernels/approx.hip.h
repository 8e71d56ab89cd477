/*
  kernels/approx.hip.h -- patterns with up to d substitutions: a backward search whose frontier carries ranges, so that the Hamming
  neighbours of a pattern share every prefix of the search and a branch dies when its range is empty.
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm, behind kernels/level.hip.h whose level it is); gfx950 only.
*/
#pragma once

//------------------------------------------------------------------------------
// A NODE is (sp, count, meta): the BWT range [sp, sp + count) of the suffixes that start with a string W, and in meta the pattern's
// number within the batch (bits 24..55), the symbols of the pattern still to match (bits 8..23: W stands against the pattern's last
// |P| - left symbols) and the mismatches spent so far (bits 0..7).  The FRONTIER holds the nodes of every pattern of the batch, grouped by
// pattern in pattern order; all nodes of one pattern have the same `left`.  It starts as one root (0, n, |P|, 0) per pattern.
//
// One level, for every node with left >= 1 and every comp value c = 1..5 (an endmarker never extends a match):
//     sp' = C[c] + rank(sp, c),  count' = rank(sp + count, c) - rank(sp, c),  spent' = spent + (c != P[left - 1]),  left' = left - 1
// and the child is kept when count' >= 1 and spent' <= max_mismatches.  A kept child with left' == 0 is a HIT and goes to the hit stream,
// any other one to the next frontier; both streams take the children in parent order, then symbol order.  So the frontier stays grouped
// by pattern, all hits of a pattern appear in one level, next to each other, and they are ascending when the matched strings are compared
// from their last symbol backwards -- the order of a depth-first search that tries the symbols 1..5 in turn.  A root with left == 0 (the
// empty pattern) is a hit itself: it goes to the hit stream as it is.
//
// A level is the count pass, the scan and the expand pass of kernels/level.hip.h with two streams, the next frontier (0) and the hits (1):
// after the scan totals[nblocks] is the size of the next frontier and totals[2 nblocks] that size plus the hits of the level, which the
// host reads back and allocates from; the expand pass moves its hit slots from behind the next frontier to behind the batch's earlier hits.
//
// QUAD = false: one lane per node, the whole record in its registers (k_kmer_level<false, .>'s way); 256 nodes per workgroup.  The default.
// QUAD = true:  four lanes per node on the record reader of kernels/quad.hip.h: lane q loads chunk q, every rank is a quad sum, every lane
//               of the quad knows all five children, lane 0 stands for the node in the ballots and lane q stores the child of the comp
//               value q + 1 (lane 0 that of 5 as well); 64 nodes per workgroup.  Instantiated in the diagnostics build only
//               (bwtm_tune("approx_kernel", 1)), as the partner of the comparison in DESIGN.md section 3.11; the same results.
// No load leaves the index, whatever the nodes hold:
// sp and sp + count are clamped to n first, a node with count == 0 loads nothing, rank(0, .) is 0 and rank(n, .) is C[c + 1] - C[c],
// neither of them a load -- so a root loads nothing, and a range that ends at n loads the record of sp alone, also when n is a multiple of
// the record's 128 positions.  The pattern's symbol is read only from inside the batch's text.  Every store is checked against the
// capacity the host allocated from the read-back.  There is no loop whose length depends on data.

constexpr u32 APPROX_MAX_MISMATCHES = 8;
constexpr u64 APPROX_MAX_LEN = 65535;             // `left` has 16 bits

__host__ __device__ inline u64 approx_meta(u64 pattern, u64 left, u64 spent) { return (pattern << 24) | (left << 8) | spent; }
__host__ __device__ inline u64 approx_pattern(u64 meta) { return meta >> 24; }

// Three arrays of `capacity` entries: a frontier, or the hit stream of a batch.
struct ApproxNodes
{
  u64* sp; u64* cnt; u64* meta; u64 capacity;
};

// level_lane_ranks for the four lanes of a quad (lane q of it): chunk q of each record, every rank a quad sum.  Quad-uniform.
__device__ inline void approx_quad_ranks(const IndexView& x, const u64* sC, u32 q, u64 sp, u64 e, u64 rs[6], u64 re[6])
{
  const bool at_end = (e == x.n), from_zero = (sp == 0);
  QuadRec ra, rb;
  ra.ch = make_uint4(0, 0, 0, 0); ra.s_q = 0; ra.s_5 = 0; rb = ra;
  if(from_zero && at_end) { }                                                          // the root: no load
  else if(from_zero) { quad_load(x, e, q, rb); }
  else if(at_end || (e >> REC_SHIFT) == (sp >> REC_SHIFT)) { quad_load(x, sp, q, ra); rb = ra; }
  else { quad_load(x, sp, e, q, ra, rb); }
#pragma unroll
  for(u32 c = 1; c < 6; c++)
  {
    const u64 a = quad_rank(ra, q, c, sp), b = quad_rank(rb, q, c, e);                 // every lane of the quad takes part in the sums
    rs[c] = (from_zero ? 0 : a);
    re[c] = (at_end ? sC[c + 1] - sC[c] : b);
  }
}

// One root per pattern of the batch: out[k] = (0, n, (k, |P_k|, 0)), k < nb <= out.capacity.
__global__ void __launch_bounds__(BLOCK_THREADS) k_approx_roots(const u64* offsets, u64 nb, u64 n, ApproxNodes out)
{
  const u64 k = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(k >= nb || k >= out.capacity) { return; }
  const u64 begin = offsets[k], end = offsets[k + 1];
  u64 len = (end > begin ? end - begin : 0);
  if(len > APPROX_MAX_LEN) { len = APPROX_MAX_LEN; }                       // the host has refused such a pattern
  out.sp[k] = 0; out.cnt[k] = n; out.meta[k] = approx_meta(k, len, 0);
}

template<bool QUAD> constexpr u32 approx_block_nodes() { return (QUAD ? BLOCK_THREADS / 4 : BLOCK_THREADS); }

// QUAD: four lanes per node (see above).
// EMIT == false: totals[blockIdx.x] and totals[nblocks + blockIdx.x] = this workgroup's children for the next frontier and its hits.
// EMIT == true:  totals as the exclusive scan left them; the children go to next.*[..] and hits.*[hit_base + ..], never at or beyond
//                either capacity.
// text[0 .. text_bytes) and offsets[0 .. nb] are the batch's patterns, count = nodes of the frontier `in`, nblocks = gridDim.x.
template<bool QUAD, bool EMIT>
__global__ void __launch_bounds__(BLOCK_THREADS) k_approx_level(IndexView x, const u8* text, u64 text_bytes, const u64* offsets, u64 nb, u32 max_mismatches,
  const u64* in_sp, const u64* in_cnt, const u64* in_meta, u64 count, u64 nblocks, u64* totals, ApproxNodes next, ApproxNodes hits, u64 hit_base)
{
  __shared__ u64 sC[8];
  __shared__ u32 s_wave[BLOCK_THREADS / WAVE][2];
  load_C(sC, x);
  const u32 q = threadIdx.x & 3;
  const u64 k = (QUAD ? ((u64)blockIdx.x * BLOCK_THREADS + threadIdx.x) >> 2 : (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x);
  u64 csp[5] = {0, 0, 0, 0, 0}, ccnt[5] = {0, 0, 0, 0, 0}, cmeta[5] = {0, 0, 0, 0, 0};
  u32 keep = 0;                                                             // bit j: the child of comp value j + 1 is kept
  bool is_hit = false;                                                      // this lane's kept children are hits
  if(k < count)                                                             // quad-uniform, as every branch below: they depend on the node alone
  {
    u64 sp = in_sp[k], cnt = in_cnt[k];
    const u64 meta = in_meta[k];
    if(sp > x.n) { sp = x.n; }
    if(cnt > x.n - sp) { cnt = x.n - sp; }
    const u64 pattern = approx_pattern(meta), left = (meta >> 8) & 0xFFFFu, spent = meta & 0xFFu;
    if(left == 0)                                                           // the empty pattern's root
    {
      csp[0] = sp; ccnt[0] = cnt; cmeta[0] = meta; keep = 1; is_hit = true;
    }
    else if(cnt > 0 && pattern < nb)
    {
      const u64 at = offsets[pattern] + left - 1;
      if(at < text_bytes)
      {
        const u32 want = text[at];
        u64 rs[6], re[6];
        if(QUAD) { approx_quad_ranks(x, sC, q, sp, sp + cnt, rs, re); }
        else { level_lane_ranks(x, sC, sp, sp + cnt, rs, re); }
#pragma unroll
        for(u32 j = 0; j < 5; j++)
        {
          const u64 a = rs[j + 1], b = re[j + 1];
          const u64 cost = spent + (j + 1 != want ? 1u : 0u);
          csp[j] = sC[j + 1] + a; ccnt[j] = b - a; cmeta[j] = approx_meta(pattern, left - 1, cost);
          if(b > a && cost <= max_mismatches) { keep |= 1u << j; }
        }
        is_hit = (left == 1);
      }
    }
  }
  // both streams in lane order within a wave, wave order within a workgroup, workgroup order through the scan; a lane's children in symbol order
  const u32 wave = threadIdx.x >> 6;
  const bool stands = (!QUAD || q == 0);                                    // this lane stands for its node in the ballots
  const u64 below = (1ull << (QUAD ? (lane_id() & ~3u) : lane_id())) - 1ull;
  u32 wave_next, wave_hits, before_next, before_hits;                       // a lane's kept children all go to one of the two streams
  level_place<5>(is_hit ? 0u : keep, stands, below, &wave_next, &before_next);
  level_place<5>(is_hit ? keep : 0u, stands, below, &wave_hits, &before_hits);
  if(lane_id() == 0) { s_wave[wave][0] = wave_next; s_wave[wave][1] = wave_hits; }
  __syncthreads();
  if(!EMIT) { level_publish<2>(s_wave, totals, nblocks); return; }
  if(keep == 0) { return; }
  const ApproxNodes& out = (is_hit ? hits : next);
  u64 slot = level_slot<2>(s_wave, totals, nblocks, is_hit ? 1u : 0u, wave) + (is_hit ? before_hits : before_next);
  if(is_hit) { slot = hit_base + (slot - totals[nblocks]); }                // the scan ran through both streams; the hit stream continues at hit_base
#pragma unroll
  for(u32 j = 0; j < 5; j++)
  {
    if((keep >> j) & 1u)
    {
      if((!QUAD || (j & 3u) == q) && slot < out.capacity) { nt_store(out.sp + slot, csp[j]); nt_store(out.cnt + slot, ccnt[j]); nt_store(out.meta + slot, cmeta[j]); }
      slot++;
    }
  }
}

// The hits meta[base .. base + nh) of one level: first[p] = the slot of pattern p's first hit, end[p] = one behind its last.  A pattern's
// hits stand next to each other, so the lane whose left neighbour belongs to another pattern writes the one, the lane whose right
// neighbour does the other.  Patterns without hits keep first[p] = end[p] = 0.
__global__ void __launch_bounds__(BLOCK_THREADS) k_approx_mark(const u64* meta, u64 base, u64 nh, u64 nb, u64* first, u64* end)
{
  const u64 t = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(t >= nh) { return; }
  const u64 i = base + t;
  const u64 p = approx_pattern(meta[i]);
  if(p >= nb) { return; }
  if(t == 0 || approx_pattern(meta[i - 1]) != p) { first[p] = i; }
  if(t + 1 == nh || approx_pattern(meta[i + 1]) != p) { end[p] = i + 1; }
}

// kept[p] = min(hits of pattern p, max_hits) (max_hits == 0: all of them) for p < nb, kept[nb] = 0: the input of the scan that gives hit_offsets.
__global__ void __launch_bounds__(BLOCK_THREADS) k_approx_cap(const u64* first, const u64* end, u64 nb, u64 max_hits, u64* kept)
{
  const u64 p = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(p > nb) { return; }
  u64 c = 0;
  if(p < nb && end[p] > first[p]) { c = end[p] - first[p]; }
  if(max_hits > 0 && c > max_hits) { c = max_hits; }
  kept[p] = c;
}

// The kept hits in pattern order: hit i of the stream, the j-th of its pattern, goes to base[p] + j when j < base[p + 1] - base[p].
__global__ void __launch_bounds__(BLOCK_THREADS) k_approx_gather(const u64* hit_sp, const u64* hit_cnt, const u64* hit_meta, u64 total, u64 nb, const u64* first,
  const u64* base, u64* out_sp, u64* out_cnt, u8* out_mismatches, u64 capacity)
{
  const u64 i = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(i >= total) { return; }
  const u64 meta = hit_meta[i];
  const u64 p = approx_pattern(meta);
  if(p >= nb || i < first[p]) { return; }
  const u64 j = i - first[p], b = base[p];
  if(j >= base[p + 1] - b) { return; }
  const u64 slot = b + j;
  if(slot >= capacity) { return; }
  out_sp[slot] = hit_sp[i]; out_cnt[slot] = hit_cnt[i]; out_mismatches[slot] = (u8)(meta & 0xFFu);
}
