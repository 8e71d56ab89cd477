/*
  kernels/edit.hip.h -- patterns within edit distance e (insertions, deletions, substitutions): the frontier search of kernels/approx.hip.h
  whose node carries a band of the edit-distance matrix instead of one mismatch counter, so that its hits appear over several levels.
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm, behind kernels/approx.hip.h whose streams it uses); gfx950 only.
*/
#pragma once

//------------------------------------------------------------------------------
// A NODE is (sp, count, pattern, band): the BWT range [sp, sp + count) of the suffixes that start with a string W, the pattern's number
// within the batch, and the column D_W[i] = ed(W, the last i symbols of the pattern P) around i = t, where t = |W| is the DEPTH: the
// level's number, the same for every node of a frontier and therefore a kernel argument.  The band is 15 fields of 4 bits in one word,
// field f for i = t + f - 7, every field saturated at 8 (a value beyond every budget); a field whose i is below 0 or above m = |P| holds 8.
// An entry of the matrix that is <= e <= 7 lies within |i - t| <= e, and so does a cheapest path to it: what the 15 fields lose is above
// every budget anyway, and e appears only in the two comparisons below.  The frontier starts as one root (0, n, k, D[i] = i) per pattern.
//
// One level, for every node with t < m + e and every comp value c = 1..5 (an endmarker never extends a match): the range of cW as in
// kernels/approx.hip.h, and the column
//     D_cW[i] = min(D_W[i - 1] + (c != P[m - i]), D_W[i] + 1, D_cW[i - 1] + 1),  D_cW[0] = t + 1
// whose field g stands under the parent's fields g (the diagonal) and g + 1.  A child with a non-empty range is
//     KEPT for the next frontier   when the minimum of its column is <= e and t + 1 < m + e (a node at depth m + e has no viable child;
//                                  the minimum never decreases with depth, so nothing is lost), and
//     A HIT                        when D_cW[m] <= e: (sp, count, (pattern, length t + 1, edits D_cW[m])) goes to the hit stream.
// The two are independent: a child can be both.  A root with m <= e is a hit itself, the empty string (0, n, (k, 0, m)), and is expanded
// as well.  Both streams take the children in parent order, then symbol order, the root's own hit before its children's: the frontier
// stays grouped by pattern and, within a pattern, ascending when the strings are compared from their last symbol backwards; the hits
// of one pattern and one length stand next to each other in the stream, in that order.
//
// A level is the count pass, the scan and the expand pass of kernels/level.hip.h with k_approx_level's two streams, the next frontier and
// the hits; here a lane may bring children to both.  One lane per node, 256 nodes per workgroup.
// No load leaves the index or the batch's text, whatever the nodes hold: sp and sp + count are clamped to n first, a node with count == 0
// loads nothing, rank(0, .) and rank(n, .) are not loads (level_lane_ranks), a pattern number beyond the batch expands nothing, every index
// into the text is clamped into it before the load.  Every store is checked against the capacity the host allocated from the read-back.
// There is no loop whose length depends on data.

constexpr u32 EDIT_MAX_EDITS = 7;
constexpr u32 EDIT_FIELDS = 15;                   // |i - t| <= 7
constexpr u32 EDIT_SAT = 8;
constexpr u32 EDIT_SLOTS = 2 * EDIT_MAX_EDITS + 1;

// A hit's meta word: the pattern (bits 32..63), the length of the matched string (bits 8..31: up to 65 535 + 7), its distance (bits 0..7).
__host__ __device__ inline u64 edit_hit_meta(u64 pattern, u64 length, u64 edits) { return (pattern << 32) | ((length & 0xFFFFFFu) << 8) | (edits & 0xFFu); }
__host__ __device__ inline u64 edit_hit_pattern(u64 meta) { return meta >> 32; }
__host__ __device__ inline u64 edit_hit_length(u64 meta) { return (meta >> 8) & 0xFFFFFFu; }

// Four arrays of `capacity` entries: a frontier.
struct EditNodes
{
  u64* sp; u64* cnt; u64* pattern; u64* band; u64 capacity;
};

// The length of pattern p of the batch, at most APPROX_MAX_LEN (the host has refused a longer one).
__device__ inline u64 edit_pattern_length(const u64* offsets, u64 p)
{
  const u64 begin = offsets[p], end = offsets[p + 1];
  const u64 len = (end > begin ? end - begin : 0);
  return (len > APPROX_MAX_LEN ? APPROX_MAX_LEN : len);
}

// One root per pattern of the batch: out[k] = (0, n, k, D[i] = i for 0 <= i <= min(|P_k|, 7)), k < nb <= out.capacity.
__global__ void __launch_bounds__(BLOCK_THREADS) k_edit_roots(const u64* offsets, u64 nb, u64 n, EditNodes out)
{
  const u64 k = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(k >= nb || k >= out.capacity) { return; }
  const u64 m = edit_pattern_length(offsets, k);
  u64 band = 0;
#pragma unroll
  for(u32 f = 0; f < EDIT_FIELDS; f++)
  {
    const u64 v = (f >= 7 && (u64)(f - 7) <= m ? f - 7 : EDIT_SAT);
    band |= v << (4 * f);
  }
  out.sp[k] = 0; out.cnt[k] = n; out.pattern[k] = k; out.band[k] = band;
}

// EMIT == false: totals[blockIdx.x] and totals[nblocks + blockIdx.x] = this workgroup's children for the next frontier and its hits.
// EMIT == true:  totals as the exclusive scan left them; the kept children go to next.*[..] and the hits to hits.*[hit_base + ..], never
//                at or beyond either capacity.
// text[0 .. text_bytes) and offsets[0 .. nb] are the batch's patterns, t the depth of the frontier `in`, count its nodes, nblocks = gridDim.x.
template<bool EMIT>
__global__ void __launch_bounds__(BLOCK_THREADS) k_edit_level(IndexView x, const u8* text, u64 text_bytes, const u64* offsets, u64 nb, u32 max_edits, u64 t,
  const u64* in_sp, const u64* in_cnt, const u64* in_pattern, const u64* in_band, u64 count, u64 nblocks, u64* totals, EditNodes next, ApproxNodes hits, u64 hit_base)
{
  __shared__ u64 sC[8];
  __shared__ u32 s_wave[BLOCK_THREADS / WAVE][2];
  load_C(sC, x);
  const u64 k = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  u64 csp[5] = {0, 0, 0, 0, 0}, ccnt[5] = {0, 0, 0, 0, 0}, cband[5] = {0, 0, 0, 0, 0};
  u32 cedits = 0;                                                           // 4 bits per child: D_cW[m]
  u32 keep = 0;                                                             // bit j: the child of comp value j + 1 goes to the next frontier
  u32 hit = 0;                                                              // bit 0: this root is a hit itself; bit j + 1: the child of comp value j + 1 is one
  u64 pattern = 0, m = 0, sp = 0, cnt = 0;
  if(k < count)
  {
    sp = in_sp[k]; cnt = in_cnt[k];
    pattern = in_pattern[k];
    const u64 old = in_band[k];
    if(sp > x.n) { sp = x.n; }
    if(cnt > x.n - sp) { cnt = x.n - sp; }
    if(pattern < nb)
    {
      m = edit_pattern_length(offsets, pattern);
      if(t == 0 && m <= max_edits) { hit = 1; }
      if(cnt > 0 && t < m + max_edits)
      {
        // the child's field g stands for i = t + g - 6; the pattern's symbol of that row, where the row exists, as 3 bits of `syms`
        const long long i0 = (long long)t - 6;
        const u64 last = offsets[pattern] + m;                              // one behind the pattern's text
        u64 syms = 0;
#pragma unroll
        for(u32 g = 0; g < EDIT_FIELDS; g++)
        {
          const long long i = i0 + (long long)g;
          if(i >= 1 && (u64)i <= m && text_bytes > 0)
          {
            u64 at = last - (u64)i;
            if(at >= text_bytes) { at = text_bytes - 1; }
            syms |= (u64)(text[at] & 7u) << (3 * g);
          }
        }
        u64 rs[6], re[6];
        level_lane_ranks(x, sC, sp, sp + cnt, rs, re);
        const u32 top = (u32)(t + 1 < EDIT_SAT ? t + 1 : EDIT_SAT);         // D_cW[0]
#pragma unroll
        for(u32 j = 0; j < 5; j++)
        {
          u64 band = 0;
          u32 prev = EDIT_SAT, least = EDIT_SAT, at_m = EDIT_SAT;
#pragma unroll
          for(u32 g = 0; g < EDIT_FIELDS; g++)
          {
            const long long i = i0 + (long long)g;
            const u32 diag = (u32)(old >> (4 * g)) & 15u;
            const u32 up = (g + 1 < EDIT_FIELDS ? (u32)(old >> (4 * (g + 1))) & 15u : EDIT_SAT);
            const u32 want = (u32)(syms >> (3 * g)) & 7u;
            u32 v = min(min(diag + (j + 1 != want ? 1u : 0u), up + 1u), prev + 1u);
            if(i == 0) { v = top; }
            if(i < 0 || (u64)i > m) { v = EDIT_SAT; }
            v = min(v, EDIT_SAT);
            prev = v; least = min(least, v);
            if(i >= 0 && (u64)i == m) { at_m = v; }
            band |= (u64)v << (4 * g);
          }
          const u64 a = rs[j + 1], b = re[j + 1];
          csp[j] = sC[j + 1] + a; ccnt[j] = b - a; cband[j] = band;
          cedits |= at_m << (4 * j);
          if(b > a)
          {
            if(least <= max_edits && t + 1 < m + max_edits) { keep |= 1u << j; }
            if(at_m <= max_edits) { hit |= 2u << j; }
          }
        }
      }
    }
  }
  // both streams in lane order within a wave, wave order within a workgroup, workgroup order through the scan; a lane's children in symbol order
  const u32 wave = threadIdx.x >> 6;
  const u64 below = (1ull << lane_id()) - 1ull;
  u32 wave_next, wave_hits, before_next, before_hits;
  level_place<5>(keep, true, below, &wave_next, &before_next);
  level_place<6>(hit, true, below, &wave_hits, &before_hits);
  if(lane_id() == 0) { s_wave[wave][0] = wave_next; s_wave[wave][1] = wave_hits; }
  __syncthreads();
  if(!EMIT) { level_publish<2>(s_wave, totals, nblocks); return; }
  if(keep == 0 && hit == 0) { return; }
  u64 slot = level_slot<2>(s_wave, totals, nblocks, 0, wave) + before_next;
  u64 hslot = hit_base + (level_slot<2>(s_wave, totals, nblocks, 1, wave) - totals[nblocks]) + before_hits;
  if(hit & 1u)
  {
    if(hslot < hits.capacity) { nt_store(hits.sp + hslot, sp); nt_store(hits.cnt + hslot, cnt); nt_store(hits.meta + hslot, edit_hit_meta(pattern, 0, m)); }
    hslot++;
  }
#pragma unroll
  for(u32 j = 0; j < 5; j++)
  {
    if((keep >> j) & 1u)
    {
      if(slot < next.capacity) { nt_store(next.sp + slot, csp[j]); nt_store(next.cnt + slot, ccnt[j]); nt_store(next.pattern + slot, pattern); nt_store(next.band + slot, cband[j]); }
      slot++;
    }
    if((hit >> (j + 1)) & 1u)
    {
      if(hslot < hits.capacity)
      {
        nt_store(hits.sp + hslot, csp[j]); nt_store(hits.cnt + hslot, ccnt[j]); nt_store(hits.meta + hslot, edit_hit_meta(pattern, t + 1, (cedits >> (4 * j)) & 15u));
      }
      hslot++;
    }
  }
}

// The length slot of a hit of pattern p: its length - (m - e), 0 .. 2 e; anything else (a node that is not the search's) is EDIT_SLOTS.
__device__ inline u32 edit_slot(const u64* offsets, u64 p, u64 meta, u32 max_edits)
{
  const u64 s = edit_hit_length(meta) + max_edits - edit_pattern_length(offsets, p);      // wraps below 0
  return (s <= 2ull * max_edits && s < EDIT_SLOTS ? (u32)s : EDIT_SLOTS);
}

// The hits meta[base .. base + nh) of one level: first[s nb + p] = the position of the first hit of pattern p in length slot s, end[s nb + p]
// = one behind its last.  The hits of one pattern and one length stand next to each other, so the lane whose left neighbour has another
// pattern or length writes the one, the lane whose right neighbour has the other.  Slots without hits keep first = end = 0.
__global__ void __launch_bounds__(BLOCK_THREADS) k_edit_mark(const u64* meta, u64 base, u64 nh, const u64* offsets, u64 nb, u32 max_edits, u64* first, u64* end)
{
  const u64 t = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(t >= nh) { return; }
  const u64 i = base + t;
  const u64 key = meta[i] >> 8;                                             // (pattern, length)
  const u64 p = edit_hit_pattern(meta[i]);
  if(p >= nb) { return; }
  const u32 s = edit_slot(offsets, p, meta[i], max_edits);
  if(s >= EDIT_SLOTS) { return; }
  if(t == 0 || (meta[i - 1] >> 8) != key) { first[(u64)s * nb + p] = i; }
  if(t + 1 == nh || (meta[i + 1] >> 8) != key) { end[(u64)s * nb + p] = i + 1; }
}

// kept[p] = min(hits of pattern p over its length slots, max_hits) (max_hits == 0: all of them) for p < nb, kept[nb] = 0: the input of
// the scan that gives hit_offsets.
__global__ void __launch_bounds__(BLOCK_THREADS) k_edit_cap(const u64* first, const u64* end, u64 nb, u32 max_edits, u64 max_hits, u64* kept)
{
  const u64 p = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(p > nb) { return; }
  u64 c = 0;
  if(p < nb)
  {
#pragma unroll
    for(u32 s = 0; s < EDIT_SLOTS; s++)
    {
      if(s <= 2 * max_edits) { const u64 a = first[(u64)s * nb + p], b = end[(u64)s * nb + p]; c += (b > a ? b - a : 0); }
    }
  }
  if(max_hits > 0 && c > max_hits) { c = max_hits; }
  kept[p] = c;
}

// The kept hits in pattern order, shortest first: hit i of the stream, the j-th of its pattern and length slot, goes to base[p] + the
// sizes of the pattern's earlier slots + j when that is below base[p + 1].
__global__ void __launch_bounds__(BLOCK_THREADS) k_edit_gather(const u64* hit_sp, const u64* hit_cnt, const u64* hit_meta, u64 total, const u64* offsets, u64 nb, u32 max_edits,
  const u64* first, const u64* end, const u64* base, u64* out_sp, u64* out_cnt, u32* out_lengths, u8* out_edits, u64 capacity)
{
  const u64 i = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(i >= total) { return; }
  const u64 meta = hit_meta[i];
  const u64 p = edit_hit_pattern(meta);
  if(p >= nb) { return; }
  const u32 mine = edit_slot(offsets, p, meta, max_edits);
  if(mine >= EDIT_SLOTS || i < first[(u64)mine * nb + p]) { return; }
  u64 j = i - first[(u64)mine * nb + p];
#pragma unroll
  for(u32 s = 0; s < EDIT_SLOTS; s++)
  {
    if(s < mine) { const u64 a = first[(u64)s * nb + p], b = end[(u64)s * nb + p]; j += (b > a ? b - a : 0); }
  }
  const u64 b = base[p];
  if(j >= base[p + 1] - b) { return; }
  const u64 slot = b + j;
  if(slot >= capacity) { return; }
  out_sp[slot] = hit_sp[i]; out_cnt[slot] = hit_cnt[i]; out_lengths[slot] = (u32)edit_hit_length(meta); out_edits[slot] = (u8)(meta & 0xFFu);
}
