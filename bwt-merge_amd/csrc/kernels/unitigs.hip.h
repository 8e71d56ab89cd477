/*
  kernels/unitigs.hip.h -- the unitigs of the k-mer graph over the solid k-mers of a spectrum (bwtm_unitigs_*): the compacted de Bruijn
  graph with its coverage and links, built on the device.
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm, behind kernels/correct.hip.h whose table it reads); gfx950 only.
*/
#pragma once

//------------------------------------------------------------------------------
// THE RULE (include/bwtm.h states it in full).  The NODES are the S k-mers of count >= threshold, node index = rank in code order: the
// entries of a CorrectTable.  x -> y is an EDGE when the last k - 1 symbols of x are the first k - 1 of y; it is COMPACTABLE when x has
// no other edge out and y no other edge in.  The compactable edges form disjoint paths and disjoint cycles: each is one UNITIG, a cycle
// beginning at its node of smallest code; the unitigs are numbered by the code of their first node, and the edges that are not
// compactable are the LINKS between a unitig's last node and another's first.
//
// k_unitig_links     one lane per node.  The four successors ((x << 2) | r) & mask share their first k - 1 symbols, so they are
//                    neighbours in the table: one lower bound and at most four entries give out(x) and, when it is 1, the one
//                    successor.  The four predecessors (r << 2 (k - 1)) | (x >> 2) are four lookups: in(x).  Five lookups per node.
// k_unitig_next      one lane per node x with one successor y: the edge is compactable when in(y) == 1, which y's lane has written
//                    in the launch before.  Then next[x] = y stays and y is no start: start[y] = 0, written by this lane alone, since
//                    y has no other edge in.  Otherwise next[x] = none.  No atomic decides a link.
// k_unitig_walk      one lane per node; the lane of a START (a node without a compactable edge in) that nobody has visited follows
//                    next[] with one dependent load per step and no lookup, and gives every node of its path (start, offset).  It
//                    leaves the sum of the path's counts in the start's own count.  Time: one memory round trip per node of the
//                    longest unitig; work: one load per node.
// k_unitig_unreached counts the nodes no walk visited.  They all lie on cycles of compactable edges (a path has a start).  Usually
//                    there are none, and the cycle phase is this one reduction.
// k_unitig_cycle_*   otherwise ceil(log2(unreached)) rounds of pointer jumping over the unreached nodes, double buffered:
//                    m'[x] = min(m[x], m[j[x]]), j'[x] = j[j[x]], from m[x] = x, j[x] = next[x].  After r rounds m[x] is the smallest
//                    index among the 2^r nodes from x on: with 2^r >= the cycle's length, the cycle's smallest index.  The node that
//                    equals its minimum becomes a start, and k_unitig_walk runs once more: a walk ends when it returns to its start.
//                    (Walking the cycle from every one of its nodes would take time and work in the square of its length.)
// k_unitig_number    one lane per node, after the exclusive scan of the start flags has numbered the starts in code order: the node's
//                    unitig is its start's number; a start writes the unitig's occurrences; a LAST node (no next, or next == its
//                    start) writes the unitig's node count, flags and text length, and its own index for k_unitig_fill_links.
// k_unitig_text      one lane per node, after the scan of the text lengths: a first node writes its k symbols at the unitig's
//                    offset, node j its last symbol at offset + j + k - 1.
// k_unitig_fill_links one lane per unitig: the successors of its last node, found as in k_unitig_links, give the unitigs they begin.
// k_unitig_place     one lane per queried code: one lookup.
//
// Each node, text byte and link is written by exactly one lane; the three atomics add to the statistics.  Two runs give the same bytes.
//
// No load leaves its buffer, whatever the table holds: bucket bounds are clamped in correct_lower_bound, every index read from next[],
// head[] or the jump arrays is compared with S before it is used, a walk ends after S steps at the latest, and the text is written
// below `symbols` only.

constexpr u64 UNITIG_NONE = ~0ull;
constexpr u32 UNITIG_CIRCULAR = 1;

__device__ inline u64 unitig_mask(u32 k) { return (k == 32 ? ~0ull : (1ull << (2 * k)) - 1ull); }

// The entries [lo, lo + n) that hold successors of x, n <= 4; *base = the successor of rank 0, so that an entry's rank is code - base.
__device__ inline u32 unitig_successors(const CorrectTable& t, u64 x, u64* lo, u64* base)
{
  *base = (x << 2) & unitig_mask(t.k);
  *lo = correct_lower_bound(t, *base);
  u32 n = 0;
  for(u64 e = *lo; e < t.solid && n < 4; e++, n++)
  {
    const u64 c = t.codes[e];
    if(c < *base || c - *base >= 4) { break; }
  }
  return n;
}

// out[slot[i]] = cnt[i] for the k-mers of count >= threshold: the sibling of k_correct_compact for the counts.
__global__ void __launch_bounds__(BLOCK_THREADS) k_unitig_counts(const u64* cnt, const u64* slot, u64 n, u64 threshold, u64* out, u64 solid)
{
  const u64 i = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(i < n && cnt[i] >= threshold)
  {
    const u64 s = slot[i];
    if(s < solid) { out[s] = cnt[i]; }
  }
}

// Nodes [first, end).  next[i] = the one successor or none, deg[i] = out | in << 4, start[i] = 1 (start[S] = 0); stats[0] += lookups.
__global__ void __launch_bounds__(BLOCK_THREADS) k_unitig_links(u64 first, u64 end, CorrectTable t, u64* next, u8* deg, u64* start, unsigned long long* stats)
{
  const u64 i = first + (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  u64 looks = 0;
  if(i < end)
  {
    const u64 x = t.codes[i] & unitig_mask(t.k);                                                  // every code looked up lies below 4^k: its bucket exists
    u64 lo, base;
    const u32 out = unitig_successors(t, x, &lo, &base);
    const u32 shift = 2 * (t.k - 1);                                                              // 0 for k = 1, where x >> 2 is 0
    u32 in = 0;
#pragma unroll
    for(u64 r = 0; r < 4; r++) { in += (correct_index(t, (r << shift) | (x >> 2)) != UNITIG_NONE ? 1u : 0u); }
    looks = 5;
    next[i] = (out == 1 ? lo : UNITIG_NONE);
    deg[i] = (u8)(out | (in << 4));
    start[i] = 1;
    if(i + 1 == t.solid) { start[t.solid] = 0; }
  }
  const u64 wave_looks = wave_sum(looks);
  if(lane_id() == 0 && wave_looks != 0) { atomicAdd(stats, (unsigned long long)wave_looks); }
}

__global__ void __launch_bounds__(BLOCK_THREADS) k_unitig_next(u64 first, u64 end, u64 solid, u64* next, const u8* deg, u64* start)
{
  const u64 i = first + (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(i >= end) { return; }
  const u64 y = next[i];
  if(y < solid && (deg[y] >> 4) == 1) { start[y] = 0; }
  else if(y != UNITIG_NONE) { next[i] = UNITIG_NONE; }
}

// head[] holds UNITIG_NONE for the nodes nobody has visited.  cnt[start] becomes the sum of the counts of the start's path.
__global__ void __launch_bounds__(BLOCK_THREADS) k_unitig_walk(u64 first, u64 end, u64 solid, const u64* next, u64* cnt, const u64* start, u64* head, u64* off)
{
  const u64 i = first + (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(i >= end || start[i] == 0 || head[i] != UNITIG_NONE) { return; }
  u64 cur = i, j = 0, occ = 0;
  do
  {
    head[cur] = i; off[cur] = j; occ += cnt[cur];
    j++;
    cur = next[cur];
  } while(cur < solid && cur != i && j < solid);
  cnt[i] = occ;
}

__global__ void __launch_bounds__(BLOCK_THREADS) k_unitig_unreached(const u64* head, u64 solid, unsigned long long* out)
{
  __shared__ u64 lds[BLOCK_THREADS / WAVE];
  u64 acc = 0;
  for(u64 i = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x; i < solid; i += (u64)gridDim.x * BLOCK_THREADS) { acc += (head[i] == UNITIG_NONE ? 1u : 0u); }
  const u64 total = block_reduce<0>(acc, lds);
  if(threadIdx.x == 0 && total != 0) { atomicAdd(out, (unsigned long long)total); }
}

__global__ void __launch_bounds__(BLOCK_THREADS) k_unitig_cycle_init(u64 first, u64 end, u64 solid, const u64* head, const u64* next, u64* m, u64* j)
{
  const u64 i = first + (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(i >= end || head[i] != UNITIG_NONE) { return; }
  const u64 y = next[i];
  m[i] = i; j[i] = (y < solid ? y : i);
}

__global__ void __launch_bounds__(BLOCK_THREADS) k_unitig_cycle_jump(u64 first, u64 end, u64 solid, const u64* head, const u64* m0, const u64* j0, u64* m1, u64* j1)
{
  const u64 i = first + (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(i >= end || head[i] != UNITIG_NONE) { return; }
  u64 p = j0[i];
  if(p >= solid) { p = i; }
  const u64 a = m0[i], b = m0[p];
  m1[i] = (b < a ? b : a); j1[i] = j0[p];
}

__global__ void __launch_bounds__(BLOCK_THREADS) k_unitig_cycle_starts(u64 first, u64 end, const u64* head, const u64* m, u64* start)
{
  const u64 i = first + (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(i < end && head[i] == UNITIG_NONE && m[i] == i) { start[i] = 1; }
}

// rank = the exclusive scan of the start flags; head[i] turns from the node's start into the node's unitig.  A last node writes
// nodes, flags, last and lens (the text length n + k - 1, into the array whose scan gives the offsets) of its unitig; a start its
// occurrences.  stats[1] = max(stats[1], nodes of a unitig), stats[2] += nodes of circular unitigs.
__global__ void __launch_bounds__(BLOCK_THREADS) k_unitig_number(u64 first, u64 end, u64 solid, u64 unitigs, u32 k, const u64* next, u64* head, const u64* off,
  const u64* cnt, const u64* rank, u64* nodes, u64* occ, u8* flags, u64* last, u64* lens, unsigned long long* stats)
{
  const u64 i = first + (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(i >= end) { return; }
  u64 h = head[i];
  if(h >= solid) { h = i; }
  const u64 u = rank[h];
  head[i] = u;
  if(u >= unitigs) { return; }
  if(h == i) { occ[u] = cnt[i]; }
  const u64 y = next[i];
  if(y >= solid || y == h)
  {
    const u64 n = off[i] + 1;
    const bool circular = (y == h);
    nodes[u] = n; last[u] = i; flags[u] = (u8)(circular ? UNITIG_CIRCULAR : 0u); lens[u] = n + k - 1;
    atomicMax(stats + 1, (unsigned long long)n);
    if(circular) { atomicAdd(stats + 2, (unsigned long long)n); }
  }
}

__global__ void __launch_bounds__(BLOCK_THREADS) k_unitig_text(u64 first, u64 end, u32 k, u32 skip, const u64* codes, const u64* unitig, const u64* off,
  const u64* offsets, u64 unitigs, u8* text, u64 symbols)
{
  const u64 i = first + (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(i >= end) { return; }
  const u64 u = unitig[i];
  if(u >= unitigs) { return; }
  const u64 c = codes[i], j = off[i], at = offsets[u];
  if(j == 0)
  {
    for(u32 q = 0; q < k; q++) { if(at + q < symbols) { text[at + q] = (u8)kmer_comp((u32)(c >> (2 * (k - 1 - q))) & 3u, skip); } }
  }
  else if(at + j + k - 1 < symbols) { text[at + j + k - 1] = (u8)kmer_comp((u32)c & 3u, skip); }
}

// links[4 u + r] = the unitig of the successor of rank r of u's last node, none where that k-mer is no node; a circular unitig has none.
__global__ void __launch_bounds__(BLOCK_THREADS) k_unitig_fill_links(u64 first, u64 end, CorrectTable t, const u64* last, const u8* flags, const u64* unitig, u64* links,
  unsigned long long* stats)
{
  const u64 u = first + (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  u64 looks = 0;
  if(u < end)
  {
    u64 link[4] = {UNITIG_NONE, UNITIG_NONE, UNITIG_NONE, UNITIG_NONE};
    const u64 x = last[u];
    if(x < t.solid && (flags[u] & UNITIG_CIRCULAR) == 0)
    {
      u64 lo, base;
      const u32 n = unitig_successors(t, t.codes[x], &lo, &base);
      looks = 1;
      for(u32 e = 0; e < n; e++)
      {
        const u64 r = t.codes[lo + e] - base, v = unitig[lo + e];
#pragma unroll
        for(u32 q = 0; q < 4; q++) { if(r == q) { link[q] = v; } }                                // no indexed store into registers
      }
    }
#pragma unroll
    for(u32 q = 0; q < 4; q++) { links[4 * u + q] = link[q]; }
  }
  const u64 wave_looks = wave_sum(looks);
  if(lane_id() == 0 && wave_looks != 0) { atomicAdd(stats, (unsigned long long)wave_looks); }
}

// (unitig, offset) of every queried code, none twice for a code that is no node (a code of 4^k or more among them).
__global__ void __launch_bounds__(BLOCK_THREADS) k_unitig_place(CorrectTable t, const u64* unitig, const u64* off, const u64* codes, u64 count, u64* out_unitig, u64* out_offset)
{
  const u64 q = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(q >= count) { return; }
  const u64 c = codes[q];
  const u64 at = (c <= unitig_mask(t.k) ? correct_index(t, c) : UNITIG_NONE);
  out_unitig[q] = (at != UNITIG_NONE ? unitig[at] : UNITIG_NONE);
  out_offset[q] = (at != UNITIG_NONE ? off[at] : UNITIG_NONE);
}
