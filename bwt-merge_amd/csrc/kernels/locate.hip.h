/*
  kernels/locate.hip.h -- from a BWT position back to the collection: the sequence that holds the suffix, and the suffix's offset in it.
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm, behind kernels/quad.hip.h whose record reader and walk it uses); gfx950 only.
*/
#pragma once

//------------------------------------------------------------------------------
// The LF walk from any position p,
//     pos = p; d = 0; loop { c = BWT[pos]; if c == 0 stop; pos = C[c] + rank(pos, c); d++ }
// ends after d steps at pos_end, the suffix that is a whole sequence: d is the offset of p's suffix in that sequence.  WHICH sequence the walk
// cannot say: every endmarker is encoded as 0 and the whole-sequence suffixes sort by content, so LF through the 0 does not land on the
// sequence's number.  k = rank(pos_end, 0) numbers the whole-sequence suffixes in BWT order, and ONE TABLE PER INDEX, start_to_id[k], turns
// that number into the id.  The table comes from the same walk started at pos = j for every sequence j (sequence j ends at position j):
// start_to_id[rank(pos_end, 0)] = j.  A position p < m, the endmarker suffix of sequence p, locates to (p, length of p) with no special case.
//
// The table's entries are u64: 8 bytes per sequence -- 8 GB for 10^9 reads, against about 50 GB of records for 10^11 bases of such reads.
//
// Four lanes per walk and the walk of k_seq_lengths itself (quad_walk_to_start, kernels/quad.hip.h), so the same bounds: a walk ends after
// max_len steps at the latest and never loads beyond position n - 1, whatever the records hold; a walk still alive after max_len steps, a
// position >= n or a symbol outside 0..5 sets status = min(status, j) and stores nothing for j.  rank(pos_end, 0) is below n on any
// records but below m only on sound ones: it is checked against m before it addresses the table.

constexpr u64 LOCATE_UNSET = ~0ull;          // the table's fill value before the build (a pool block is not zero)

// The walk from pos to the start of its sequence: false when it is no walk of a sound index within max_len steps.  On success pos is
// pos_end, d the number of steps, and k = rank(pos_end, 0) < m, taken from the record the walk ended in.  Quad-uniform.
__device__ inline bool locate_walk(const IndexView& x, const u64* sC, u32 q, u32 max_len, u64& pos, u32& d, u64& k)
{
  QuadRec last;
  if(!quad_walk_to_start(x, sC, q, max_len, pos, d, last)) { return false; }
  k = quad_rank_zero(last, q, pos);
  return k < x.m;
}

// table[rank(pos_end, 0)] = id for the sequences first .. first + count - 1.  Distinct sequences of a sound index end at distinct
// whole-sequence suffixes: plain stores.
__global__ void __launch_bounds__(BLOCK_THREADS) k_locate_build(IndexView x, u64 first, u64 count, u32 max_len, u64* table, unsigned long long* status)
{
  __shared__ u64 sC[8];
  load_C(sC, x);
  const u32 q = threadIdx.x & 3;
  const u64 j = ((u64)blockIdx.x * BLOCK_THREADS + threadIdx.x) >> 2;
  if(j >= count) { return; }
  const u64 id = first + j;
  u64 pos = id, k = 0;
  u32 d = 0;
  const bool ok = (id < x.m) && locate_walk(x, sC, q, max_len, pos, d, k);
  if(q != 0) { return; }
  if(ok) { table[k] = id; }
  else { atomicMin(status, (unsigned long long)j); }
}

// Entries of the table that no sequence claimed (still the fill value) or that are no sequence: 0 after the build of a sound index.
__global__ void __launch_bounds__(BLOCK_THREADS) k_locate_check(const u64* table, u64 m, unsigned long long* bad)
{
  u64 mine = 0;
  for(u64 k = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x; k < m; k += (u64)gridDim.x * BLOCK_THREADS) { mine += (table[k] >= m ? 1 : 0); }
  const u64 total = wave_sum(mine);
  if(lane_id() == 0 && total != 0) { atomicAdd(bad, (unsigned long long)total); }
}

// Hit slot h of a batch: its position is positions[h], or, with ranges (positions == nullptr), range_start[r] + (h - range_first_hit[r])
// for the last range r of the batch's `nranges` with range_first_hit[r] <= h (range_first_hit[0] == 0, ascending; the ranges of a batch
// hold at least one hit each).  ids[h] = table[rank(pos_end, 0)], offs[h] = steps.  Neighbouring slots of one range start in the same
// record: the first loads of a wave coalesce.  A table entry that is no sequence counts as damage, like a walk that does not end.
__global__ void __launch_bounds__(BLOCK_THREADS) k_locate(IndexView x, const u64* table, const u64* positions, const u64* range_start,
  const u64* range_first_hit, u64 nranges, u64 count, u32 max_len, u64* ids, u64* offs, unsigned long long* status)
{
  __shared__ u64 sC[8];
  load_C(sC, x);
  const u32 q = threadIdx.x & 3;
  const u64 h = ((u64)blockIdx.x * BLOCK_THREADS + threadIdx.x) >> 2;
  if(h >= count) { return; }
  u64 pos;
  if(positions) { pos = positions[h]; }
  else
  {
    const u64 r = last_at_or_below(range_first_hit, nranges, h);
    pos = range_start[r] + (h - range_first_hit[r]);
  }
  u64 k = 0, id = 0;
  u32 d = 0;
  bool ok = locate_walk(x, sC, q, max_len, pos, d, k);
  if(ok) { id = table[k]; ok = (id < x.m); }
  if(q != 0) { return; }
  if(ok) { ids[h] = id; offs[h] = d; }
  else { atomicMin(status, (unsigned long long)h); }
}
