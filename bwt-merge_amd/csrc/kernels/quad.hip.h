/*
  kernels/quad.hip.h -- four lanes per LF walk: the record reader and the walk that the per-chain queries share (k_seq_*, k_locate*,
  k_overlap_*, k_ms_scan), on the quad primitives of kernels/search_walk.hip.h (dpp_quad, quad_sum_u64, quad_or_u32, quad_rank_part; the layout of
  a quad is described there).
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm, behind kernels/search_walk.hip.h); gfx950 only.
*/
#pragma once

//------------------------------------------------------------------------------
// The record reader.  What lane q of a quad holds of the record of one position: chunk q and the lane's super-table entries (symbol
// q + 1, and N).  The functions below take the position again: the record does not remember it (the overlap search reads rank(n, .) next
// to the record of n - 1).  A quad is uniform in control flow, and the quad permutes never read across quads.
struct QuadRec
{
  uint4 ch;              // {plane0, plane1, plane2, header word} of chunk q
  u64 s_q, s_5;          // super-table entries of symbol q + 1 and of N
};

// Chunk q of the record of pos and the lane's two super-table entries, all requested together.  The empty asm pins the values here: left
// alone, the compiler sinks the header word and the super-table loads behind the test of the symbol, which makes them a second round
// trip that depends on the first.
__device__ inline void quad_load(const IndexView& x, u64 pos, u32 q, QuadRec& rec)
{
  rec.ch = x.recs[4 * (pos >> REC_SHIFT) + q];
  const u64* s = x.sup + (pos >> SUPER_SHIFT) * SUP_STRIDE;
  rec.s_q = s[1 + q]; rec.s_5 = s[5];
  asm volatile("" : "+v"(rec.ch.x), "+v"(rec.ch.y), "+v"(rec.ch.z), "+v"(rec.ch.w), "+v"(rec.s_q), "+v"(rec.s_5));
}

// Two records at once.  Both chunks are requested before either record's super-table entries: the chunks are the HBM round trips, and
// with the second one queued behind the first record's super-table addresses k_overlap_scan ran 10 % slower (profiles/walk_family_ab.txt).
// All twelve values are pinned together: the one-record quad_load twice would hold the first record's values before the second record
// is requested.
__device__ inline void quad_load(const IndexView& x, u64 pa, u64 pb, u32 q, QuadRec& a, QuadRec& b)
{
  a.ch = x.recs[4 * (pa >> REC_SHIFT) + q];
  b.ch = x.recs[4 * (pb >> REC_SHIFT) + q];
  const u64* sa = x.sup + (pa >> SUPER_SHIFT) * SUP_STRIDE;
  const u64* sb = x.sup + (pb >> SUPER_SHIFT) * SUP_STRIDE;
  a.s_q = sa[1 + q]; a.s_5 = sa[5];
  b.s_q = sb[1 + q]; b.s_5 = sb[5];
  asm volatile("" : "+v"(a.ch.x), "+v"(a.ch.y), "+v"(a.ch.z), "+v"(a.ch.w), "+v"(a.s_q), "+v"(a.s_5),
                    "+v"(b.ch.x), "+v"(b.ch.y), "+v"(b.ch.z), "+v"(b.ch.w), "+v"(b.s_q), "+v"(b.s_5));
}

// BWT[pos]: held by the lane whose 32 positions contain pos.
__device__ inline u32 quad_symbol(const QuadRec& rec, u32 q, u64 pos)
{
  const u32 jp = (u32)(pos & (REC_POS - 1)), t = jp & 31;
  const u32 mine = ((rec.ch.x >> t) & 1u) | (((rec.ch.y >> t) & 1u) << 1) | (((rec.ch.z >> t) & 1u) << 2);
  return quad_or_u32((jp >> 5) == q ? mine : 0u);
}

// rank(pos, c) for c in 1..5.
__device__ inline u64 quad_rank(const QuadRec& rec, u32 q, u32 c, u64 pos)
{
  const u32 jp = (u32)(pos & (REC_POS - 1));
  const u64 part = (u64)quad_rank_part(rec.ch, q, c, jp) + (c == q + 1 ? rec.s_q : 0) + ((q == 0 && c == 5) ? rec.s_5 : 0);
  return quad_sum_u64(part);
}

// rank(pos, 0) = pos - (the counts of 1..5 before pos): every lane adds the five counts of its 32 positions, its slices of the five
// header fields and its super-table entries.
__device__ inline u64 quad_rank_zero(const QuadRec& rec, u32 q, u64 pos)
{
  const u32 jp = (u32)(pos & (REC_POS - 1));
  u64 part = rec.s_q + (q == 0 ? rec.s_5 : 0);
#pragma unroll
  for(u32 c = 1; c < 6; c++) { part += quad_rank_part(rec.ch, q, c, jp); }
  return pos - quad_sum_u64(part);
}

// BWT[pos] and, when it is a symbol 1..5, pos = LF(pos).  sC = C of the index.
__device__ inline u32 quad_step(const QuadRec& rec, u32 q, const u64* sC, u64& pos)
{
  const u32 c = quad_symbol(rec, q, pos);
  if(c == 0 || c > 5) { return c; }                                       // quad-uniform
  pos = sC[c] + quad_rank(rec, q, c, pos);
  return c;
}

// The walk from pos back to the start of its sequence: false when it is no walk of a sound index within max_len steps.  Every walk ends
// after max_len steps at the latest and never loads beyond position n - 1, whatever the records hold: a position >= n, a symbol outside
// 0..5 or a walk still alive after max_len steps fails.  On success pos is the position that holds the endmarker, `steps` the number of
// symbols before it and `last` the record of pos.  Quad-uniform.
__device__ inline bool quad_walk_to_start(const IndexView& x, const u64* sC, u32 q, u32 max_len, u64& pos, u32& steps, QuadRec& last)
{
  steps = 0;
  while(true)
  {
    if(pos >= x.n) { return false; }
    quad_load(x, pos, q, last);
    const u32 c = quad_step(last, q, sC, pos);
    if(c == 0) { return true; }
    if(c > 5 || steps == max_len) { return false; }
    steps++;
  }
}

// sC[0 .. 8) = C of the index, for the whole workgroup (every thread of it calls this).
__device__ inline void load_C(u64* sC, const IndexView& x)
{
  if(threadIdx.x < 8) { sC[threadIdx.x] = x.C[threadIdx.x]; }
  __syncthreads();
}

// The last k < n with first[k] <= h, for first[0] <= h and first[] never decreasing (n >= 1).
__device__ inline u64 last_at_or_below(const u64* first, u64 n, u64 h)
{
  u64 lo = 0, hi = n;                                            // first[lo] <= h < first[hi]
  while(hi - lo > 1)
  {
    const u64 mid = lo + (hi - lo) / 2;
    if(first[mid] <= h) { lo = mid; } else { hi = mid; }
  }
  return lo;
}
