/*
  kernels/sequences.hip.h -- sequences of the collection by id: the LF walk from the endmarker back to the start of the sequence, as text.
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm, behind kernels/search_walk.hip.h whose quad helpers it uses); gfx950 only.
*/
#pragma once

//------------------------------------------------------------------------------
// Sequence k ends at position k (its endmarker is the k-th suffix), so
//     pos = k; loop { c = BWT[pos]; if c == 0 stop; prepend c; pos = C[c] + rank(pos, c) }
// yields it back to front.  FOUR lanes per sequence, as in k_lf_walk_quad: lane q of a quad loads chunk q of the record with one dwordx4,
// the symbol at pos comes out of the same chunk, every lane counts in its own 32 positions and a quad-wide DPP butterfly adds the pieces
// and the super-table entry.  One dependent HBM access per step, plus the super row (a few hundred lines, L2 resident).
//
// Two kernels walk every sequence twice: the first stores its length, the host turns the lengths into offsets, the second stores the
// symbols at their final places.  No staging buffer of unknown size per sequence exists: the text of a batch is allocated at its exact
// size between the two launches.
//
// A quad is uniform in control flow (its four lanes hold the same pos, c and step count), and the quad permutes never read across quads:
// quads that have finished, and the idle quads behind `count` in the last wave or workgroup, have left the loop and feed nobody.
// Every walk ends after max_len symbols at the latest and never loads beyond position n - 1, whatever the records hold.

constexpr u64 SEQ_STATUS_NONE = ~0ull;

// Chunk q of the record of pos and the lane's super-table entries (symbol q + 1, and N), all requested together.  The empty asm pins the
// values here: left alone, the compiler sinks the header word and the super-table loads behind the test of the symbol, which makes them a
// second round trip that depends on the first.
__device__ inline void seq_load(const IndexView& x, u64 pos, u32 q, uint4& ch, u64& s_q, u64& s_5)
{
  ch = x.recs[4 * (pos >> REC_SHIFT) + q];
  const u64* s = x.sup + (pos >> SUPER_SHIFT) * SUP_STRIDE;
  s_q = s[1 + q]; s_5 = s[5];
  asm volatile("" : "+v"(ch.x), "+v"(ch.y), "+v"(ch.z), "+v"(ch.w), "+v"(s_q), "+v"(s_5));
}

// BWT[pos] and, when it is a symbol 1..5, LF(pos) from chunk q of the record of pos (`ch`) and the super-table entries the lane loaded.
__device__ inline u32 seq_step(uint4 ch, u64 s_q, u64 s_5, u32 q, const u64* sC, u64& pos)
{
  const u32 jp = (u32)(pos & (REC_POS - 1)), t = jp & 31;
  const u32 mine = ((ch.x >> t) & 1u) | (((ch.y >> t) & 1u) << 1) | (((ch.z >> t) & 1u) << 2);
  const u32 c = quad_or_u32((jp >> 5) == q ? mine : 0u);
  if(c == 0 || c > 5) { return c; }                                       // quad-uniform
  const u64 part = (u64)quad_rank_part(ch, q, c, jp) + (c == q + 1 ? s_q : 0) + ((q == 0 && c == 5) ? s_5 : 0);
  pos = sC[c] + quad_sum_u64(part);
  return c;
}

// lengths[j] = symbols of sequence ids[j] (ids == nullptr: first_id + j).  A sequence that is still alive after max_len symbols, an id that
// is no sequence, a position outside the index or a symbol outside the alphabet: status = min(status, j), and nothing is stored for j.
__global__ void __launch_bounds__(BLOCK_THREADS) k_seq_lengths(IndexView x, const u64* ids, u64 first_id, u64 count, u32 max_len, u32* lengths,
  unsigned long long* status)
{
  __shared__ u64 sC[8];
  if(threadIdx.x < 8) { sC[threadIdx.x] = x.C[threadIdx.x]; }
  __syncthreads();
  const u32 q = threadIdx.x & 3;
  const u64 j = ((u64)blockIdx.x * BLOCK_THREADS + threadIdx.x) >> 2;
  if(j >= count) { return; }
  u64 pos = (ids ? ids[j] : first_id + j);
  bool bad = (pos >= x.m);
  u32 len = 0;
  while(!bad)
  {
    if(pos >= x.n) { bad = true; break; }
    uint4 ch; u64 s_q, s_5;
    seq_load(x, pos, q, ch, s_q, s_5);
    const u32 c = seq_step(ch, s_q, s_5, q, sC, pos);
    if(c == 0) { break; }
    if(c > 5 || len == max_len) { bad = true; break; }
    len++;
  }
  if(q != 0) { return; }
  if(bad) { atomicMin(status, (unsigned long long)j); }
  else { lengths[j] = len; }
}

// The second walk: symbol t from the end of sequence j goes to text[offsets[j] + lengths[j] - 1 - t].  Lane 0 of the quad gathers the symbols
// of one 8-byte-aligned word of the text in a register; a word that lies wholly inside the sequence's slot leaves as one 8-byte store, the
// bytes of the first and the last partial word as single bytes -- never a read-modify-write: the other bytes of such a word belong to the
// quad of the neighbouring sequence.  `text` is 8-byte aligned.  The walk takes exactly lengths[j] steps (what k_seq_lengths counted on the
// same records), so every store falls into the slot.
__global__ void __launch_bounds__(BLOCK_THREADS) k_seq_emit(IndexView x, const u64* ids, u64 first_id, u64 count, const u64* offsets, const u32* lengths,
  u8* text)
{
  __shared__ u64 sC[8];
  if(threadIdx.x < 8) { sC[threadIdx.x] = x.C[threadIdx.x]; }
  __syncthreads();
  const u32 q = threadIdx.x & 3;
  const u64 j = ((u64)blockIdx.x * BLOCK_THREADS + threadIdx.x) >> 2;
  if(j >= count) { return; }
  u64 pos = (ids ? ids[j] : first_id + j);
  const u32 len = lengths[j];
  const u64 end = offsets[j] + len;
  u64 at = end, word = 0;
  for(u32 t = 0; t < len; t++)
  {
    if(pos >= x.n) { break; }
    uint4 ch; u64 s_q, s_5;
    seq_load(x, pos, q, ch, s_q, s_5);
    const u32 c = seq_step(ch, s_q, s_5, q, sC, pos);
    if(c == 0 || c > 5) { break; }
    at--;
    word |= (u64)c << (8 * (u32)(at & 7));
    if((at & 7) == 0 || t + 1 == len)
    {
      // `word` holds the bytes [at, top) of the text: a whole aligned word, or the part of one at either end of the slot
      const u64 top = ((at | 7) + 1 < end ? (at | 7) + 1 : end);
      if(q == 0)
      {
        if(top - at == 8) { *(u64*)(text + at) = word; }
        else
        {
#pragma clang loop vectorize(disable) interleave(disable)
          for(u64 b = at; b < top; b++) { text[b] = (u8)(word >> (8 * (u32)(b & 7))); }      // single bytes: no wider store may form here
        }
      }
      word = 0;
    }
  }
}
