/*
  kernels/sequences.hip.h -- sequences of the collection by id: the LF walk from the endmarker back to the start of the sequence, as text.
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm, behind kernels/quad.hip.h whose record reader and walk it uses); gfx950 only.
*/
#pragma once

//------------------------------------------------------------------------------
// Sequence k ends at position k (its endmarker is the k-th suffix), so
//     pos = k; loop { c = BWT[pos]; if c == 0 stop; prepend c; pos = C[c] + rank(pos, c) }
// yields it back to front.  FOUR lanes per sequence, the record reader of kernels/quad.hip.h (QuadRec, quad_load, quad_step): one dependent
// HBM access per step, plus the super row (a few hundred lines, L2 resident).
//
// Two kernels walk every sequence twice: the first stores its length, the host turns the lengths into offsets, the second stores the
// symbols at their final places.  No staging buffer of unknown size per sequence exists: the text of a batch is allocated at its exact
// size between the two launches.
//
// A quad is uniform in control flow (its four lanes hold the same pos, c and step count), and the quad permutes never read across quads:
// quads that have finished, and the idle quads behind `count` in the last wave or workgroup, have left the loop and feed nobody.
// Every walk ends after max_len symbols at the latest and never loads beyond position n - 1, whatever the records hold
// (quad_walk_to_start; k_seq_emit repeats the bounds in its own loop, which stores as it goes).

// The status word of a launch of this family holds the smallest slot that failed (atomicMin), or this value when none did.
constexpr u64 SEQ_STATUS_NONE = ~0ull;

// lengths[j] = symbols of sequence ids[j] (ids == nullptr: first_id + j).  A sequence that is still alive after max_len symbols, an id that
// is no sequence, a position outside the index or a symbol outside the alphabet: status = min(status, j), and nothing is stored for j.
__global__ void __launch_bounds__(BLOCK_THREADS) k_seq_lengths(IndexView x, const u64* ids, u64 first_id, u64 count, u32 max_len, u32* lengths,
  unsigned long long* status)
{
  __shared__ u64 sC[8];
  load_C(sC, x);
  const u32 q = threadIdx.x & 3;
  const u64 j = ((u64)blockIdx.x * BLOCK_THREADS + threadIdx.x) >> 2;
  if(j >= count) { return; }
  u64 pos = (ids ? ids[j] : first_id + j);
  u32 len = 0;
  QuadRec last;
  const bool ok = (pos < x.m) && quad_walk_to_start(x, sC, q, max_len, pos, len, last);
  if(q != 0) { return; }
  if(ok) { lengths[j] = len; }
  else { atomicMin(status, (unsigned long long)j); }
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
  load_C(sC, x);
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
    QuadRec rec;
    quad_load(x, pos, q, rec);
    const u32 c = quad_step(rec, q, sC, pos);
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
