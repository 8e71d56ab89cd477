/*
  kernels/stream.hip.h -- the samples of one PIECE of a streamed merge (api/stream.hip.h): the result leaves the device slice by slice, and
  a block's sample needs the start of the block behind it, so the samples trail the bytes by one block.
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm); gfx950 only.

  The ENTRIES of a piece, in block order: [the block that was still open when the slice before ended (six numbers carried on the device)]
  + the slice's own blocks (block_start, and cum32 as the encoder wrote it or the u64 counts of the rank-query form) + [on the final
  piece: the position behind the last block, bases, with the symbol totals].  An entry is (start position, occurrences of 1..5 before it),
  absolute.  Sample k of the piece is the difference of entries k + 1 and k; the last entry becomes the next piece's carry.  No record is read.
*/
#pragma once

struct PieceSrc
{
  const u64* block_start;   // the slice's own blocks
  const u32* cum32;         // [5][nb], relative to the super block of the block's start (null: `cum` answers)
  const u64* cum;           // [6][nb] absolute (k_block_cum_slice)
  const u64* sup;           // super table of the whole result
  const u64* carry;         // six numbers of the open block (read when has_carry)
  u64 nb;
  u32 has_carry, has_tail;
  u64 tail[6];              // (bases, totals of 1..5, unused)
};

__device__ inline void piece_entry(const PieceSrc& s, u64 j, u64 e[6])
{
  if(s.has_carry)
  {
    if(j == 0)
    {
#pragma unroll
      for(int c = 0; c < 6; c++) { e[c] = s.carry[c]; }
      return;
    }
    j--;
  }
  if(j >= s.nb)                                       // only asked for when has_tail
  {
#pragma unroll
    for(int c = 0; c < 6; c++) { e[c] = s.tail[c]; }
    return;
  }
  const u64 p = s.block_start[j];
  e[0] = p;
  if(s.cum32)
  {
    const u64* row = s.sup + (p >> SUPER_SHIFT) * SUP_STRIDE;
#pragma unroll
    for(u32 c = 1; c < 6; c++) { e[c] = row[c] + s.cum32[(u64)(c - 1) * s.nb + j]; }
  }
  else
  {
#pragma unroll
    for(u32 c = 1; c < 6; c++) { e[c] = s.cum[(u64)c * s.nb + j]; }
  }
}

// Samples [0, ns) of a piece whose first sample is the global block g0 (ns = entries - 1).
//   T = u8 / u16 / u32: the compact form of bwtm_index_download_samples_compact -- fields[6][ns] (positions of the block, its occurrences of
//     1..5), and for every global block that is a multiple of 64 its entry in anchors[6][nanch] (anchor_first = index of the piece's first one);
//   T = u64: the full form -- `fields` receives cum[6][ns] (row 0: the start minus the five) and `anchors` block_end[ns].
// carry_out (another buffer than s.carry) receives the last entry unless the piece is the final one; out_max the longest block (one atomic per wave).
template<class T>
__global__ void __launch_bounds__(BLOCK_THREADS) k_piece_fields(PieceSrc s, u64 ns, u64 g0, T* fields, u64* anchors, u64 anchor_first, u64 nanch,
  u64* carry_out, unsigned long long* out_max)
{
  const u64 j = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  u64 len = 0;
  if(j < ns)
  {
    u64 e0[6], e1[6];
    piece_entry(s, j, e0); piece_entry(s, j + 1, e1);
    len = e1[0] - e0[0];
    if(sizeof(T) == 8)
    {
      u64 sum = 0;
#pragma unroll
      for(int c = 1; c < 6; c++) { fields[(u64)c * ns + j] = (T)e0[c]; sum += e0[c]; }
      fields[j] = (T)(e0[0] - sum);
      anchors[j] = e1[0] - 1;
    }
    else
    {
#pragma unroll
      for(int c = 0; c < 6; c++) { fields[(u64)c * ns + j] = (T)(e1[c] - e0[c]); }
      if(((g0 + j) & 63) == 0)
      {
        const u64 k = ((g0 + j) >> 6) - anchor_first;
        if(k < nanch)
        {
#pragma unroll
          for(int c = 0; c < 6; c++) { anchors[(u64)c * nanch + k] = e0[c]; }
        }
      }
    }
  }
  if(j == 0 && !s.has_tail && s.has_carry + s.nb > 0)
  {
    u64 e[6]; piece_entry(s, s.has_carry + s.nb - 1, e);
#pragma unroll
    for(int c = 0; c < 6; c++) { carry_out[c] = e[c]; }
  }
  const u64 m = wave_max(len);
  if(lane_id() == 0 && m > 0) { atomicMax(out_max, (unsigned long long)m); }
}

// A few words for the host, stored into page-locked host memory by a kernel.  The streamed merge reads a slice's last head, size table and
// end offset this way: a small D2H COPY on the compute stream queues behind the slice-sized copy that is in flight on the copy stream
// (they share the copy engines), which serialized every slice's device work with the download of the slice before.
__global__ void __launch_bounds__(WAVE) k_store_host(const u64* src, u64* host_dst, u32 count)
{
  const u32 k = blockIdx.x * WAVE + threadIdx.x;
  if(k < count) { host_dst[k] = src[k]; }
}
