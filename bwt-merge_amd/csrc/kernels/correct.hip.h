/*
  kernels/correct.hip.h -- k-mer error correction of reads against the solid k-mers of a spectrum (bwtm_corrector_*, bwtm_correct_*).
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm, behind kernels/kmers.hip.h whose codes it reads); gfx950 only.
*/
#pragma once

//------------------------------------------------------------------------------
// THE TABLE.  The codes of the k-mers of count >= threshold, ascending (they are a subsequence of the k-mer handle's codes, which are
// sorted), and a DIRECTORY over the top D of their 2 k used bits: dir[b] = the first entry whose bucket (code >> (2 k - D)) is at least b,
// dir[2^D] = S, the number of entries.  A lookup is two neighbouring directory loads and a binary search inside [dir[b], dir[b + 1]),
// which holds one or two entries on average: D = min(2 k, 24, max(1, ceil(log2 S))) (correct_dir_bits), so that there are at most about
// two buckets per entry, the directory is at most 128 MiB, and 2 k - D is a shift of 0 .. 63 (k = 32 uses all 64 bits of a code).
//
// THE RULE (include/bwtm.h states it in full).  A window of k symbols is SOLID when it holds no `skip` symbol and its code is in the
// table; a position is COVERED when a solid window contains it.  Round by round, the leftmost uncovered position i that has EXACTLY ONE
// kept symbol c != W[i] which makes the window at max(0, i - k + 1) solid -- or, failing that, the window at min(i, m - k) -- takes
// that symbol.  A read whose positions are all covered ends CLEAN or CORRECTED; one that runs out of rounds or has no such position
// FAILED, and its text is restored.
//
// k_correct_wave: one wave per read, four reads per workgroup, the working text in global memory (a read may be 2^24 symbols long;
// nothing of it is staged in LDS).  A round walks the read in chunks of 64 positions.  Every lane loads the symbols of two positions,
// base + lane and base + 64 + lane; six ballots turn them into the two bit planes of the symbols' ranks and a plane of the symbols that
// are no k-mer symbol (skip, and everything behind the read's end), as wave-uniform 128-bit words.  Lane l's window starts at base + l:
// its k bits of each plane are one funnel shift away, its code is the bit reversal and the interleave of the two (no memory, no loop over
// k), and its lookup is the only load.  The solid windows come back as one ballot; a position is uncovered when the last solid window at
// or before it starts more than k - 1 positions earlier, which every lane decides from the ballot and the carry of the chunks before.
// The uncovered positions of a chunk are taken in ascending order, wave-uniformly; the up to eight candidate windows of one position
// (two windows, four symbols) are built and looked up by eight lanes at once, each from the working text itself, since its window may
// begin before the chunk.  A substitution ends the round.
//
// What a round does not look at again.  When the substituted position i was the leftmost uncovered one, every position before i was
// covered, and the windows that start before i - k + 1 do not hold i: the positions before P = i - k + 1 stay covered whatever later
// rounds substitute at or behind P... as long as no uncovered position is skipped.  So the next round starts its windows at P - k + 1
// and judges the positions from P on (a later substitution at i' >= P moves P to i' - k + 1, which may be smaller: positions in between
// were covered in the round that found i').  When an uncovered position without a unique candidate lies before i, the next round starts
// at 0 again: it is the rule's text either way.
//
// No atomic decides anything: the three atomics of a wave add to the statistics of the call.  Two runs give the same bytes.
//
// No load leaves the buffers, whatever the table holds: a bucket's bounds are clamped to S before the search, the symbols are loaded
// only below the read's end, and the text of read r is offsets[r] .. offsets[r + 1], which the host has checked (or produced).

constexpr u32 CORRECT_CLEAN = 0, CORRECT_CORRECTED = 1, CORRECT_FAILED = 2, CORRECT_SHORT = 3;
constexpr u32 CORRECT_MAX_DIR_BITS = 24;
constexpr u32 CORRECT_WAVES = BLOCK_THREADS / WAVE;        // reads per workgroup of k_correct_wave

// D of the header: min(2 k, 24, max(1, ceil(log2 solid))).
__host__ __device__ inline u32 correct_dir_bits(u32 k, u64 solid)
{
  u32 lg = 0;
  while(lg < 63 && (1ull << lg) < solid) { lg++; }
  u32 d = (lg < 1 ? 1u : lg);
  if(d > 2 * k) { d = 2 * k; }
  return (d > CORRECT_MAX_DIR_BITS ? CORRECT_MAX_DIR_BITS : d);
}

struct CorrectTable
{
  const u64* codes;      // solid entries, ascending
  const u64* dir;        // 2^dir_bits + 1 entries
  u64 solid;
  u32 k, skip, dir_bits;
};

// The rank 0..3 of a kept comp value among the four (the inverse of kmer_comp); c != skip.
__device__ inline u32 correct_rank(u32 c, u32 skip) { return c - 1u - (c > skip ? 1u : 0u); }

__device__ inline bool correct_lookup(const CorrectTable& t, u64 code)
{
  const u64 b = code >> (2 * t.k - t.dir_bits);
  u64 lo = t.dir[b], hi = t.dir[b + 1];
  if(hi > t.solid) { hi = t.solid; }
  if(lo > hi) { lo = hi; }
  const u64 end = hi;
  while(lo < hi)
  {
    const u64 mid = lo + ((hi - lo) >> 1);
    if(t.codes[mid] < code) { lo = mid + 1; } else { hi = mid; }
  }
  return lo < end && t.codes[lo] == code;
}

// The index of the first entry >= code, t.solid when there is none (kernels/unitigs.hip.h).  The search stays inside the bucket of
// `code`, clamped as above; when the bucket holds no such entry the answer is its end, dir[b + 1], which is the first entry of the later
// buckets: the bucket's lower bound is the table's.  code must lie below 4^k, so that its bucket exists.
__device__ inline u64 correct_lower_bound(const CorrectTable& t, u64 code)
{
  const u64 b = code >> (2 * t.k - t.dir_bits);
  u64 lo = t.dir[b], hi = t.dir[b + 1];
  if(hi > t.solid) { hi = t.solid; }
  if(lo > hi) { lo = hi; }
  while(lo < hi)
  {
    const u64 mid = lo + ((hi - lo) >> 1);
    if(t.codes[mid] < code) { lo = mid + 1; } else { hi = mid; }
  }
  return lo;
}

// correct_lookup that says where: the index of the entry that holds `code`, ~0 when none does.
__device__ inline u64 correct_index(const CorrectTable& t, u64 code)
{
  const u64 at = correct_lower_bound(t, code);
  return (at < t.solid && t.codes[at] == code ? at : ~0ull);
}

// flags[i] = (cnt[i] >= threshold) for i < n, flags[n] = 0: the exclusive scan of the n + 1 flags gives every kept code its slot and,
// in its last entry, the number of solid k-mers.
__global__ void __launch_bounds__(BLOCK_THREADS) k_correct_flag(const u64* cnt, u64 n, u64 threshold, u64* flags)
{
  const u64 i = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(i <= n) { flags[i] = (i < n && cnt[i] >= threshold ? 1ull : 0ull); }
}

// out[slot[i]] = code[i] for the k-mers of count >= threshold; nothing at or beyond `solid`.
__global__ void __launch_bounds__(BLOCK_THREADS) k_correct_compact(const u64* code, const u64* cnt, const u64* slot, u64 n, u64 threshold, u64* out, u64 solid)
{
  const u64 i = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(i < n && cnt[i] >= threshold)
  {
    const u64 s = slot[i];
    if(s < solid) { out[s] = code[i]; }
  }
}

// One thread per entry e and one more, e == solid, that closes the directory off: an entry whose bucket differs from its predecessor's
// (the first entry's predecessor has bucket -1) writes dir[b] = e for every bucket b in (previous bucket, own bucket]; the last thread
// writes dir[b] = solid for every b behind the last entry's bucket, up to 2^dir_bits.  With solid == 0 that thread writes all of it.
__global__ void __launch_bounds__(BLOCK_THREADS) k_correct_dir(const u64* codes, u64 solid, u32 shift, u64 buckets, u64* dir)
{
  const u64 e = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(e > solid) { return; }
  u64 first = (e == 0 ? 0 : (codes[e - 1] >> shift) + 1);                 // the first bucket this thread may write
  u64 last = (e == solid ? buckets : codes[e] >> shift);                  // the last one
  if(last > buckets) { last = buckets; }
  for(u64 b = first; b <= last; b++) { dir[b] = e; }
}

// A 32-bit word spread over the even bits of 64.
__device__ inline u64 correct_spread(u64 v)
{
  v &= 0xFFFFFFFFull;
  v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
  v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
  v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
  v = (v | (v << 2)) & 0x3333333333333333ull;
  v = (v | (v << 1)) & 0x5555555555555555ull;
  return v;
}

// Bits lane .. lane + 63 of the 128-bit word (hi : lo).
__device__ inline u64 correct_funnel(u64 lo, u64 hi, u32 lane) { return (lane == 0 ? lo : (lo >> lane) | (hi << (64 - lane))); }

// stats[0] += table lookups, stats[1] += rounds, stats[2] = max(stats[2], edits of one read).
__global__ void __launch_bounds__(BLOCK_THREADS) k_correct_wave(CorrectTable t, const u8* in, u8* work, const u64* offsets, u64 count, u32 max_rounds,
  u8* status, u32* edits, unsigned long long* stats)
{
  const u64 read = ((u64)blockIdx.x * BLOCK_THREADS + threadIdx.x) >> 6;                       // wave-uniform
  if(read >= count) { return; }
  const u32 lane = lane_id();
  const u32 k = t.k, skip = t.skip;
  const u64 beg = offsets[read], m = offsets[read + 1] - beg;
  const u8* src = in + beg;
  u8* w = work + beg;
  for(u64 p = lane; p < m; p += WAVE) { w[p] = src[p]; }
  __threadfence_block();                                                                      // the lanes read each other's symbols
  u32 st = CORRECT_SHORT, rounds = 0, ed = 0;
  u64 looks = 0;
  if(m >= k)
  {
    const u64 nwin = m - k + 1;
    const u64 kmask = (1ull << k) - 1ull;                                                     // k <= 32
    u64 from = 0;                                                                             // P of the header: the positions before it are covered
    for(;;)
    {
      bool counted = false, stuck = false, fixed = false, uncovered_any = false, out_of_rounds = false;
      long long last = -(1ll << 40);                                                          // start of the last solid window so far
      for(u64 base = (from >= k - 1 ? from - (k - 1) : 0); base < m && !fixed && !out_of_rounds; base += WAVE)
      {
        const u64 p0 = base + lane, p1 = p0 + WAVE;
        const u32 s0 = (p0 < m ? w[p0] : 0u), s1 = (p1 < m ? w[p1] : 0u);
        const bool v0 = (s0 >= 1 && s0 <= 5 && s0 != skip), v1 = (s1 >= 1 && s1 <= 5 && s1 != skip);
        const u32 r0 = (v0 ? correct_rank(s0, skip) : 0u), r1 = (v1 ? correct_rank(s1, skip) : 0u);
        const u64 lo0 = __ballot(r0 & 1u), lo1 = __ballot(r1 & 1u), hi0 = __ballot(r0 & 2u), hi1 = __ballot(r1 & 2u);
        const u64 no0 = __ballot(!v0), no1 = __ballot(!v1);
        bool solid = false;
        if(p0 < nwin && (correct_funnel(no0, no1, lane) & kmask) == 0)
        {
          // bit j of a plane's window = symbol j; the code wants symbol j at bits 2 (k - 1 - j): reverse the k bits, then interleave
          const u64 wl = __brevll(correct_funnel(lo0, lo1, lane) & kmask) >> (64 - k);
          const u64 wh = __brevll(correct_funnel(hi0, hi1, lane) & kmask) >> (64 - k);
          solid = correct_lookup(t, correct_spread(wl) | (correct_spread(wh) << 1));
          looks++;
        }
        const u64 sol = __ballot(solid);
        const u64 upto = sol & ((2ull << lane) - 1ull);                                        // the solid windows at base .. base + lane
        const long long mine = (upto != 0 ? (long long)(base + 63u - (u32)__builtin_clzll(upto)) : last);
        u64 unc = __ballot(p0 < m && p0 >= from && (long long)p0 - mine >= (long long)k);
        if(sol != 0) { last = (long long)(base + 63u - (u32)__builtin_clzll(sol)); }
        while(unc != 0)                                                                       // wave-uniform
        {
          uncovered_any = true;
          if(!counted)
          {
            if(rounds == max_rounds) { out_of_rounds = true; break; }
            rounds++; counted = true;
          }
          const u64 i = base + (u32)__builtin_ctzll(unc);
          unc &= unc - 1;
          // lanes 0..3: the window at max(0, i - k + 1) with the four kept symbols at i; lanes 4..7: the one at min(i, m - k), when it is another
          const u64 o0 = (i >= k - 1 ? i - (k - 1) : 0), o1 = (i < nwin ? i : nwin - 1);
          const u32 c = kmer_comp(lane & 3u, skip);
          const u64 o = (lane < 4 ? o0 : o1);
          bool found = false;
          if(lane < 8 && (lane < 4 || o1 != o0) && w[i] != c)
          {
            u64 code = 0; bool kept = true;
            for(u32 q = 0; q < k; q++)
            {
              const u32 s = (o + q == i ? c : (u32)w[o + q]);
              if(s < 1 || s > 5 || s == skip) { kept = false; }
              code = (code << 2) | (u64)(kept ? correct_rank(s, skip) : 0u);
            }
            if(kept) { found = correct_lookup(t, code); looks++; }
          }
          const u32 cand = (u32)(__ballot(found) & 0xFFull);
          u32 pick = 0;                                                                       // the one candidate, as a bit of cand, or none
          if(__popc(cand & 0xFu) == 1) { pick = cand & 0xFu; }
          else if(o1 != o0 && __popc(cand >> 4) == 1) { pick = cand >> 4; }
          if(pick != 0)
          {
            if(lane == 0) { w[i] = (u8)kmer_comp((u32)__builtin_ctz(pick), skip); }
            __threadfence_block();                                                            // the next round loads it
            ed++; fixed = true;
            from = (stuck || i < k - 1 ? 0 : i - (k - 1));
            break;
          }
          stuck = true;
        }
      }
      if(fixed) { continue; }
      st = (uncovered_any || out_of_rounds ? CORRECT_FAILED : (ed != 0 ? CORRECT_CORRECTED : CORRECT_CLEAN));
      break;
    }
    if(st == CORRECT_FAILED)                                                                  // nothing of a partial correction leaves the call
    {
      if(ed != 0) { for(u64 p = lane; p < m; p += WAVE) { w[p] = src[p]; } }
      ed = 0;
    }
  }
  const u64 wave_looks = wave_sum(looks);
  if(lane == 0)
  {
    status[read] = (u8)st; edits[read] = ed;
    if(wave_looks != 0) { atomicAdd(stats, (unsigned long long)wave_looks); }
    if(rounds != 0) { atomicAdd(stats + 1, (unsigned long long)rounds); }
    if(ed != 0) { atomicMax(stats + 2, (unsigned long long)ed); }
  }
}

#ifdef BWTM_DIAGNOSTICS
// The A/B partner of k_correct_wave (bwtm_tune("correct_kernel", 1), tools/correct_bench.py): one LANE per read, k_find_batch's shape.
// The same rule and the same restart point; the windows' codes roll from one position to the next, the position that starts the
// window just completed is judged (the last window completes the read's last k positions), and the candidates of an uncovered
// position are tried one after the other.  The same bytes and the same rounds; fewer lookups, since a round ends at the substituted
// position and not at the end of its chunk of 64 windows.
__global__ void __launch_bounds__(BLOCK_THREADS) k_correct_lane(CorrectTable t, const u8* in, u8* work, const u64* offsets, u64 count, u32 max_rounds,
  u8* status, u32* edits, unsigned long long* stats)
{
  const u64 read = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  const bool active = (read < count);
  const u32 k = t.k, skip = t.skip;
  u32 st = CORRECT_SHORT, rounds = 0, ed = 0;
  u64 looks = 0;
  if(active)
  {
    const u64 beg = offsets[read], m = offsets[read + 1] - beg;
    const u8* src = in + beg;
    u8* w = work + beg;
    for(u64 p = 0; p < m; p++) { w[p] = src[p]; }
    if(m >= k)
    {
      const u64 nwin = m - k + 1;
      const u64 cmask = (k == 32 ? ~0ull : (1ull << (2 * k)) - 1ull);
      u64 from = 0;
      for(;;)
      {
        bool counted = false, stuck = false, fixed = false, uncovered_any = false, out_of_rounds = false;
        long long last = -(1ll << 40);
        const u64 start = (from >= k - 1 ? from - (k - 1) : 0);
        u64 code = 0; u32 run = 0;
        for(u64 p = start; p < m && !fixed && !out_of_rounds; p++)
        {
          const u32 s = w[p];
          if(s >= 1 && s <= 5 && s != skip) { code = ((code << 2) | correct_rank(s, skip)) & cmask; if(run < k) { run++; } }
          else { code = 0; run = 0; }
          if(p + 1 < start + k) { continue; }
          const u64 o = p + 1 - k;                                                             // the window that ends at p
          if(run >= k) { looks++; if(correct_lookup(t, code)) { last = (long long)o; } }
          const u64 judged_end = (o + 1 == nwin ? m : o + 1);                                   // behind the last window: the rest of the read
          for(u64 i = (o > from ? o : from); i < judged_end && !fixed && !out_of_rounds; i++)
          {
            if((long long)i - last < (long long)k) { continue; }
            uncovered_any = true;
            if(!counted)
            {
              if(rounds == max_rounds) { out_of_rounds = true; break; }
              rounds++; counted = true;
            }
            const u64 o0 = (i >= k - 1 ? i - (k - 1) : 0), o1 = (i < nwin ? i : nwin - 1);
            for(u32 which = 0; which < 2 && !fixed; which++)
            {
              if(which == 1 && o1 == o0) { break; }
              const u64 ow = (which == 0 ? o0 : o1);
              u32 ncand = 0, pick = 0;
              for(u32 j = 0; j < 4; j++)
              {
                const u32 c = kmer_comp(j, skip);
                if(w[i] == c) { continue; }
                u64 wcode = 0; bool kept = true;
                for(u32 q = 0; q < k; q++)
                {
                  const u32 sq = (ow + q == i ? c : (u32)w[ow + q]);
                  if(sq < 1 || sq > 5 || sq == skip) { kept = false; }
                  wcode = (wcode << 2) | (u64)(kept ? correct_rank(sq, skip) : 0u);
                }
                if(kept) { looks++; if(correct_lookup(t, wcode)) { ncand++; pick = c; } }
              }
              if(ncand == 1)
              {
                w[i] = (u8)pick; ed++; fixed = true;
                from = (stuck || i < k - 1 ? 0 : i - (k - 1));
              }
            }
            if(!fixed) { stuck = true; }
          }
        }
        if(fixed) { continue; }
        st = (uncovered_any || out_of_rounds ? CORRECT_FAILED : (ed != 0 ? CORRECT_CORRECTED : CORRECT_CLEAN));
        break;
      }
      if(st == CORRECT_FAILED)
      {
        if(ed != 0) { for(u64 p = 0; p < m; p++) { w[p] = src[p]; } }
        ed = 0;
      }
    }
    status[read] = (u8)st; edits[read] = ed;
  }
  const u64 wave_looks = wave_sum(looks), wave_rounds = wave_sum(rounds), wave_edits = wave_max(ed);
  if(lane_id() == 0)
  {
    if(wave_looks != 0) { atomicAdd(stats, (unsigned long long)wave_looks); }
    if(wave_rounds != 0) { atomicAdd(stats + 1, (unsigned long long)wave_rounds); }
    if(wave_edits != 0) { atomicMax(stats + 2, (unsigned long long)wave_edits); }
  }
}
#endif
