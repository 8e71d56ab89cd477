/*
  kernels/mem.hip.h -- matching statistics and maximal exact matches of patterns: which pieces of a pattern occur at all, and how long.
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm, behind kernels/quad.hip.h whose record reader it uses); gfx950 only.
*/
#pragma once

//------------------------------------------------------------------------------
// For a pattern P of m symbols and an end e in 1..m, l(e) is the largest l <= e for which P[e-l .. e) occurs (0: P[e-1] alone does not).
// The backward search from P[e-1] leftwards holds, after l symbols, the range of P[e-l .. e): the last range that is not empty is the one
// of l(e).  One TASK per (pattern, end), that is per symbol of the batch's text, FOUR lanes per task on the record reader of
// kernels/quad.hip.h, the search of k_overlap_scan (kernels/overlap.hip.h): the range is [sp, e1), the records of sp and e1 are requested
// together, rank(n, .) comes from C, and nothing beyond position n - 1 is loaded.  A quad is uniform in control flow.  Adjacent tasks are
// adjacent ends of one pattern, and l(e + 1) <= l(e) + 1: the 16 tasks of a wave run nearly equally long.
//
// A maximal exact match (b, l) -- P[b .. b+l) occurs, and neither P[b-1 .. b+l) nor P[b .. b+l+1) does (or it does not exist) -- ends at
// e = b + l with l = l(e), which makes it maximal on the left, and it is maximal on the right iff no match that ends at e + 1 contains
// it: end e gives a MEM iff l(e) >= 1 and (e == m or l(e + 1) <= l(e)).  (l(e + 1) <= l(e) + 1 always: a match that ends at e + 1,
// without its last symbol, is one that ends at e.)  k_mem_flag applies that rule to the l array of the batch.  It needs no pattern
// boundary: the first end of the next pattern has l <= 1 <= l(e), which flags e as e == m would.

// Symbol t of the batch's text, t < total: task t.  Pattern k = text[offsets[k] .. offsets[k + 1]), offsets[0] == 0, offsets[count] == total;
// the task's pattern is the last k < count with offsets[k] <= t (empty patterns share their offset with the next one that is not).
// Stores (l, sp, count) of the task's end, (0, 0, 0) when its symbol does not occur; any of the three arrays may be null.  `steps` += the
// LF steps taken, one per symbol the search consumed (the first from the whole range, without a load; every other one two-record load):
// l(e) when the search stops at the pattern's begin, one more when it stops at an empty range.  One atomic per workgroup.
__global__ void __launch_bounds__(BLOCK_THREADS) k_ms_scan(IndexView x, const u8* text, const u64* offsets, u64 count, u64 total,
  u32* out_len, u64* out_sp, u64* out_cnt, unsigned long long* steps)
{
  __shared__ u64 sC[8];
  __shared__ unsigned int s_steps;
  if(threadIdx.x == 0) { s_steps = 0; }
  load_C(sC, x);
  const u32 q = threadIdx.x & 3;
  const u64 t = ((u64)blockIdx.x * BLOCK_THREADS + threadIdx.x) >> 2;
  u32 taken = 0;
  if(t < total)
  {
    const u64 begin = offsets[last_at_or_below(offsets, count, t)];
    u64 pos = t;
    u32 len = 1, best = 0;
    u64 best_sp = 0, best_cnt = 0;
    const u32 c0 = text[pos];
    u64 sp = 0, e1 = 0;                                                     // the range as [sp, e1)
    if(c0 >= 1 && c0 <= 5) { sp = sC[c0]; e1 = sC[c0 + 1]; taken = 1; }        // the step from the whole range: both ranks are C's
    while(sp < e1 && e1 <= x.n)                                             // quad-uniform; sp <= n - 1
    {
      best = len; best_sp = sp; best_cnt = e1 - sp;
      if(pos == begin) { break; }
      const u32 c = text[pos - 1];
      if(c < 1 || c > 5) { break; }
      const bool at_end = (e1 == x.n);
      QuadRec ra, rb;
      quad_load(x, sp, (at_end ? e1 - 1 : e1), q, ra, rb);
      sp = sC[c] + quad_rank(ra, q, c, sp);
      e1 = sC[c] + (at_end ? sC[c + 1] - sC[c] : quad_rank(rb, q, c, e1));
      pos--; len++; taken++;
    }
    if(q == 0)
    {
      if(out_len) { out_len[t] = best; }
      if(out_sp) { out_sp[t] = best_sp; }
      if(out_cnt) { out_cnt[t] = best_cnt; }
    }
  }
  if(q == 0 && taken > 0) { atomicAdd(&s_steps, taken); }                   // at most 64 tasks of 65 536 steps: fits 32 bits
  __syncthreads();
  if(threadIdx.x == 0 && s_steps > 0) { atomicAdd(steps, (unsigned long long)s_steps); }
}

// The MEMs of a pattern with one QUAD per PATTERN: the form bwtm_mem_batch ships (tools/mem_bench.py decided).
// The ends go from m downwards, each searched backwards as k_ms_scan does.  `bound` is the begin of the last search (it starts behind
// every position): an end gives a MEM iff its search gets below `bound` -- the rule above, stated on begins: l(e + 1) <= l(e) iff
// e - l(e) < e + 1 - l(e + 1) -- and the pattern is finished as soon as a search reaches its begin: every end below lies inside that
// match.  That skips the searches of k_ms_scan that a MEM does not need (all but one when the whole pattern occurs), but a pattern's
// ends are searched one after the other; k_ms_scan + k_mem_flag is the A/B partner (bwtm_tune("mem_kernel", 1) of a diagnostics build).
// Stores flags[t] for every symbol of its pattern (and flags[total] = 0), (l, sp, count) of the flagged ends only, per_pattern[k] = the
// pattern's MEMs of at least min_length symbols (and per_pattern[count] = 0): what the two scans and k_mem_emit read.  `steps` and
// `found` as in k_ms_scan and k_mem_flag.
__global__ void __launch_bounds__(BLOCK_THREADS) k_mem_pattern(IndexView x, const u8* text, const u64* offsets, u64 count, u64 total, u32 min_length,
  u32* out_len, u64* out_sp, u64* out_cnt, u64* flags, u64* per_pattern, unsigned long long* steps, unsigned long long* found)
{
  __shared__ u64 sC[8];
  __shared__ unsigned long long s_steps;
  __shared__ unsigned int s_found;
  if(threadIdx.x == 0) { s_steps = 0; s_found = 0; }
  load_C(sC, x);
  const u32 q = threadIdx.x & 3;
  const u64 k = ((u64)blockIdx.x * BLOCK_THREADS + threadIdx.x) >> 2;
  u64 taken = 0;
  u32 any = 0;
  if(k < count)
  {
    const u64 begin = offsets[k], end = offsets[k + 1];
    u64 bound = end + 1, kept = 0, e = end;
    for(; e > begin; e--)
    {
      u64 pos = e - 1;
      u32 len = 1, best = 0;
      u64 best_sp = 0, best_cnt = 0;
      const u32 c0 = text[pos];
      u64 sp = 0, e1 = 0;
      if(c0 >= 1 && c0 <= 5) { sp = sC[c0]; e1 = sC[c0 + 1]; taken++; }
      while(sp < e1 && e1 <= x.n)                                           // quad-uniform; sp <= n - 1
      {
        best = len; best_sp = sp; best_cnt = e1 - sp;
        if(pos == begin) { break; }
        const u32 c = text[pos - 1];
        if(c < 1 || c > 5) { break; }
        const bool at_end = (e1 == x.n);
        QuadRec ra, rb;
        quad_load(x, sp, (at_end ? e1 - 1 : e1), q, ra, rb);
        sp = sC[c] + quad_rank(ra, q, c, sp);
        e1 = sC[c] + (at_end ? sC[c + 1] - sC[c] : quad_rank(rb, q, c, e1));
        pos--; len++; taken++;
      }
      const u64 b = e - best;                                               // where the match of this end begins
      const bool mem = (best >= 1 && b < bound);
      const bool keep = (mem && best >= min_length);
      if(q == 0)
      {
        flags[e - 1] = (keep ? 1 : 0);
        if(keep) { out_len[e - 1] = best; out_sp[e - 1] = best_sp; out_cnt[e - 1] = best_cnt; }
      }
      any += (mem ? 1 : 0); kept += (keep ? 1 : 0);
      bound = b;
      if(best >= 1 && b == begin) { e--; break; }
    }
    for(u64 t = begin + q; t < e; t += 4) { flags[t] = 0; }                 // the ends inside the match that reaches the pattern's begin
    if(q == 0)
    {
      per_pattern[k] = kept;
      if(k + 1 == count) { per_pattern[count] = 0; flags[total] = 0; }
    }
  }
  if(q == 0 && taken > 0) { atomicAdd(&s_steps, (unsigned long long)taken); }
  if(q == 0 && any > 0) { atomicAdd(&s_found, any); }
  __syncthreads();
  if(threadIdx.x == 0)
  {
    if(s_steps > 0) { atomicAdd(steps, s_steps); }
    if(s_found > 0) { atomicAdd(found, (unsigned long long)s_found); }
  }
}

// flags[t] = 1 when end t + 1 of its pattern gives a MEM of at least min_length symbols, else 0, for t < total, and flags[total] = 0: the
// generic scan turns flags[0 .. total] in place into the MEM's slot.  Every flagged end adds one to per_pattern[k] of its pattern
// (zeroed by the caller; count + 1 entries, the last stays 0 and becomes the total of their scan).  found[0] += the ends that give a MEM of
// any length.  Reads only the l array and the offsets.  With k_ms_scan it is the other form of the MEM search, the A/B partner of
// k_mem_pattern: compiled into every build (tests/test_isa_mem.py holds it to no scratch), launched by a diagnostics build only.
__global__ void __launch_bounds__(BLOCK_THREADS) k_mem_flag(const u32* len, const u64* offsets, u64 count, u64 total, u32 min_length,
  u64* flags, u64* per_pattern, unsigned long long* found)
{
  __shared__ unsigned int s_found;
  if(threadIdx.x == 0) { s_found = 0; }
  __syncthreads();
  const u64 t = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(t <= total)
  {
    bool mem = false, kept = false;
    if(t < total)
    {
      const u32 l = len[t];
      mem = (l >= 1 && (t + 1 == total || len[t + 1] <= l));
      kept = (mem && l >= min_length);
    }
    flags[t] = (kept ? 1 : 0);
    if(kept) { atomicAdd((unsigned long long*)&per_pattern[last_at_or_below(offsets, count, t)], 1ull); }
    if(mem) { atomicAdd(&s_found, 1u); }
  }
  __syncthreads();
  if(threadIdx.x == 0 && s_found > 0) { atomicAdd(found, (unsigned long long)s_found); }
}

// slots[0 .. total] = the scanned flags: end t + 1 gives the MEM of slot slots[t] iff slots[t + 1] > slots[t].  Its begin within its
// pattern, its length and its range go to the four arrays (any of them null), which hold `capacity` = slots[total] entries.
__global__ void __launch_bounds__(BLOCK_THREADS) k_mem_emit(const u32* len, const u64* sp, const u64* cnt, const u64* offsets, u64 count, u64 total,
  const u64* slots, u64 capacity, u32* out_begin, u32* out_length, u64* out_sp, u64* out_count)
{
  const u64 t = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(t >= total) { return; }
  const u64 slot = slots[t];
  if(slots[t + 1] <= slot || slot >= capacity) { return; }
  const u32 l = len[t];
  const u64 begin = offsets[last_at_or_below(offsets, count, t)];
  if(out_begin) { out_begin[slot] = (u32)(t + 1 - l - begin); }
  if(out_length) { out_length[slot] = l; }
  if(out_sp) { out_sp[slot] = sp[t]; }
  if(out_count) { out_count[slot] = cnt[t]; }
}
