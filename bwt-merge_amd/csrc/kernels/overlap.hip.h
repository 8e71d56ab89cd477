/*
  kernels/overlap.hip.h -- suffix-prefix overlaps: for a query Q, the sequences whose prefix equals a suffix of Q.
  Part of bwtm_kernels.hip.h (included there, inside namespace bwtm, behind kernels/locate.hip.h whose table it uses); gfx950 only.
*/
#pragma once

//------------------------------------------------------------------------------
// The backward search of Q from its last symbol holds, after l symbols, the range [sp, ep] of the suffixes that start with Q[L-l..L).  The
// suffixes of that range that are WHOLE sequences are the ones preceded by an endmarker, and LF maps them, in order, onto the endmarker
// suffixes z0 .. z1 - 1 with
//     z0 = rank(sp, 0),  z1 = rank(ep + 1, 0):
// the same numbering of the whole-sequence suffixes in BWT order that the locator's table start_to_id is indexed by (kernels/locate.hip.h).
// So the hits of length l are table[z] for z in [z0, z1), in ascending BWT position of the target, and no walk is needed at all: one
// backward search per query -- the two rank positions of every step serve both the next LF step and the interval -- plus table look-ups.
//
// FOUR lanes per query, the record reader of kernels/quad.hip.h twice per step: the records of sp AND of ep + 1 are requested together and
// pinned together (the two-record quad_load), and both ranks of either come from those registers.  A quad is uniform in
// control flow (its lanes hold the same sp, ep, symbol and length); quads that have finished, and the idle quads behind `count`, have
// left the loop and feed nobody.  The search never loads beyond position n - 1: rank(n, .) is taken from C.
//
// The search finds the lengths ascending, the output wants them descending (longest overlap first).  Two passes over the same text: the
// COUNT pass stores, per query, the number of non-empty intervals and of hits (both before max_hits) and the hits kept; two scans on the
// device turn them into the first record and the first hit slot of every query; the EMIT pass repeats the search and, with T hits in all
// and `seen` hits found so far, gives an interval of cnt hits the slots [T - seen - cnt, T - seen) of its query, and the i-th interval
// found the record nint - 1 - i: a query's records lie in slot order.  Of the slots only those below kept = min(T, max_hits) exist: a record's count is what is left of
// it below the cut (possibly 0), its first slot is clamped to the cut, so first slots never decrease through the batch and the LAST record
// with first <= h is the one that holds hit h.

struct OverlapRecs
{
  u64* first;      // first hit slot of the interval, numbered through the batch
  u64* z0;         // rank(sp, 0): the interval's first entry of the table
  u64* cnt;        // hits kept of it (after the max_hits cut)
  u64* len;        // the overlap's length
};

// Query k = text[offsets[k] .. offsets[k + 1]), comp values 1..5 (anything else ends the search there: nothing matches it).
// EMIT == false: rec_base[k] = the query's intervals, n_hits[k] = its hits, hit_base[k] = the hits kept of them; the generic scan then turns
// rec_base[0 .. count] and hit_base[0 .. count] in place into the first record and the first hit slot of every query.
// EMIT == true: reads the three arrays as the scans left them and stores the query's records.
template<bool EMIT>
__global__ void __launch_bounds__(BLOCK_THREADS) k_overlap_scan(IndexView x, const u8* text, const u64* offsets, u64 count, u64 min_overlap, u64 max_hits,
  u64* rec_base, u64* n_hits, u64* hit_base, OverlapRecs recs)
{
  __shared__ u64 sC[8];
  load_C(sC, x);
  const u32 q = threadIdx.x & 3;
  const u64 k = ((u64)blockIdx.x * BLOCK_THREADS + threadIdx.x) >> 2;
  if(k >= count) { return; }
  const u64 begin = offsets[k], end = offsets[k + 1];
  u64 total = 0, kept = 0, nint = 0, base_r = 0, base_h = 0;
  if(EMIT)
  {
    total = n_hits[k]; base_r = rec_base[k]; nint = rec_base[k + 1] - base_r; base_h = hit_base[k];
    kept = (max_hits > 0 && total > max_hits ? max_hits : total);
  }
  u64 seen = 0, found = 0;
  if(end > begin)
  {
    u64 pos = end - 1, len = 1;
    const u32 c0 = text[pos];
    u64 sp = 0, e1 = 0;                                                     // the range as [sp, e1), e1 = ep + 1
    if(c0 >= 1 && c0 <= 5) { sp = sC[c0]; e1 = sC[c0 + 1]; }
    while(sp < e1 && e1 <= x.n)                                             // quad-uniform; sp <= n - 1
    {
      const bool at_end = (e1 == x.n);
      const u64 pe = (at_end ? e1 - 1 : e1);
      const u32 c = (pos > begin ? (u32)text[pos - 1] : 0u);                // the next symbol, 0: none
      QuadRec ra, rb;
      quad_load(x, sp, pe, q, ra, rb);
      if(len >= min_overlap)
      {
        const u64 z0 = quad_rank_zero(ra, q, sp);
        const u64 z1 = (at_end ? sC[1] - sC[0] : quad_rank_zero(rb, q, e1));
        if(z1 > z0)
        {
          const u64 cnt = z1 - z0;
          if(EMIT)
          {
            if(found >= nint || cnt > total - seen) { break; }              // not what the count pass saw: nothing more is stored
            const u64 lo = total - seen - cnt;                              // the interval's slots of the query: [lo, lo + cnt)
            if(q == 0)
            {
              const u64 r = base_r + (nint - 1 - found);
              recs.first[r] = base_h + (lo < kept ? lo : kept);
              recs.z0[r] = z0;
              recs.cnt[r] = (lo < kept ? (cnt < kept - lo ? cnt : kept - lo) : 0);
              recs.len[r] = len;
            }
          }
          seen += cnt; found++;
        }
      }
      if(c < 1 || c > 5) { break; }
      sp = sC[c] + quad_rank(ra, q, c, sp);
      e1 = sC[c] + (at_end ? sC[c + 1] - sC[c] : quad_rank(rb, q, c, e1));
      pos--; len++;
    }
  }
  if(!EMIT && q == 0)
  {
    rec_base[k] = found; n_hits[k] = seen; hit_base[k] = (max_hits > 0 && seen > max_hits ? max_hits : seen);
    if(k + 1 == count) { rec_base[count] = 0; hit_base[count] = 0; }      // the scans run over count + 1 entries: the last ones become the totals
  }
}

// out[k] = lengths[k] for k < count and out[count] = 0: the lengths of a batch of sequences as the generic scan wants them, so that their
// offsets come to be where the text is and never travel.
__global__ void __launch_bounds__(BLOCK_THREADS) k_overlap_widen(const u32* lengths, u64 count, u64* out)
{
  const u64 k = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(k <= count) { out[k] = (k < count ? lengths[k] : 0); }
}

// Hit slot first_hit + j of the batch, j < count: its record is the last of the batch's nrecs with first <= slot (first[0] == 0, never
// decreasing; records that hold no hit share their first slot with the next one that does).  ids[j] = table[z0 + e], lengths[j] = len.
// An entry of the table that is no sequence, or a record that does not hold the slot, counts as damage: status = min(status, j).
__global__ void __launch_bounds__(BLOCK_THREADS) k_overlap_expand(const u64* table, u64 m, OverlapRecs recs, u64 nrecs, u64 first_hit, u64 count,
  u64* ids, u64* lengths, unsigned long long* status)
{
  const u64 j = (u64)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  if(j >= count) { return; }
  const u64 h = first_hit + j;
  const u64 lo = last_at_or_below(recs.first, nrecs, h);
  const u64 e = h - recs.first[lo];
  const u64 z = recs.z0[lo] + e;
  bool ok = (e < recs.cnt[lo] && z >= e && z < m);
  u64 id = 0;
  if(ok) { id = table[z]; ok = (id < m); }
  if(ok) { ids[j] = id; lengths[j] = recs.len[lo]; }
  else { atomicMin(status, (unsigned long long)j); }
}
