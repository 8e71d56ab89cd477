/*
  api/unitigs.hip.h -- the unitigs of the k-mer graph over the solid k-mers of a spectrum (bwtm_unitigs_*): the compacted de Bruijn graph
  with its coverage and links, built on the device in the phases of kernels/unitigs.hip.h, downloaded in slices, and k-mers placed in it.
  Part of bwtm_api.hip.

  With S = the k-mers of count >= threshold (the nodes), U = the unitigs, Y = the symbols of their texts (the sum of n_u + k - 1 = S +
  (k - 1) U) and D = min(2 k, 24, max(1, ceil(log2 S))), the handle keeps

      H = 8 max(S, 1) + 8 (2^D + 1) + 16 S + 57 U + 8 + Y bytes

    8 max(S, 1) + 8 (2^D + 1)  the corrector's table: the codes of the nodes and the bucket directory (api/correct.hip.h).
   16 S   the unitig and the offset of every node (bwtm_unitigs_place).
   57 U + 8 + Y   per unitig: the text offsets (U + 1), node counts and occurrences, 8 bytes each, one byte of flags, four links of
          8 bytes; and the text.
  in ten blocks, each rounded up by the pool: a block of 1 MiB or more to 64 KiB, of 64 MiB or more to 2 MiB (a sixteenth of the block at
  the most), a smaller one to 256 bytes; a block the pool had cached may be an eighth larger than asked for.  So
  bwtm_unitigs_bytes <= 9/8 (17/16 H + 2560).  A block of 512 MiB or more is made of whole chunks of 1 GiB (api/context.hip.h).

  Device memory of bwtm_unitigs_create, n = the k-mers of the k-mer handle.  Every block the call ever takes, added up (the pool hands a
  released block to a later request of nearly its size only, so the sum is what bounds the pool's growth):

      peak <= 17/16 (H + 8 n + 25 S + 8 U + C + (n + 2 S + U) / 128) + 2^16 bytes            (every block below 512 MiB)

    8 (n + 1)   the flags whose scan gives every solid code its slot: released when the table stands.
    8 S   the counts of the nodes beside their codes; a path's start ends up holding the path's sum.
   17 S + 8   the successor index (8) and the degrees (1) of every node, and the start flags whose scan numbers the unitigs (8 (S + 1)).
    8 U   the last node of every unitig, for its links.
    C = 32 S when some node lies on a pure cycle (two double-buffered pairs of minimum and jump pointer per node), else 0.
    (n + 2 S + U) / 128   the partial sums of the three scans (8 bytes per 2048 items, and theirs), four 8-byte cells.
  A result that does not fit is BWTM_ENOMEM.

  The kernels that run one lane per node take bwtm_tune("unitig_launch") nodes per launch (2^31, the most a grid holds with room to
  spare); the directory of the table is k_correct_dir's one launch, which holds S < 2^32 - 256.
*/
#pragma once

struct bwtm_unitigs
{
  bwtm_context* ctx = nullptr;
  bwtm_unitigs() : ctx(t_ctx) { if(ctx) { ctx->live_handles++; } }
  ~bwtm_unitigs() { if(ctx) { ctx->live_handles--; } }
  bwtm_unitigs(const bwtm_unitigs&) = delete; bwtm_unitigs& operator=(const bwtm_unitigs&) = delete;
  DevBuf codes, dir;                  // the table of the nodes (CorrectTable)
  DevBuf unitig, off;                 // per node: its unitig and its offset there
  DevBuf offsets, text;               // per unitig: U + 1 text offsets; the texts
  DevBuf nodes, occ, flags, links;    // per unitig: node count, occurrences, flags (one byte), four links
  u64 solid = 0, count = 0, symbols = 0, threshold = 0;
  u32 k = 0, skip = 0, dir_bits = 0;
  CorrectTable table() const { return CorrectTable{codes.as<const u64>(), dir.as<const u64>(), solid, k, skip, dir_bits}; }
  u64 bytes() const { return codes.bytes + dir.bytes + unitig.bytes + off.bytes + offsets.bytes + text.bytes + nodes.bytes + occ.bytes + flags.bytes + links.bytes; }
};

namespace
{
// What the last bwtm_unitigs_create of this thread did: table lookups, the longest unitig in nodes, nodes in circular unitigs, min-jump rounds.
thread_local CallStats t_unitig_stats;

constexpr u64 UNITIG_PLACE_BATCH = 1ull << 24;          // codes per batch of bwtm_unitigs_place: 24 bytes each on the device

u64 unitig_part() { return (u64)std::max<long long>(1, std::min<long long>(g_tune.unitig_launch, 1ll << 31)); }

// A kernel over the items [0, n) whose first two parameters are the range [first, end) of one launch.
#define UNITIG_LAUNCH(name, kernel, n, ...) do { \
  for(u64 first_ = 0, n_ = (n); first_ < n_; first_ += unitig_part()) \
  { \
    const u64 end_ = std::min(n_, first_ + unitig_part()); \
    LAUNCH(name, kernel, div_up(end_ - first_, BLOCK_THREADS), BLOCK_THREADS, first_, end_, __VA_ARGS__); \
  } } while(0)

// The corrector's table (corrector_build's flag / scan / compact scheme and its directory) with the counts of the solid k-mers beside it.
int unitigs_table(bwtm_unitigs* g, const bwtm_kmers* km, DevBuf& cnt)
{
  const u64 n = km->distinct;
  auto alloc_codes = [&]() -> int { return g->codes.alloc(std::max<u64>(g->solid, 1) * sizeof(u64)); };
  if(n > 0)
  {
    DevBuf flags;
    TRY(flags.alloc((n + 1) * sizeof(u64)));
    for(u64 first = 0; first < n; first += unitig_part())                                       // a part's flags[part] = 0 is the next part's first flag, which that part writes
    {
      const u64 part = std::min(unitig_part(), n - first);
      LAUNCH("correct_flag", k_correct_flag, div_up(part + 1, BLOCK_THREADS), BLOCK_THREADS, km->cnt() + first, part, g->threshold, flags.as<u64>() + first);
    }
    TRY(device_scan<0>(flags.as<const u64>(), flags.as<u64>(), n + 1));
    TRY(fetch_u64(flags.as<u64>() + n, 0));
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    g->solid = CTX.host_scratch[0];
    if(g->solid > n) { return fail(BWTM_EINVAL, "bwtm_unitigs_create: %llu of %llu k-mers counted as solid", (unsigned long long)g->solid, (unsigned long long)n); }
    TRY(alloc_codes());
    if(g->solid > 0)
    {
      TRY(cnt.alloc(g->solid * sizeof(u64)));
      for(u64 first = 0; first < n; first += unitig_part())
      {
        const u64 part = std::min(unitig_part(), n - first);
        LAUNCH("correct_compact", k_correct_compact, div_up(part, BLOCK_THREADS), BLOCK_THREADS, km->code() + first, km->cnt() + first, flags.as<const u64>() + first, part, g->threshold,
          g->codes.as<u64>(), g->solid);
        LAUNCH("unitig_counts", k_unitig_counts, div_up(part, BLOCK_THREADS), BLOCK_THREADS, km->cnt() + first, flags.as<const u64>() + first, part, g->threshold, cnt.as<u64>(), g->solid);
      }
    }
  }
  else { TRY(alloc_codes()); }
  g->dir_bits = correct_dir_bits(g->k, g->solid);
  const u64 buckets = 1ull << g->dir_bits;
  TRY(g->dir.alloc((buckets + 1) * sizeof(u64)));
  LAUNCH("correct_dir", k_correct_dir, div_up(g->solid + 1, BLOCK_THREADS), BLOCK_THREADS, g->codes.as<const u64>(), g->solid, 2 * g->k - g->dir_bits, buckets, g->dir.as<u64>());
  return BWTM_OK;                                                                               // `flags` returns to the pool (stream ordered)
}

// The nodes no walk has visited.
int unitigs_unreached(const u64* head, u64 solid, DevBuf& cell, u64* out)
{
  HIP_TRY(hipMemsetAsync(cell.p, 0, sizeof(u64), CTX.stream));
  LAUNCH("unitig_unreached", k_unitig_unreached, std::min<u64>(div_up(solid, BLOCK_THREADS), 1024), BLOCK_THREADS, head, solid, cell.as<unsigned long long>());
  TRY(fetch_u64(cell.as<u64>(), 0));
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  *out = CTX.host_scratch[0];
  return BWTM_OK;
}

int unitigs_build(bwtm_unitigs* g, const bwtm_kmers* km)
{
  DevBuf cnt;
  TRY(unitigs_table(g, km, cnt));
  const u64 S = g->solid;
  const u32 k = g->k;
  if(S == 0)
  {
    TRY(g->offsets.alloc(sizeof(u64), true));                                                   // offsets[0] = 0: U = 0
    HIP_TRY(hipStreamSynchronize(CTX.stream));
    return BWTM_OK;
  }
  const CorrectTable t = g->table();
  DevBuf next, deg, start, stats, cell;
  TRY(next.alloc(S * sizeof(u64))); TRY(deg.alloc(S)); TRY(start.alloc((S + 1) * sizeof(u64)));
  TRY(stats.alloc(4 * sizeof(u64), true)); TRY(cell.alloc(sizeof(u64)));
  DevBuf& head = g->unitig;                                                                     // a node's start, until k_unitig_number makes it the node's unitig
  TRY(head.alloc(S * sizeof(u64))); TRY(g->off.alloc(S * sizeof(u64)));
  HIP_TRY(hipMemsetAsync(head.p, 0xFF, S * sizeof(u64), CTX.stream));                           // UNITIG_NONE: not visited
  UNITIG_LAUNCH("unitig_links", k_unitig_links, S, t, next.as<u64>(), deg.as<u8>(), start.as<u64>(), stats.as<unsigned long long>());
  UNITIG_LAUNCH("unitig_next", k_unitig_next, S, S, next.as<u64>(), deg.as<const u8>(), start.as<u64>());
  UNITIG_LAUNCH("unitig_walk", k_unitig_walk, S, S, next.as<const u64>(), cnt.as<u64>(), start.as<const u64>(), head.as<u64>(), g->off.as<u64>());
  u64 unreached = 0, rounds = 0;
  TRY(unitigs_unreached(head.as<const u64>(), S, cell, &unreached));
  if(unreached > 0)                                                                             // pure cycles: their smallest nodes become starts
  {
    DevBuf m0, j0, m1, j1;
    TRY(m0.alloc(S * sizeof(u64))); TRY(j0.alloc(S * sizeof(u64))); TRY(m1.alloc(S * sizeof(u64))); TRY(j1.alloc(S * sizeof(u64)));
    UNITIG_LAUNCH("unitig_cycle_init", k_unitig_cycle_init, S, S, head.as<const u64>(), next.as<const u64>(), m0.as<u64>(), j0.as<u64>());
    while(rounds < 64 && (1ull << rounds) < unreached)
    {
      UNITIG_LAUNCH("unitig_cycle_jump", k_unitig_cycle_jump, S, S, head.as<const u64>(), m0.as<const u64>(), j0.as<const u64>(), m1.as<u64>(), j1.as<u64>());
      m0.swap(m1); j0.swap(j1);
      rounds++;
    }
    UNITIG_LAUNCH("unitig_cycle_starts", k_unitig_cycle_starts, S, head.as<const u64>(), m0.as<const u64>(), start.as<u64>());
    UNITIG_LAUNCH("unitig_walk", k_unitig_walk, S, S, next.as<const u64>(), cnt.as<u64>(), start.as<const u64>(), head.as<u64>(), g->off.as<u64>());
    TRY(unitigs_unreached(head.as<const u64>(), S, cell, &unreached));
    if(unreached > 0) { return fail(BWTM_EINVAL, "bwtm_unitigs_create: %llu nodes lie on no path and no cycle", (unsigned long long)unreached); }
  }
  // the starts in code order are the unitigs
  TRY(device_scan<0>(start.as<const u64>(), start.as<u64>(), S + 1));
  TRY(fetch_u64(start.as<u64>() + S, 0));
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  const u64 U = CTX.host_scratch[0];
  if(U == 0 || U > S) { return fail(BWTM_EINVAL, "bwtm_unitigs_create: %llu unitigs of %llu nodes", (unsigned long long)U, (unsigned long long)S); }
  g->count = U;
  DevBuf last;
  TRY(g->offsets.alloc((U + 1) * sizeof(u64), true)); TRY(g->nodes.alloc(U * sizeof(u64))); TRY(g->occ.alloc(U * sizeof(u64))); TRY(g->flags.alloc(U));
  TRY(g->links.alloc(4 * U * sizeof(u64))); TRY(last.alloc(U * sizeof(u64)));
  UNITIG_LAUNCH("unitig_number", k_unitig_number, S, S, U, k, next.as<const u64>(), head.as<u64>(), g->off.as<const u64>(), cnt.as<const u64>(), start.as<const u64>(),
    g->nodes.as<u64>(), g->occ.as<u64>(), g->flags.as<u8>(), last.as<u64>(), g->offsets.as<u64>(), stats.as<unsigned long long>());
  TRY(device_scan<0>(g->offsets.as<const u64>(), g->offsets.as<u64>(), U + 1));                 // text lengths -> text offsets
  TRY(fetch_u64(g->offsets.as<u64>() + U, 0));
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  g->symbols = CTX.host_scratch[0];
  if(g->symbols != S + (u64)(k - 1) * U) { return fail(BWTM_EINVAL, "bwtm_unitigs_create: %llu symbols for %llu nodes in %llu unitigs", (unsigned long long)g->symbols, (unsigned long long)S, (unsigned long long)U); }
  TRY(g->text.alloc(g->symbols));
  UNITIG_LAUNCH("unitig_text", k_unitig_text, S, k, g->skip, g->codes.as<const u64>(), head.as<const u64>(), g->off.as<const u64>(), g->offsets.as<const u64>(), U, g->text.as<u8>(), g->symbols);
  UNITIG_LAUNCH("unitig_fill_links", k_unitig_fill_links, U, t, last.as<const u64>(), g->flags.as<const u8>(), head.as<const u64>(), g->links.as<u64>(), stats.as<unsigned long long>());
  TRY(fetch_u64(stats.as<u64>(), 0, 3));
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  for(u32 j = 0; j < 3; j++) { t_unitig_stats[j] = CTX.host_scratch[j]; }
  t_unitig_stats[3] = rounds;
  return BWTM_OK;
}

} // namespace

extern "C" int bwtm_unitigs_create(const bwtm_kmers* kmers, uint32_t skip, uint64_t threshold, bwtm_unitigs** out)
{
  if(!kmers || !out) { return fail(BWTM_EINVAL, "bwtm_unitigs_create: null argument"); }
  ENTER(kmers->ctx);
  if(skip < 1 || skip > 5) { return fail(BWTM_EINVAL, "bwtm_unitigs_create: skip = %u is no comp value 1..5", (unsigned)skip); }
  if(kmers->k == 0 || kmers->k > KMER_MAX_K) { return fail(BWTM_EINVAL, "bwtm_unitigs_create: the k-mer handle has k = %u", (unsigned)kmers->k); }
  if(threshold == 0) { threshold = 1; }
  t_unitig_stats.reset();
  bwtm_unitigs* g = new bwtm_unitigs();
  g->k = kmers->k; g->skip = skip; g->threshold = threshold;
  const int rc = unitigs_build(g, kmers);
  if(rc != BWTM_OK) { (void)hipStreamSynchronize(CTX.stream); delete g; return rc; }
  *out = g;
  return BWTM_OK;
}

extern "C" void bwtm_unitigs_free(bwtm_unitigs* unitigs)
{
  if(!unitigs) { return; }
  Scope scope(unitigs->ctx);
  delete unitigs;                                     // the graph returns to the pool (stream ordered)
}

extern "C" uint64_t bwtm_unitigs_count(const bwtm_unitigs* unitigs) { return unitigs ? unitigs->count : 0; }
extern "C" uint64_t bwtm_unitigs_nodes(const bwtm_unitigs* unitigs) { return unitigs ? unitigs->solid : 0; }
extern "C" uint64_t bwtm_unitigs_symbols(const bwtm_unitigs* unitigs) { return unitigs ? unitigs->symbols : 0; }
extern "C" uint64_t bwtm_unitigs_bytes(const bwtm_unitigs* unitigs) { return unitigs ? unitigs->bytes() : 0; }
extern "C" uint32_t bwtm_unitigs_k(const bwtm_unitigs* unitigs) { return unitigs ? unitigs->k : 0; }

extern "C" int bwtm_unitigs_stats(uint64_t stats[4]) { return t_unitig_stats.get("bwtm_unitigs_stats", stats); }

extern "C" int bwtm_unitigs_download(const bwtm_unitigs* unitigs, uint64_t first, uint64_t count, uint64_t* offsets, uint8_t* text, uint64_t capacity,
                                     uint64_t* nodes, uint64_t* occurrences, uint8_t* flags, uint64_t* links)
{
  if(!unitigs) { return fail(BWTM_EINVAL, "bwtm_unitigs_download: null argument"); }
  ENTER(unitigs->ctx);
  if(first > unitigs->count || count > unitigs->count - first)
  {
    return fail(BWTM_EINVAL, "bwtm_unitigs_download: unitigs %llu + %llu lie beyond the %llu unitigs", (unsigned long long)first, (unsigned long long)count,
      (unsigned long long)unitigs->count);
  }
  if(count == 0) { if(offsets) { offsets[0] = 0; } return BWTM_OK; }
  const u64* d_off = unitigs->offsets.as<const u64>() + first;
  TRY(fetch_u64(d_off, 0)); TRY(fetch_u64(d_off + count, 1));
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  const u64 begin = CTX.host_scratch[0], total = CTX.host_scratch[1] - begin;
  const bool want_text = (text && capacity > 0);
  if(want_text && capacity < total)                                                             // before anything is written
  {
    return fail(BWTM_EINVAL, "bwtm_unitigs_download: capacity %llu is too small (%llu bytes of text)", (unsigned long long)capacity, (unsigned long long)total);
  }
  TRY(to_host(offsets, d_off, count + 1));
  if(want_text) { TRY(to_host(text, unitigs->text.as<const u8>() + begin, total)); }
  TRY(to_host(nodes, unitigs->nodes.as<const u64>() + first, count)); TRY(to_host(occurrences, unitigs->occ.as<const u64>() + first, count));
  TRY(to_host(flags, unitigs->flags.as<const u8>() + first, count)); TRY(to_host(links, unitigs->links.as<const u64>() + 4 * first, 4 * count));
  HIP_TRY(hipStreamSynchronize(CTX.stream));
  if(offsets) { for(u64 j = 0; j <= count; j++) { offsets[j] -= begin; } }                      // the window's offsets start at 0
  return BWTM_OK;
}

extern "C" int bwtm_unitigs_place(const bwtm_unitigs* unitigs, const uint64_t* codes, uint64_t count, uint64_t* unitig, uint64_t* offset)
{
  if(!unitigs || (count > 0 && !codes)) { return fail(BWTM_EINVAL, "bwtm_unitigs_place: null argument"); }
  ENTER(unitigs->ctx);
  if(count == 0) { return BWTM_OK; }
  const u64 batch = std::min(UNITIG_PLACE_BATCH, count);
  DevBuf d_codes, d_unitig, d_offset;
  TRY(d_codes.alloc(batch * sizeof(u64))); TRY(d_unitig.alloc(batch * sizeof(u64))); TRY(d_offset.alloc(batch * sizeof(u64)));
  for(u64 done = 0; done < count; done += batch)
  {
    const u64 nb = std::min(batch, count - done);
    HIP_TRY(hipMemcpyAsync(d_codes.p, codes + done, nb * sizeof(u64), hipMemcpyHostToDevice, CTX.stream));
    LAUNCH("unitig_place", k_unitig_place, div_up(nb, BLOCK_THREADS), BLOCK_THREADS, unitigs->table(), unitigs->unitig.as<const u64>(), unitigs->off.as<const u64>(),
      d_codes.as<const u64>(), nb, d_unitig.as<u64>(), d_offset.as<u64>());
    TRY(to_host(at_or_null(unitig, done), d_unitig.as<const u64>(), nb)); TRY(to_host(at_or_null(offset, done), d_offset.as<const u64>(), nb));
    HIP_TRY(hipStreamSynchronize(CTX.stream));                                                  // the batch's buffers are reused
  }
  return BWTM_OK;
}
