/*
  bwtm_kernels.hip.h -- hand-written gfx950 (CDNA4, wave64) kernels of the rank-array /
  interleave path.  Included by bwtm_api.hip only.

  Kernel map (reference code each one replaces):
    k_block_len        BWT::build scan of the run stream            bwt.cpp:487-502
    k_build_sup/recs   native blocks -> device records ("transcode at upload", BWT::load)
    k_block_cum        samples[c] at the block starts               bwt.cpp:489-511
    k_sym_*            plain symbols -> device records (input tooling)
    k_ingest_*         reads -> BWT symbols of a leaf (suffix radix sort; SURVEY 8(f1), no counterpart in the reference)
    k_frontier_*       buildRA + BWT::inverse_select + BWT::rank, level-synchronous form (product)
                                                                    fmi.cpp:272-334, bwt.cpp:318-341, 445-464
    k_bound_suffix_min, k_tile_build_frontier
                       mergeRA / RLArray / RankArray: the sorted emits of every step -> bitvector tiles
                                                                    fmi.cpp:139-257, support.h:396-638
    k_lf_walk_binned, k_lf_walk_quad, k_part_*, k_tile_build
                       the same two stages in per-chain form (small shards, long sequences, > 40-bit coordinates)
    k_cut_search_seg, k_pull_tables, k_node_cut_search, k_gather_nodes, k_frontier_step<.., PULL>
                       the same search with the records PARTITIONED over several GPUs (one part each): the thread fan-out of
                       fmi.cpp:351-358 as position ranges instead of sequence blocks (kernels/partition.hip.h, api/pmerge.hip.h)
    kernels/diagnostics.hip.h (only with -DBWTM_DIAGNOSTICS): timing-only and A/B variants, not in the product
    kernels/search_view.hip.h, k_frontier_step<.., VIEW>, k_frontier_gather (only with -DBWTM_EXPERIMENTAL): the two-plane search
                       view and the sliced frontier search -- exact, tested, measured, not in the product (include/bwtm_experimental.h)
    k_chunk_popc       RA finalize (prefix counts of the interleaving bitvector)
    k_interleave_*     mergeBWT                                     bwt.cpp:215-282
    k_enc_*            RunBuffer + Run::write, block starts of BWT::build
                                                                    utils.h:121-142, support.h:256-282, bwt.cpp:496
    k_fold_*           byte-offset carry of Run::write across segments (array.size() % 64, support.h:267)
    k_piece_fields     the samples of one piece of a streamed merge, from the encoder's block starts and cum32 (kernels/stream.hip.h)
    k_rank_batch, k_inverse_select_batch, k_extract, k_find_batch
                       BWT::rank / inverse_select / extract, FMI::find  bwt.cpp:318-464, fmi.h:195-221
    kernels/quad.hip.h (no kernel): four lanes per LF walk -- the record reader (QuadRec, quad_load, quad_symbol, quad_rank,
                       quad_rank_zero, quad_step) and the bounded walk (quad_walk_to_start) under the three families below, on the quad
                       primitives of kernels/search_walk.hip.h
    k_seq_lengths, k_seq_emit
                       sequences by id: the LF walk from the endmarker, on the reader of kernels/quad.hip.h (kernels/sequences.hip.h; no
                       counterpart in the reference, the inverse of k_ingest_*)
    k_locate_build, k_locate_check, k_locate
                       from a BWT position to (sequence id, offset): the same walk from any position, and one table per index that
                       numbers the whole-sequence suffixes (kernels/locate.hip.h; the step the reference's queries leave to the host)
    k_overlap_scan<EMIT>, k_overlap_expand
                       suffix-prefix overlaps: one backward search per query (the same reader, two records per step) whose rank(., 0)
                       pairs are intervals of the locator's table, counted, then emitted longest first and expanded to (id, length)
                       (kernels/overlap.hip.h; the overlap step of a string-graph assembler, no counterpart in the reference)
    k_ms_scan, k_mem_pattern, k_mem_emit (k_mem_flag)
                       matching statistics and maximal exact matches of patterns: one backward search per (pattern, end) on the same
                       reader, which keeps the last range that is not empty; for the MEMs one quad per pattern, ends descending, that
                       flags the ends whose search gets below the begin of the search before, the flags scanned into slots and emitted
                       as (begin, length, range); k_mem_flag, the same flags from the lengths of k_ms_scan, is the A/B partner
                       (kernels/mem.hip.h; the seeds of seed-and-extend, no counterpart in the reference)
    kernels/level.hip.h (no kernel): what the four level-wise trie walks below share -- the lane's ranks of a range (level_lane_ranks) and
                       the stable placement of a level's children without atomics: count pass, one scan, expand pass (level_place,
                       level_publish, level_slot)
    k_kmer_level<QUAD, EMIT>, k_kmer_sum, k_kmer_hist
                       the distinct k-mers with their counts: the suffix trie down to depth k, level by level, every level the stable
                       split by symbol of the one before (count pass, scan, expand-and-scatter pass), and the spectrum of the result
                       (kernels/kmers.hip.h; no counterpart in the reference)
    k_kmer_join_level<EMIT>, k_kmer_join_summary
                       the k-mers of two indexes side by side: one joint walk down both suffix tries, a node a range in each index
                       (an insertion point where the string is absent), the same stable split per level, and the summary of the result
                       (kernels/kmer_join.hip.h; the first levels of the merger's own search, generalised; no counterpart in the reference)
    k_approx_roots, k_approx_level<QUAD, EMIT>, k_approx_mark, k_approx_cap, k_approx_gather
                       patterns with up to d substitutions: the backward search of a batch as one frontier of (range, pattern, symbols
                       left, mismatches spent), every level a count pass, a scan and an expand pass into the next frontier and the hit
                       stream, both in parent-then-symbol order; then every pattern's hits found by their neighbours and gathered
                       (kernels/approx.hip.h; no counterpart in the reference)
    k_edit_roots, k_edit_level<EMIT>, k_edit_mark, k_edit_cap, k_edit_gather
                       patterns within edit distance e: the same frontier, a node (range, pattern, 15 fields of the edit-distance
                       column around its depth), a child kept for the next frontier and / or a hit, independently, so that a pattern's
                       hits appear over 2 e + 1 levels; then marked and gathered per pattern and length
                       (kernels/edit.hip.h; no counterpart in the reference)
    k_correct_flag, k_correct_compact, k_correct_dir, k_correct_wave
                       k-mer error correction of reads: the codes of the solid k-mers compacted out of a spectrum, a bucket directory over
                       their top bits, and one wave per read that looks its windows up 64 at a time, finds the uncovered positions from a
                       ballot and substitutes one symbol per round (kernels/correct.hip.h; no counterpart in the reference)
    k_unitig_counts, k_unitig_links, k_unitig_next, k_unitig_walk, k_unitig_unreached, k_unitig_cycle_init, k_unitig_cycle_jump,
    k_unitig_cycle_starts, k_unitig_number, k_unitig_text, k_unitig_fill_links, k_unitig_place
                       the unitigs of the k-mer graph over that table: degrees and the one compactable successor per node, a walk per
                       path start, pointer jumping for the smallest node of a pure cycle, two scans that number the unitigs and place
                       their text, the links of their last nodes (kernels/unitigs.hip.h; no counterpart in the reference)
*/
#pragma once

#include <hip/hip_runtime.h>
#include "bwtm_device.h"
#include "bwtm_bitmerge.h"
#ifdef BWTM_EXPERIMENTAL
#include "bwtm_view.h"
#endif

namespace bwtm
{

constexpr int WAVE = 64;
constexpr int BLOCK_THREADS = 256;

// Read-only view of a device index for kernels.
struct IndexView
{
  const uint4* recs;     // 4 x uint4 per record
  const u64*   sup;      // SUP_STRIDE u64 per super
  u64 n;                 // positions
  u64 m;                 // sequences
  u64 nrecs;
  u64 C[8];              // C[c] = number of symbols smaller than c
#ifdef BWTM_EXPERIMENTAL
  const uint4* view;     // the search view (4 x uint4 per 160 positions; null unless built: bwtm_view.h)
  const u64* vsup;
  u64 nview;
#endif
};

// Streaming stores: data that is written once and not read again by the kernel that writes it (the next frontier's coordinates, emits, records
// of a transcode / interleave, encoded bytes) goes past the L2 with the non-temporal hint, which leaves the cache to the lines that ARE re-used
// (the records neighbouring elements share).  Round 5: -2.8 % on k_frontier_step from its two stores alone (profiles/r05_nt_stores_ab.txt).
typedef unsigned int bwtm_v4u __attribute__((ext_vector_type(4)));
__device__ inline void nt_store(uint4* p, const uint4& v) { __builtin_nontemporal_store(bwtm_v4u{v.x, v.y, v.z, v.w}, (bwtm_v4u*)p); }
__device__ inline void nt_store(uint2* p, const uint2& v) { __builtin_nontemporal_store((unsigned long long)v.x | ((unsigned long long)v.y << 32), (unsigned long long*)p); }
__device__ inline void nt_store(unsigned short* p, unsigned short v) { __builtin_nontemporal_store(v, p); }
__device__ inline void nt_store(u64* p, u64 v) { __builtin_nontemporal_store(v, p); }
__device__ inline void nt_store(u32* p, u32 v) { __builtin_nontemporal_store(v, p); }

#include "kernels/common.hip.h"
#include "kernels/transcode.hip.h"
#include "kernels/queries.hip.h"
#include "kernels/search_walk.hip.h"
#include "kernels/quad.hip.h"
#include "kernels/sequences.hip.h"
#include "kernels/locate.hip.h"
#include "kernels/overlap.hip.h"
#include "kernels/mem.hip.h"
#include "kernels/level.hip.h"
#include "kernels/kmers.hip.h"
#include "kernels/kmer_join.hip.h"
#include "kernels/approx.hip.h"
#include "kernels/edit.hip.h"
#include "kernels/correct.hip.h"
#include "kernels/unitigs.hip.h"
#ifdef BWTM_DIAGNOSTICS
#include "kernels/diagnostics.hip.h"
#endif
#ifdef BWTM_EXPERIMENTAL
#include "kernels/search_view.hip.h"
#endif
#include "kernels/search_frontier.hip.h"
#include "kernels/partition.hip.h"
#ifdef BWTM_EXPERIMENTAL
#include "kernels/search_partition.hip.h"
#endif
#include "kernels/search_range.hip.h"
#include "kernels/interleave.hip.h"
#include "kernels/encoder.hip.h"
#include "kernels/stream.hip.h"
#include "kernels/ingest.hip.h"

} // namespace bwtm
