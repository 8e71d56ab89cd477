/*
  bwtm.h -- C ABI of the MI355X-native rank-array / interleave path of bwt-merge.

  The reference (jltsiren/bwt-merge) has no FFI: its seam for this path is the C++ API
      FMI::FMI(FMI& a, FMI& b, MergeParameters)          fmi.h:110, fmi.cpp:336-369
      BWT::BWT(BWT& a, BWT& b, RankArray& ra)            bwt.h:73,  bwt.cpp:286-314
  called from merge() in bwt_merge.cpp:287-299.  This header is the boundary a maintainer
  binds instead; the C++ facade in bwt-merge_amd/csrc/host keeps the
  reference's class and member names and routes them here.

  Conventions
    * Plain pointers and sizes only.  Host pointers unless a parameter says "device".
    * Every function returns 0 on success and a non-zero BWTM_E* code on failure;
      bwtm_last_error() returns a message for the calling thread's last failure.
      (The reference prints to std::cerr and calls std::exit(EXIT_FAILURE); the facade and
      the CLI convert the status codes back into that behaviour.)
    * Calls are blocking and not re-entrant per handle.  All device state lives in a CONTEXT (one HIP
      device, the library's streams, its memory pool); a host thread per GPU binds its own context
      (bwtm_init / bwtm_context_make_current) and handles remember the context they were created in, so
      a C++ host can drive several GPUs from several threads of one process (ParallelLoop's workers,
      fmi.cpp:351-358, become one thread per GPU).  Calls on the same context are serialized.
    * Device buffers are owned by the library behind opaque handles; host output buffers
      are owned by the caller (sizes are queried first).
    * All integers are unsigned 64-bit like the reference's size_type (utils.h:44).
*/
#ifndef BWTM_H
#define BWTM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BWTM_SIGMA 6            /* Run::SIGMA, support.h:228 */
#define BWTM_RLE_BLOCK 64       /* Run::BLOCK_SIZE, support.h:227 */

enum
{
  BWTM_OK = 0,
  BWTM_EINVAL = 1,              /* bad argument / malformed input */
  BWTM_ENODEV = 2,              /* no usable GPU, or HIP runtime failure */
  BWTM_ENOMEM = 3,              /* device or host allocation failed */
  BWTM_EALPHABET = 4,           /* fmi.cpp:338-342: cannot merge BWTs with different alphabets */
  BWTM_EPEER = 5                /* another part of a multi-GPU merge failed or did not arrive (bwtm_group_*, bwtm_part_*) */
};

typedef struct bwtm_context bwtm_context; /* one HIP device + the library's streams and memory pool */
typedef struct bwtm_index bwtm_index;   /* device-resident FM-index: replaces a loaded FMI (fmi.h:225-226) */
typedef struct bwtm_ra    bwtm_ra;      /* device-resident rank array: replaces RankArray (support.h:576-638) */

/* --- library ------------------------------------------------------------------------ */

/* Binds the calling thread to the process-wide default context of HIP device `device` (created on
   first use).  Threads that never call it use device 0. */
int bwtm_init(int device);
/* Additional contexts (e.g. two independent pipelines on one GPU, or explicit per-thread ownership).
   A context may be current in one thread at a time; destroying it requires that its handles are gone. */
int bwtm_context_create(int device, bwtm_context** out);
int bwtm_context_make_current(bwtm_context* context);      /* NULL: back to the default context of device 0 */
void bwtm_context_destroy(bwtm_context* context);
const char* bwtm_last_error(void);
/* Knobs for tests and measurements; the defaults are what a caller wants.
   Keys that select timing-only kernel variants exist only in builds with -DBWTM_DIAGNOSTICS. */
int bwtm_tune(const char* key, long long value);
/* Returns the cached device memory of the calling thread's context to the driver (device buffers
   released by handles are kept in a pool for reuse). */
int bwtm_trim(void);
/* Blocks until all work queued in the calling thread's context has finished. */
int bwtm_synchronize(void);
/* Peak number of bytes of device memory the context has held from the driver since the last call with reset != 0. */
uint64_t bwtm_device_bytes_peak(int reset);

/* Page-locked host memory: transfers from / to it run at PCIe speed and overlap with kernels
   (the BlockArray of the facade, support.h:90-150, allocates its bytes here). */
int bwtm_host_alloc(uint64_t nbytes, void** out);
void bwtm_host_free(void* p);

/* --- index: BWT::load + BWT::build (bwt.cpp:132-148, 476-512) on the device ------------ */

/* Uploads a run-length encoded BWT in the native byte format (the BlockArray of
   BWT::data, bwt.h:173) and builds the device rank structure from it.
   `C` may be NULL (then it is derived from the symbol counts like Alphabet(counts),
   support.cpp:84-91). */
int bwtm_index_upload(const uint8_t* data, uint64_t nbytes, uint64_t sequences, uint64_t bases,
                      const uint64_t C[BWTM_SIGMA + 1], bwtm_index** out);
/* The upload is chunked: the H2D copy of chunk k + 1 runs on the context's copy stream while the first
   decode pass of chunk k runs on its compute stream.  `C`, when given, must agree with the symbol
   counts of the stream (BWTM_EINVAL otherwise). */
/* The same index without the stream ever being resident on the device as a whole: the bytes travel in chunks of the upload_chunk knob
   (whole groups of 62 blocks) through a ring of at most three chunk buffers, and the records of chunk k are built while chunk k + 1 is on
   the link; the running position and symbol counts stay on the device, and the header is validated once, after the last chunk, with
   the verdicts of bwtm_index_upload (on failure the half-built index is freed).  The result holds records and super table only, like
   the result of bwtm_interleave: bwtm_index_bytes() is 0 until bwtm_index_encode().
   staging_bytes_peak: the largest sum of the device buffers the call held besides the records and the super table; it does not depend
   on nbytes (at most 4 x chunk_bytes + 64 KiB).  chunk_bytes: the upload_chunk knob in whole groups, no more than the stream's groups.
   `stats` may be NULL. */
typedef struct { uint64_t chunks, chunk_bytes, staging_bytes_peak; double ms_total; } bwtm_upload_stats;
int bwtm_index_upload_streamed(const uint8_t* data, uint64_t nbytes, uint64_t sequences, uint64_t bases,
                               const uint64_t C[BWTM_SIGMA + 1], bwtm_index** out, bwtm_upload_stats* stats /* may be NULL */);
/* Same, from a device buffer that already holds the native bytes (the bytes are copied). */
int bwtm_index_from_device(const void* device_data, uint64_t nbytes, uint64_t sequences, uint64_t bases,
                           const uint64_t C[BWTM_SIGMA + 1], bwtm_index** out);
/* Same, without the copy: the index reads the caller's device buffer in place (BWT::load without a
   second resident copy of BWT::data).  The buffer must be 16-byte aligned, readable up to the next
   multiple of 16 bytes after `nbytes`, and must stay valid and unmodified until the index is freed or
   bwtm_index_drop_native() is called (both wait for the library's queued readers). */
int bwtm_index_from_device_borrowed(const void* device_data, uint64_t nbytes, uint64_t sequences, uint64_t bases,
                                    const uint64_t C[BWTM_SIGMA + 1], bwtm_index** out);
/* Builds an index directly from a plain symbol string on the device (one comp value 0..5
   per byte, `bases` of them; sequences = number of 0 symbols).  Used by the input tooling. */
int bwtm_index_from_symbols_device(const void* device_symbols, uint64_t bases, bwtm_index** out);
void bwtm_index_free(bwtm_index* index);

uint64_t bwtm_index_bases(const bwtm_index* index);       /* BWT::size(),      bwt.h:108 */
uint64_t bwtm_index_sequences(const bwtm_index* index);   /* BWT::sequences(), bwt.h:109 */
uint64_t bwtm_index_bytes(const bwtm_index* index);       /* BWT::bytes(),     bwt.h:110 (0 until encoded) */
uint64_t bwtm_index_blocks(const bwtm_index* index);      /* number of 64-byte blocks */
void     bwtm_index_C(const bwtm_index* index, uint64_t C[BWTM_SIGMA + 1]);   /* Alphabet::C */

/* Makes sure the native byte stream (and its samples) exist on the device: runs the
   canonical run encoder (Run::write semantics, support.h:256-282) and the sample builder
   (BWT::build, bwt.cpp:476-512) if the index was produced by bwtm_interleave(). */
int bwtm_index_encode(bwtm_index* index);
/* Drops the native byte stream and samples, keeping only the device rank structure
   (what a chained merge needs as its next input). */
int bwtm_index_drop_native(bwtm_index* index);

/* The device buffer holding the native bytes (valid until the index is freed / dropped). */
int bwtm_index_device_data(bwtm_index* index, void** device_ptr, uint64_t* nbytes);
/* Copies the native bytes to the host (`capacity` >= bwtm_index_bytes()). */
int bwtm_index_download_data(bwtm_index* index, uint8_t* out, uint64_t capacity);
/* Samples in the form BWT::build computes them: block_end[blocks] = last sequence position
   of each block (the set bits of block_boundaries, bwt.h:176) and cum[6][blocks + 1]
   row-major = CumulativeArray::sum(k) of samples[c] (support.h:338-343). */
int bwtm_index_download_samples(bwtm_index* index, uint64_t* block_end, uint64_t* cum);
/* The same information in 12 or 24 instead of 56 bytes per block (the reference keeps it compressed too: seven
   sd_vectors).  FIELDS [6][blocks], `width` bytes each: positions in block k, then its occurrences of symbols 1..5;
   ANCHORS [6][ceil(blocks / 64)] of uint64: start position and counts of 1..5 before block 64 j.  Hence
     block_end[k]   = anchors[0][k / 64] + sum(fields[0][64 (k / 64) .. k]) - 1
     cum[c][k]      = anchors[c][k / 64] + sum(fields[c][64 (k / 64) .. k - 1])          (c = 1..5; c = 0: start - the five)
   bwtm_index_samples_width() tells the narrowest width that holds every field: 1, 2, 4, or 8 (= use the full arrays above);
   a stream of short runs (read collections: ~85 positions per block) takes 1. */
int bwtm_index_samples_width(bwtm_index* index, int* width);
int bwtm_index_download_samples_compact(bwtm_index* index, int width, void* fields, uint64_t* anchors);

/* Queries on the device structure (batch forms of BWT::rank, bwt.cpp:318-341, and
   BWT::inverse_select, bwt.cpp:445-464).  Arrays are host arrays of length `count`. */
int bwtm_rank_batch(const bwtm_index* index, const uint64_t* positions, const uint8_t* comps,
                    uint64_t count, uint64_t* out_ranks);
int bwtm_inverse_select_batch(const bwtm_index* index, const uint64_t* positions, uint64_t count,
                              uint64_t* out_ranks, uint8_t* out_comps);
/* Backward search of `count` patterns (FMI::find, fmi.h:195-209; what bwt_merge -v runs, bwt_merge.cpp:240-260).
   Pattern k is the comp values patterns[offsets[k] .. offsets[k + 1]); results are closed ranges
   [sp, ep], empty when sp > ep; the empty pattern matches [0, bases - 1].  offsets[0 .. count] must not decrease
   (BWTM_EINVAL names the first pattern whose end lies before its begin); patterns holds offsets[count] bytes. */
int bwtm_find_batch(const bwtm_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t count,
                    uint64_t* out_sp, uint64_t* out_ep);
/* Backward search of `count` patterns with up to max_mismatches (0..8) substitutions (bwtm_find_edit_batch allows insertions and deletions as well); no reverse complements.  Patterns are
   laid out as for bwtm_find_batch, comp values 1..5 (N's comp value is a symbol like the others); at most 65 535 symbols each.
   A HIT of a pattern P of m symbols is a string W of m comp values 1..5 that occurs inside a sequence (nothing spans an endmarker)
   and differs from P in at most max_mismatches places.  It is reported once, as (sp, count, mismatches): [sp, sp + count - 1] is
   the closed range bwtm_find_batch returns for W, ready for bwtm_locate_ranges, and mismatches the number of places.  Distinct hits
   have disjoint ranges.  The empty pattern has the single hit (0, bases, 0); with max_mismatches == 0 a pattern has one hit, the
   range of bwtm_find_batch, or none when that range is empty.
   ORDER: the hits of a pattern are ascending when the matched strings W are compared from their LAST symbol backwards (the order in
   which a backward search that tries the comp values 1..5 in turn meets them; nothing is sorted).  max_hits > 0 keeps the first
   max_hits hits of every pattern in that order.  The result is the same from run to run.
   hit_offsets[count + 1] always receives the exclusive prefix sums of the kept hits.  capacity == 0, or all three output arrays NULL:
   sizes only (the search still runs).  Otherwise capacity >= hit_offsets[count] (BWTM_EINVAL if not, and nothing is written) and the
   hits of pattern k occupy [hit_offsets[k], hit_offsets[k + 1]) of out_sp / out_count / out_mismatches, any of which may be NULL;
   nothing behind hit_offsets[count] is touched.
   The Hamming neighbours of a pattern share every prefix of the search: the patterns of a batch are one frontier of ranges, expanded
   level by level (two launches, one scan and one small read-back per level; as many levels as the longest pattern has symbols),
   and a branch dies when its range is empty.  The call works in batches of bwtm_tune("approx_batch") patterns (default 2^16, at
   most 2^28, 0 restores the default), because a frontier's size is known only once it has been counted.  Device memory beyond
   the index, per batch, with P = its largest frontier (at least its patterns), H = its hits before max_hits and T = the bytes of its
   pattern text: at most 240 P + 128 H + 2 T + 2^20 bytes while every block stays below 512 MiB (api/approx.hip.h derives it).
   A frontier or hit buffer that does not fit the device is BWTM_ENOMEM: lower approx_batch or max_mismatches.
   Works on any whole index, not on a window.  BWTM_EINVAL, bwtm_last_error() naming the first offender: a null argument, a window
   of an index, max_mismatches > 8, offsets that decrease, a pattern longer than 65 535 symbols, a pattern symbol outside 1..5. */
int bwtm_find_approx_batch(const bwtm_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t count,
                           uint32_t max_mismatches, uint64_t max_hits, uint64_t* hit_offsets /* count + 1 */,
                           uint64_t* out_sp, uint64_t* out_count, uint8_t* out_mismatches, uint64_t capacity);
/* What the calling thread's last bwtm_find_approx_batch did: stats[0] = nodes expanded (the sizes of all frontiers, every batch
   once), stats[1] = P and stats[2] = H of the formula above (the largest over the batches), stats[3] = levels run. */
int bwtm_find_approx_stats(uint64_t stats[4]);
/* Backward search of `count` patterns within edit distance max_edits (0..7): insertions, deletions and substitutions at a cost of 1
   each; no reverse complements.  Patterns are laid out as for bwtm_find_approx_batch, comp values 1..5 (N's comp value is a symbol
   like the others); at most 65 535 symbols each.
   A HIT of a pattern P of m symbols is a string W of comp values 1..5 that occurs inside a sequence (nothing spans an endmarker)
   and whose Levenshtein distance ed(W, P) is <= max_edits; the alignment is global on both sides, the whole of W against the whole
   of P.  It is reported once, as (sp, count, edits, length): [sp, sp + count - 1] is the closed range bwtm_find_batch returns for W,
   ready for bwtm_locate_ranges, edits is ed(W, P) itself (the minimum, not the cost of the path that found W) and length is |W|,
   m - max_edits <= |W| <= m + max_edits.  The ranges of distinct hits are disjoint or nested: W and Wx may both be hits.  When
   m <= max_edits the empty string is a hit, (0, bases, m, 0).  With max_edits == 0 a pattern has one hit, the range of
   bwtm_find_batch with edits = 0 and length = m, or none when that range is empty.
   ORDER: the hits of a pattern come shortest W first and, within one length, ascending when the strings W are compared from their
   LAST symbol backwards (the order of bwtm_find_approx_batch, per length; nothing is sorted).  max_hits > 0 keeps the first max_hits
   hits of every pattern in that order.  The result is the same from run to run.
   hit_offsets[count + 1] always receives the exclusive prefix sums of the kept hits.  capacity == 0, or all four output arrays NULL:
   sizes only (the search still runs).  Otherwise capacity >= hit_offsets[count] (BWTM_EINVAL if not, and nothing is written) and the
   hits of pattern k occupy [hit_offsets[k], hit_offsets[k + 1]) of out_sp / out_count / out_edits / out_lengths, any of which may be
   NULL; nothing behind hit_offsets[count] is touched.
   The strings near a pattern share every suffix of the search: W is built backwards, and its node carries the column
   ed(W, last i symbols of P) for |i - |W|| <= 7.  A child is kept while its range is not empty and the least entry of its column
   is within the budget, and is a hit when the entry of i = m is; the patterns of a batch are one frontier, expanded level by level
   (two launches, one scan and one small read-back per level; at most longest pattern + max_edits levels).  The call works in batches of
   bwtm_tune("approx_batch") patterns, as bwtm_find_approx_batch does, and a call of several batches searches each of them twice.
   Device memory beyond the index, per batch, with P = its largest frontier (at least its patterns), H = its hits before max_hits,
   T = the bytes of its pattern text and e = max_edits: at most (308 + 34 e) P + 132 H + 2 T + 2^20 bytes while every block stays
   below 512 MiB (api/edit.hip.h derives it).  A frontier or hit buffer that does not fit the device is BWTM_ENOMEM: lower
   approx_batch or max_edits.
   Works on any whole index, not on a window.  BWTM_EINVAL, bwtm_last_error() naming the first offender: a null argument, a window
   of an index, max_edits > 7, offsets that decrease, a pattern longer than 65 535 symbols, a pattern symbol outside 1..5. */
int bwtm_find_edit_batch(const bwtm_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t count,
                         uint32_t max_edits, uint64_t max_hits, uint64_t* hit_offsets /* count + 1 */,
                         uint64_t* out_sp, uint64_t* out_count, uint8_t* out_edits, uint32_t* out_lengths, uint64_t capacity);
/* What the calling thread's last bwtm_find_edit_batch did: stats[0] = nodes expanded (the sizes of all frontiers, every batch
   once), stats[1] = P and stats[2] = H of the formula above (the largest over the batches), stats[3] = levels run. */
int bwtm_find_edit_stats(uint64_t stats[4]);
/* Which pieces of a pattern occur at all, and how long they are: matching statistics and maximal exact matches (MEMs), the seeds of
   seed-and-extend.  Patterns are laid out as for bwtm_find_batch: pattern k = patterns[offsets[k] .. offsets[k+1]), comp values 1..5
   (N's comp value is a symbol like the others), at most 65 535 symbols each; no reverse complements.  "W occurs" means that
   bwtm_find_batch returns a non-empty range for W: W lies inside a sequence, nothing spans an endmarker.
   MATCHING STATISTICS of a pattern P of m symbols: for an end e in 1..m, l(e) is the largest l <= e such that P[e-l .. e) occurs, and 0
   when P[e-1] alone does not.  The entry of symbol position i = e - 1 is (length, sp, count): length = l(e), and [sp, sp + count - 1]
   is the closed range bwtm_find_batch returns for P[e-l .. e); (0, 0, 0) when l(e) = 0.  The entries of all patterns lie at index
   offsets[k] + i - offsets[0], one per symbol of the text: each output holds offsets[count] - offsets[0] entries.  Any of the three
   outputs may be NULL, not all.
   A MAXIMAL EXACT MATCH of P is a pair (b, l) with l >= min_length >= 1 such that P[b .. b+l) occurs, b == 0 or P[b-1 .. b+l) does not
   occur, and b + l == m or P[b .. b+l+1) does not occur: the substrings of P that occur and are contained in no longer substring of P
   that occurs (BWA's super-maximal exact matches, stated on the pattern).  End e gives one iff l(e) >= min_length and (e == m or
   l(e+1) <= l(e)); l(e+1) <= l(e) + 1 always holds.  A pattern has at most m MEMs; their begins and their ends both ascend strictly,
   and they are reported in that order as (begin, length, sp, count), the range ready for bwtm_locate_ranges.  The empty pattern has
   none.  The result is the same from run to run.
   hit_offsets[count + 1] always receives the exclusive prefix sums of the MEMs per pattern.  capacity == 0, or all four output arrays
   NULL: sizes only (the search still runs).  Otherwise capacity >= hit_offsets[count] (BWTM_EINVAL if not, and nothing is written)
   and the MEMs of pattern k occupy [hit_offsets[k], hit_offsets[k + 1]) of out_begin / out_length / out_sp / out_count, any of which
   may be NULL; nothing behind hit_offsets[count] is touched.
   The statistics take one backward search per symbol of the text, four lanes each, which keeps its last range that is not empty.  The
   MEMs take four lanes per pattern: its ends are searched from m downwards, an end gives a MEM iff its search gets below the begin of
   the search before, and the pattern is finished when a search reaches its begin.  Both calls work in batches of bwtm_tune("mem_batch") patterns (default 2^20, at most 2^28, 0 restores the default),
   cut at pattern boundaries; a batch also ends before its text reaches 2^29 symbols.  Device memory beyond the index, per batch of B
   patterns with T symbols of text and M MEMs kept: at most 21 T + 8 B + 2^24 bytes (bwtm_matching_stats_batch) and
   29 T + 28 M + 16 B + 2^25 bytes (bwtm_mem_batch) while every block stays below 512 MiB (api/mem.hip.h derives it).  A
   bwtm_mem_batch call of several batches runs the search of each batch twice (once for the sizes, once before it emits).
   Measured on an MI355X, 3.03 Gbase index, 2^16 patterns of 100 symbols cut from its reads, unchanged / 1 % / 5 % substituted
   (tools/mem_bench.py): the statistics 160 / 151 / 111 ns per pattern, the MEMs at min_length 1
   32.5 / 131.5 / 133.8 ns per pattern.  Not measured: longer patterns, patterns foreign to the index, calls of several batches.
   Work on any whole index, not on a window.  BWTM_EINVAL, bwtm_last_error() naming the first offender: a null argument, a window of
   an index, min_length == 0, offsets that decrease, a pattern longer than 65 535 symbols, a pattern symbol outside 1..5. */
int bwtm_matching_stats_batch(const bwtm_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t count,
                              uint32_t* out_lengths, uint64_t* out_sp, uint64_t* out_count);
int bwtm_mem_batch(const bwtm_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t count, uint32_t min_length,
                   uint64_t* hit_offsets /* count + 1 */, uint32_t* out_begin, uint32_t* out_length, uint64_t* out_sp,
                   uint64_t* out_count, uint64_t capacity);
/* What the calling thread's last call of either did: stats[0] = LF steps taken (pairs of ranks; every batch once), stats[1] = tasks
   run (bwtm_matching_stats_batch: the symbols of the text, one search each; bwtm_mem_batch: the patterns), stats[2] = MEMs before min_length (0 after bwtm_matching_stats_batch), stats[3] = batches. */
int bwtm_mem_stats(uint64_t stats[4]);
/* Plain symbols [first, first + count) (BWT::extract, bwt.h:134-164), one byte each.  first <= bases and
   count <= bases - first, or BWTM_EINVAL (a sum that wraps included); first == bases with count == 0 is accepted. */
int bwtm_extract(const bwtm_index* index, uint64_t first, uint64_t count, uint8_t* out);
/* Sequences of the collection by id, as plain comp values 1..5 in forward order, endmarkers not included.
   ids == NULL: the ids first_id .. first_id + count - 1; otherwise ids[0 .. count) in any order, repeats allowed (first_id ignored).
   offsets[count + 1] always receives the exclusive prefix sums of the lengths (offsets[count] = bytes of text).
   text == NULL or capacity == 0: sizes only.  Otherwise capacity >= offsets[count] (BWTM_EINVAL if not) and sequence j
   occupies text[offsets[j] .. offsets[j + 1]); bytes beyond offsets[count] are not touched.
   max_len: no sequence may be longer (0: 65536; at most 2^24); a longer one, or an id >= sequences, is BWTM_EINVAL and
   bwtm_last_error() names the first offending id.  Works on any whole index (uploaded, merged, built; records suffice),
   not on a window.  The call works in batches of the extract_batch knob (2^20 sequences): its device memory beyond the
   index is that of one batch. */
int bwtm_sequences_extract(const bwtm_index* index, const uint64_t* ids, uint64_t first_id, uint64_t count, uint64_t max_len,
                           uint64_t* offsets, uint8_t* text, uint64_t capacity);

/* From BWT positions back to the collection: position p is the suffix that starts at offset o of sequence id (o = the length
   of the sequence: its endmarker suffix, p < sequences).  A locator is one table of `sequences` 64-bit entries on the device
   (bwtm_locator_bytes; 8 GB for 10^9 reads), built by one LF walk per sequence; a located position costs one walk to the
   start of its sequence and one table entry.  Works on any whole index (uploaded, merged, built; records suffice), not on
   a window.  max_len as in bwtm_sequences_extract (0: 65536; at most 2^24): a longer sequence is BWTM_EINVAL and
   bwtm_last_error() names it; an index whose walks do not give every sequence a start of its own is refused as damaged.
   The locator BORROWS the index: the index must outlive it and must not be consumed (bwtm_merge_consume) meanwhile; after a
   merge, build a new locator on the result.  The build and the locate calls work in batches of the locate_batch knob (2^20
   sequences / hits, at most 2^28): device memory beyond the index and the table is that of one batch. */
typedef struct bwtm_locator bwtm_locator;
int bwtm_locator_create(const bwtm_index* index, uint64_t max_len, bwtm_locator** out);
void bwtm_locator_free(bwtm_locator* locator);
uint64_t bwtm_locator_bytes(const bwtm_locator* locator);          /* device bytes of the table */
/* (out_ids[k], out_offsets[k]) of positions[k]; a position >= bases is BWTM_EINVAL and bwtm_last_error() names it. */
int bwtm_locate_batch(const bwtm_locator* locator, const uint64_t* positions, uint64_t count,
                      uint64_t* out_ids, uint64_t* out_offsets);
/* The positions of `count` closed ranges [sp, ep] in bwtm_find_batch's convention (sp > ep: empty; ep >= bases in a
   non-empty range is BWTM_EINVAL).  max_hits > 0 keeps the first max_hits positions of every range.  hit_offsets[count + 1]
   always receives the exclusive prefix sums of the kept hit counts.  out_ids == NULL or capacity == 0: sizes only, no GPU
   work.  Otherwise capacity >= hit_offsets[count] (BWTM_EINVAL if not) and the hits of range r occupy
   [hit_offsets[r], hit_offsets[r + 1]) of out_ids / out_offsets in ascending BWT position; nothing behind
   hit_offsets[count] is touched.  The positions are generated on the device. */
int bwtm_locate_ranges(const bwtm_locator* locator, const uint64_t* sp, const uint64_t* ep, uint64_t count,
                       uint64_t max_hits, uint64_t* hit_offsets /* count + 1 */,
                       uint64_t* out_ids, uint64_t* out_offsets, uint64_t capacity);

/* Suffix-prefix overlaps, the overlap step of a string-graph assembler: a hit of a query Q of L symbols is a pair (t, l) with
   min_overlap <= l <= L, l <= |S_t| and S_t[0 .. l) == Q[L - l .. L).  l == |S_t| is a hit (S_t is a suffix of Q), and when Q is
   sequence q of the index, (q, L) is one too; a sequence that overlaps itself with l < L is an ordinary hit.  Reverse complements
   are not searched: an index that holds both strands gives them.  The hits of a query come longest overlap first and, within one
   length, in ascending BWT position of the target's whole-sequence suffix (targets ascending as strings, a prefix before its
   extensions, equal ones by id).  max_hits > 0 keeps the first max_hits hits of every query in that order: the longest.
   One backward search per query and one table entry per hit: no walk.
   hit_offsets[count + 1] always receives the exclusive prefix sums of the kept hit counts.  out_ids == NULL or capacity == 0:
   sizes only -- unlike bwtm_locate_ranges, that call does run the search (its count pass) on the GPU.  Otherwise
   capacity >= hit_offsets[count] (BWTM_EINVAL if not, and nothing beyond hit_offsets is written) and the hits of query k occupy
   [hit_offsets[k], hit_offsets[k + 1]) of out_ids (the target t) / out_lengths (l); nothing behind hit_offsets[count] is touched.
   BWTM_EINVAL, with bwtm_last_error() naming the first offender: min_overlap == 0, a query symbol outside 1..5, offsets that
   decrease, an id >= sequences, a sequence longer than the locator's max_len, an entry of the table that is no sequence.  A query
   shorter than min_overlap has no hits; a pattern may be longer than every sequence.  The calls work in batches of the
   overlap_batch knob (2^20 queries, at most 2^28) and expand in hit batches of locate_batch: device memory beyond the index and
   the table is one batch's text, 24 bytes per query, its interval records (32 bytes each, at most one per symbol of the text) and one
   batch of hits.
   A call of more than one batch runs the count pass of every batch twice (once for the sizes, once before its expansion). */
/* queries as patterns: query k = queries[offsets[k] .. offsets[k+1]), comp values 1..5 */
int bwtm_overlap_batch(const bwtm_locator* locator, const uint8_t* queries, const uint64_t* offsets, uint64_t count,
                       uint64_t min_overlap, uint64_t max_hits, uint64_t* hit_offsets /* count + 1 */,
                       uint64_t* out_ids, uint64_t* out_lengths, uint64_t capacity);
/* queries are sequences of the index itself, read on the device and never brought to the host: ids == NULL: first_id ..
   first_id + count - 1, otherwise ids[0 .. count) in any order, repeats allowed (the conventions of bwtm_sequences_extract) */
int bwtm_overlap_sequences(const bwtm_locator* locator, const uint64_t* ids, uint64_t first_id, uint64_t count,
                           uint64_t min_overlap, uint64_t max_hits, uint64_t* hit_offsets,
                           uint64_t* out_ids, uint64_t* out_lengths, uint64_t capacity);

/* The distinct k-mers of the collection with their counts: the question an assembler or a QC step asks before it computes overlaps
   (coverage peak, genome size, the solid / weak threshold of error correction).  `skip` is one comp value 1..5, the comp of N (5 in
   the default alphabet, 4 in the sorted one); the four other comp values, ranked 0..3 in ascending order, are the k-mer alphabet.
   A k-mer (1 <= k <= 32) is a string of k such symbols; its COUNT is the number of pairs (i, o) with S_i[o .. o + k) equal to it
   (occurrences inside sequences: nothing spans an endmarker, a sequence shorter than k contributes nothing); its CODE holds 2 bits
   per symbol, the first symbol in the highest used bits, so codes compare like the strings; its RANGE is the closed BWT range
   [sp, sp + count - 1] of the suffixes that start with it, the one bwtm_find_batch returns for it and bwtm_locate_ranges takes.
   min_count (0 is taken as 1) keeps the k-mers whose count is at least min_count.  The result lists the kept k-mers in ascending
   code order, which is ascending sp order as well, and lives on the device; it does not borrow the index once created.
   The suffix trie is expanded level by level on the device: 2 (k - 1) launches over frontiers of 24 bytes per node and one small
   read-back per level.  Works on any whole index (uploaded, merged, built; records and super table suffice), not on a window.
   Device memory of the call beyond the index, with P = the largest entry of bwtm_kmers_levels: at most 240 P + 2^20 bytes while
   every block stays below 512 MiB (api/kmers.hip.h derives it); the handle keeps 24 bytes per kept k-mer.  A result that does not
   fit the device is BWTM_ENOMEM: raise min_count or lower k.
   BWTM_EINVAL, bwtm_last_error() saying which: k == 0 or k > 32, skip outside 1..5, a window of an index, first + count beyond
   bwtm_kmers_distinct (a sum that wraps included), bins < 2. */
typedef struct bwtm_kmers bwtm_kmers;
int bwtm_kmers_create(const bwtm_index* index, uint32_t k, uint32_t skip, uint64_t min_count, bwtm_kmers** out);
void bwtm_kmers_free(bwtm_kmers* kmers);
uint64_t bwtm_kmers_distinct(const bwtm_kmers* kmers);             /* kept k-mers */
uint64_t bwtm_kmers_total(const bwtm_kmers* kmers);                /* sum of their counts */
uint64_t bwtm_kmers_bytes(const bwtm_kmers* kmers);                /* device bytes the handle holds */
/* nodes[t] (t = 0 .. k - 1) = number of distinct (t + 1)-mers with count >= min_count: the frontier after each level; 0 behind k */
int bwtm_kmers_levels(const bwtm_kmers* kmers, uint64_t nodes[32]);
/* entries [first, first + count) in code order; any of the three output arrays may be NULL */
int bwtm_kmers_download(const bwtm_kmers* kmers, uint64_t first, uint64_t count,
                        uint64_t* codes, uint64_t* counts, uint64_t* sp);
/* hist[j] = number of kept k-mers of count j for j < bins - 1; hist[bins - 1] = those of count >= bins - 1; bins >= 2 */
int bwtm_kmers_histogram(const bwtm_kmers* kmers, uint64_t bins, uint64_t* hist);

/* The k-mers of TWO collections side by side: which k-mers a and b share and which only one of them holds (sample against sample,
   reads against a reference, a new batch against the index it is about to be merged into).  k, skip, codes and counts are those
   of bwtm_kmers_create.  Both suffix tries are walked down together, so every entry carries, for each index x, its count cnt_x
   and sp_x: the first position of its BWT range in x when cnt_x > 0 (the range bwtm_find_batch returns), and otherwise its
   INSERTION POINT, the number of suffixes of x that are smaller than the k-mer.  For the merged index of a and b the k-mer's
   count is cnt_a + cnt_b and its sp is sp_a + sp_b.
   A k-mer is kept when  min_a <= cnt_a <= max_a,  min_b <= cnt_b <= max_b  and  cnt_a + cnt_b >= min_sum.  min_a and min_b may
   be 0 (the k-mer may be absent there); a min_sum of 0 is taken as 1 (a k-mer neither index holds is never listed); max_x ==
   UINT64_MAX is no bound.  All defaults (0, UINT64_MAX, 0, UINT64_MAX, 1): the union with both counts.  min_a = min_b = 1: the
   shared k-mers.  min_b = m, max_a = 0: in b at least m times and absent from a.  The lower bounds prune every level of the walk,
   the upper bounds act at level k only.
   The result lists the kept k-mers in ascending code order, which is ascending sp_a and ascending sp_b as well (both non-strict),
   and lives on the device; it does not borrow the indexes once created.  a and b may be the same handle: then both sides are equal.
   The walk is 2 (k - 1) launches over frontiers of 40 bytes per node and one small read-back per level.  Works on any two whole
   indexes of one context (uploaded, merged, built; records and super table suffice), not on a window.
   Device memory of the call beyond the two indexes, with P = the largest entry of bwtm_kmer_join_levels: at most 392 P + 2^20
   bytes while every block stays below 512 MiB (api/kmer_join.hip.h derives it); the handle keeps 40 bytes per kept k-mer and
   nothing else.  A result that does not fit the device is BWTM_ENOMEM: raise a lower bound or lower k.
   BWTM_EINVAL, bwtm_last_error() naming the first offender: a null argument, a window of an index on either side, indexes of
   different contexts, k == 0 or k > 32, skip outside 1..5, min_a > max_a, min_b > max_b, first + count beyond
   bwtm_kmer_join_distinct (a sum that wraps included). */
typedef struct bwtm_kmer_join bwtm_kmer_join;
int bwtm_kmer_join_create(const bwtm_index* a, const bwtm_index* b, uint32_t k, uint32_t skip,
                          uint64_t min_a, uint64_t max_a, uint64_t min_b, uint64_t max_b, uint64_t min_sum,
                          bwtm_kmer_join** out);
void bwtm_kmer_join_free(bwtm_kmer_join* join);
uint64_t bwtm_kmer_join_distinct(const bwtm_kmer_join* join);      /* kept k-mers */
uint64_t bwtm_kmer_join_bytes(const bwtm_kmer_join* join);         /* device bytes the handle holds */
/* nodes[t] for t < k - 1 = the (t + 1)-mers the lower bounds keep: the frontier after each level; nodes[k - 1] = the result, after
   the upper bounds as well; 0 behind k */
int bwtm_kmer_join_levels(const bwtm_kmer_join* join, uint64_t nodes[32]);
/* entries [first, first + count) in code order; any of the five output arrays may be NULL */
int bwtm_kmer_join_download(const bwtm_kmer_join* join, uint64_t first, uint64_t count,
                            uint64_t* codes, uint64_t* count_a, uint64_t* count_b, uint64_t* sp_a, uint64_t* sp_b);
/* Over the kept k-mers: stats[0], [1], [2] = those only in a (cnt_b == 0), only in b (cnt_a == 0), in both; stats[3] = the
   occurrences in a of the first class, stats[4] = those in b of the second, stats[5], stats[6] = those in a and in b of the third */
int bwtm_kmer_join_summary(const bwtm_kmer_join* join, uint64_t stats[7]);

/* K-mer error correction of reads against the spectrum, the step of a string-graph assembler between counting k-mers and computing
   overlaps: every read is made to consist of SOLID k-mers by single substitutions, on the device.  k (1..32), `skip` (the comp of N)
   and the codes are those of bwtm_kmers_create; the kept alphabet is the four comp values other than skip.  threshold t >= 1 (0 is
   taken as 1); max_rounds R, 0 <= R <= 65535.
   A window of k symbols is solid when it holds no skip symbol and its k-mer has count >= t in the table.  Position i of a read of m
   symbols is COVERED when some solid window that starts at o contains it, max(0, i - k + 1) <= o <= min(i, m - k).  The rule for a
   read S:
     1. m < k: status SHORT, text unchanged, edits 0.
     2. r = 0, edits = 0, W a copy of S.  Repeat:
        a. every position of W covered: stop, status CLEAN if edits == 0, else CORRECTED; the text is W.
        b. r == R: stop with FAILED.  Otherwise r += 1.
        c. the uncovered positions i in ascending order; for each the window start o = max(0, i - k + 1) and after it
           o = min(i, m - k) if that differs.  The candidates are the kept symbols c != W[i] for which the window at o with c
           written at i is solid (a skip symbol elsewhere in the window: none).  The first (i, o) with EXACTLY ONE candidate sets
           W[i] = c, edits += 1, and the next round begins.
        d. no (i, o) had exactly one candidate: stop with FAILED.
     3. FAILED returns the original text S and edits 0: nothing of a partial correction leaves the call.
   One substitution per round; W[i] may be skip itself, so an N is corrected like any other symbol; reads are independent of each
   other.  Reverse complements are not looked at: an index that holds both strands gives them.
   The corrector COPIES the codes of the k-mers of count >= threshold out of the k-mer handle, which may be freed at once, and builds
   a bucket directory over their top bits: with S = bwtm_corrector_solid and D = min(2 k, 24, max(1, ceil(log2 S))), bucket b is the
   range of codes whose top D of their 2 k used bits equal b, and the handle holds 8 max(S, 1) + 8 (2^D + 1) bytes plus what the pool
   rounds up (a block of 1 MiB or more to 64 KiB, of 64 MiB or more to 2 MiB, a smaller one to 256 bytes; two blocks; a block of 512 MiB or
   more, S above 2^26, is made of whole chunks of 1 GiB: bwtm_corrector_bytes reports what is held).  While it is
   created, 8 bytes per k-mer of the k-mer handle are held besides.  A k-mer handle created with a min_count above threshold simply
   lacks the k-mers below min_count: they are not solid.  `skip` MUST be the skip the k-mer handle was created with: the handle does
   not record it, so a different value cannot be refused, and it would read every code in another alphabet.  An empty table (S == 0) is valid: every read of k symbols or more FAILS.
   Both correct calls work in batches of bwtm_tune("correct_batch") reads (default 2^20, at most 2^28).  Device memory of a call
   beyond the table and the index, with B = reads and T = bytes of text of the largest batch: at most 17/8 T + 27 (B + 1) + 2^16
   bytes while every block stays below 512 MiB (api/correct.hip.h derives it): the batch's text and its working copy, offsets,
   status, edits and, for bwtm_correct_sequences, the extract stage of bwtm_sequences_extract.
   BWTM_EINVAL, bwtm_last_error() naming the first offender: a null argument, skip outside 1..5, max_rounds > 65535, offsets that
   decrease, a symbol outside 1..5, a window of an index, an id >= sequences, a sequence longer than max_len, a corrector and an
   index of different contexts, a capacity that is too small. */
#define BWTM_CORRECT_CLEAN 0
#define BWTM_CORRECT_CORRECTED 1
#define BWTM_CORRECT_FAILED 2
#define BWTM_CORRECT_SHORT 3
typedef struct bwtm_corrector bwtm_corrector;
int bwtm_corrector_create(const bwtm_kmers* kmers, uint32_t skip, uint64_t threshold, bwtm_corrector** out);
void bwtm_corrector_free(bwtm_corrector* corrector);
uint64_t bwtm_corrector_solid(const bwtm_corrector* corrector);    /* k-mers of count >= threshold */
uint64_t bwtm_corrector_bytes(const bwtm_corrector* corrector);    /* device bytes the handle holds */
uint32_t bwtm_corrector_k(const bwtm_corrector* corrector);
/* Reads from the host, laid out as for bwtm_find_batch: read j = patterns[offsets[j] .. offsets[j + 1]), comp values 1..5, a read
   may be empty.  out_text has the input's layout (the same offsets); out_status[j] is one of BWTM_CORRECT_*, out_edits[j] the
   substitutions made in read j.  Any of the three outputs may be NULL. */
int bwtm_correct_batch(const bwtm_corrector* corrector, const uint8_t* patterns, const uint64_t* offsets, uint64_t count,
                       uint32_t max_rounds, uint8_t* out_text, uint8_t* out_status, uint32_t* out_edits);
/* Reads of an index, extracted and corrected on the device; ids / first_id / count / max_len / offsets / text / capacity as in
   bwtm_sequences_extract.  offsets, text, out_status and out_edits may be NULL in any combination.  text == NULL or capacity == 0 is
   a status call: the correction still runs, offsets, status and edits are filled, no text comes back.  Otherwise capacity >=
   offsets[count] (BWTM_EINVAL if not): max_len and the capacity are checked before anything is written, so a refused call leaves
   offsets, text, status and edits as they were (size the text with a status call, or with bwtm_sequences_extract); nothing behind
   offsets[count] is touched.  A call of more than one batch walks every sequence twice (once for the lengths, once for the
   text). */
int bwtm_correct_sequences(const bwtm_corrector* corrector, const bwtm_index* index, const uint64_t* ids, uint64_t first_id,
                           uint64_t count, uint64_t max_len, uint32_t max_rounds, uint64_t* offsets /* count + 1 */,
                           uint8_t* text, uint64_t capacity, uint8_t* out_status, uint32_t* out_edits);
/* What the calling thread's last correct call did: stats[0] = table lookups, stats[1] = rounds run over all reads, stats[2] = the
   most edits in one read, stats[3] = batches. */
int bwtm_correct_stats(uint64_t stats[4]);

/* The unitigs of the k-mer graph, the step of an assembler behind counting and correcting: the compacted de Bruijn graph over the
   solid k-mers of a spectrum, with its coverage and links, built on the device.  k (1..32), `skip` (the comp of N), the codes and
   the counts are those of bwtm_kmers_create; threshold t >= 1 (0 is taken as 1).  Reverse complements are not looked at: an index
   that holds both strands gives them.
   NODES.  The k-mers of the handle with count >= t: S of them, in ascending code order; node index = rank in that order.
   EDGES.  x -> y when both are nodes and the last k - 1 symbols of x are the first k - 1 of y (k = 1: every node has an edge to
   every node).  out(x) and in(x) are the numbers of such edges, 0..4; a self-loop counts in both.  An edge x -> y is COMPACTABLE
   when out(x) == 1 and in(y) == 1.  Every node therefore has at most one compactable edge in and one out: the compactable edges
   form disjoint paths and disjoint cycles.
   UNITIGS.  Each path is one unitig; a single node with no compactable edge is a path of one.  Each cycle is one unitig with
   BWTM_UNITIG_CIRCULAR set; it begins at the cycle's node of smallest code and runs once around.  Every node lies in exactly one
   unitig, at exactly one offset.  A unitig of n nodes has a text of n + k - 1 comp values: the first node's k symbols, then the
   last symbol of every further node (for a circular unitig the last k - 1 symbols repeat the first k - 1).  Its occurrences are
   the sum of its nodes' counts.  Unitigs are numbered in ascending code order of their first node: U of them.
   LINKS.  links[4 u + r] is the unitig that BEGINS with the node reached from unitig u's last node by appending the kept symbol
   of rank r (the r-th of the four comp values other than skip), UINT64_MAX when that k-mer is not a node.  Every non-compactable
   edge x -> y has x last in its unitig and y first in its unitig, so the links of all unitigs are all the non-compactable edges of
   the graph.  A circular unitig has four UINT64_MAX.  A unitig may link to itself: a cycle entered by a tail is a linear unitig
   that begins at the join node, and its last node links back to it.
   The handle COPIES what it needs out of the k-mer handle, which may be freed at once.  A k-mer handle created with a min_count
   above the threshold simply lacks the k-mers below min_count: they are no nodes.  `skip` MUST be the skip the k-mer handle was
   created with (the handle does not record it).  S == 0 is valid and gives U == 0.  Two runs give the same bytes.
   Memory (api/unitigs.hip.h derives both).  With Y = bwtm_unitigs_symbols = S + (k - 1) U and D = min(2 k, 24, max(1, ceil(log2 S)))
   the handle keeps H = 8 max(S, 1) + 8 (2^D + 1) + 16 S + 57 U + 8 + Y bytes in ten blocks -- the corrector's table of the nodes,
   unitig and offset of every node, and per unitig the text offsets, node counts, occurrences, flags, links and the text -- plus
   what the pool rounds up: bwtm_unitigs_bytes <= 9/8 (17/16 H + 2560).  bwtm_unitigs_create takes, handle included, at most
   17/16 (H + 8 n + 25 S + 8 U + C + (n + 2 S + U) / 128) + 2^16 bytes of device memory while every block stays below 512 MiB: n =
   the k-mers of the k-mer handle, C = 32 S when some node lies on a cycle of compactable edges only, else 0.  A result that
   does not fit the device is BWTM_ENOMEM.  The time of the call grows with the longest unitig (one dependent load per node of
   it): bwtm_unitigs_stats reports its length.
   BWTM_EINVAL, bwtm_last_error() naming the first offender: a null argument (the handle, `out`, the codes of a place call), skip
   outside 1..5, first + count beyond U (a sum that wraps included), a capacity that is too small. */
#define BWTM_UNITIG_CIRCULAR 1
typedef struct bwtm_unitigs bwtm_unitigs;
int bwtm_unitigs_create(const bwtm_kmers* kmers, uint32_t skip, uint64_t threshold, bwtm_unitigs** out);
void bwtm_unitigs_free(bwtm_unitigs* unitigs);
uint64_t bwtm_unitigs_count(const bwtm_unitigs* unitigs);      /* U */
uint64_t bwtm_unitigs_nodes(const bwtm_unitigs* unitigs);      /* S */
uint64_t bwtm_unitigs_symbols(const bwtm_unitigs* unitigs);    /* the sum of n_u + k - 1 */
uint64_t bwtm_unitigs_bytes(const bwtm_unitigs* unitigs);      /* device bytes the handle holds */
uint32_t bwtm_unitigs_k(const bwtm_unitigs* unitigs);
/* The unitigs [first, first + count): offsets (count + 1 entries, starting at 0: unitig first + j has the text
   text[offsets[j] .. offsets[j + 1])), text (capacity >= offsets[count]), nodes, occurrences and flags (count entries each), links
   (4 per unitig, numbered in the whole graph).  Every output may be NULL.  text == NULL or capacity == 0 is a sizing call: the
   other outputs are filled, no text comes back.  The range and the capacity are checked before anything is written: a refused
   download writes nothing. */
int bwtm_unitigs_download(const bwtm_unitigs* unitigs, uint64_t first, uint64_t count, uint64_t* offsets, uint8_t* text,
                          uint64_t capacity, uint64_t* nodes, uint64_t* occurrences, uint8_t* flags, uint64_t* links);
/* Where k-mers sit in the graph: unitig[j] and offset[j] = the unitig of codes[j] and the offset of that node in it, UINT64_MAX
   twice for a code that is no node (a code of 4^k or more among them).  Either output may be NULL. */
int bwtm_unitigs_place(const bwtm_unitigs* unitigs, const uint64_t* codes, uint64_t count, uint64_t* unitig, uint64_t* offset);
/* What the calling thread's last bwtm_unitigs_create did: stats[0] = table lookups, stats[1] = the longest unitig in nodes,
   stats[2] = nodes in circular unitigs, stats[3] = rounds of pointer jumping (0 when no node lies on a cycle of compactable
   edges only). */
int bwtm_unitigs_stats(uint64_t stats[4]);

/* --- rank array: buildRA + mergeRA + RankArray (fmi.cpp:139-334, support.h:576-638) ---- */

/* An empty rank array for inserting `b` into `a`. */
int bwtm_ra_create(const bwtm_index* a, const bwtm_index* b, bwtm_ra** out);
/* Same, but the interleaving bitvector lives in a caller-owned, ZEROED device buffer of at
   least bwtm_ra_buffer_bytes(a, b) bytes (e.g. a tensor that a collective library can reduce
   in place).  The buffer must outlive the rank array. */
uint64_t bwtm_ra_buffer_bytes(const bwtm_index* a, const bwtm_index* b);
int bwtm_ra_create_on(const bwtm_index* a, const bwtm_index* b, void* device_buffer, uint64_t nbytes, bwtm_ra** out);
void bwtm_ra_free(bwtm_ra* ra);
/* Search phase for the sequences [seq_first, seq_last] of b (closed range, like the
   sequence blocks of ParallelLoop, utils.cpp:169-209).  May be called for several
   disjoint ranges (e.g. one range per GPU); results accumulate in `ra`. */
int bwtm_search(const bwtm_index* a, const bwtm_index* b, uint64_t seq_first, uint64_t seq_last, bwtm_ra* ra);
/* The device buffer that holds the rank array as the interleaving bitvector (bit i + RA[i]
   set for every position i of b; 64-bit words, little-endian bit order) so that shards
   computed on different GPUs can be combined with one collective (sum == or, set bits are
   disjoint). */
int bwtm_ra_device_buffer(bwtm_ra* ra, void** device_ptr, uint64_t* nbytes);
/* ra |= the interleaving bitvector of another rank array for the same inputs that lives ON THE SAME DEVICE (shards
   searched into separate buffers, e.g. by two contexts of one GPU); across devices use a collective on
   bwtm_ra_device_buffer().  Blocking. */
int bwtm_ra_or_from(bwtm_ra* ra, const void* device_bits, uint64_t nbytes);
/* Cross-check of two searches over the same inputs (e.g. a shard of the sequences walked per chain against the whole collection
   searched level by level): the number of set bits of `part` and the number of 64-bit words in which `part` has a bit that `whole`
   lacks (must be 0).  Neither array needs to be finalized. */
int bwtm_ra_subset_check(bwtm_ra* part, bwtm_ra* whole, uint64_t* part_bits, uint64_t* words_outside);
/* Finishes the rank array after all bwtm_search() calls / the exchange. */
int bwtm_ra_finalize(bwtm_ra* ra);
uint64_t bwtm_ra_values(const bwtm_ra* ra);   /* number of set bits after finalize (must equal bases of b) */
/* RA[i] for every position i of b (what the reference stores as (rank, count) runs). */
int bwtm_ra_download(bwtm_ra* ra, uint64_t* out, uint64_t capacity);
/* The raw bitvector words. */
int bwtm_ra_download_bits(bwtm_ra* ra, uint64_t* out_words, uint64_t capacity_words);
/* The rank array in the reference's own form: maximal (rank, count) runs in rank order, what RankArray
   iterates over (support.h:576-638, bwt.cpp:194-213).  *nruns receives the number of runs; up to
   `capacity` of them are written (call with capacity 0 to size the buffers). */
int bwtm_ra_download_runs(bwtm_ra* ra, uint64_t* ranks, uint64_t* counts, uint64_t capacity, uint64_t* nruns);

/* --- interleave: BWT::BWT(a, b, ra) (bwt.cpp:286-314) ------------------------------------ */

/* Interleaves a and b according to a finalized rank array.  The result is a device index
   (header, rank structure, C = C_a + C_b); call bwtm_index_encode() for the native bytes.
   a, b and ra stay valid (the facade frees them to mirror "destroying them"). */
int bwtm_interleave(const bwtm_index* a, const bwtm_index* b, bwtm_ra* ra, bwtm_index** out);

/* --- the whole path: FMI::FMI(a, b, parameters) (fmi.cpp:336-369) -------------------------- */

/* search over all sequences of b + finalize + interleave + encode + samples. */
int bwtm_merge(const bwtm_index* a, const bwtm_index* b, bwtm_index** out);
/* The same with the reference's ownership: "merges a and b, destroying them" (fmi.h:107-109).  Both
   handles are freed by the call (also when it fails); their device memory is released as soon as the
   stage that last needs it has run (native bytes after the transcode, records after the interleave:
   the counterpart of BlockArray::clearUntil in mergeBWT, bwt.cpp:224-225). */
int bwtm_merge_consume(bwtm_index* a, bwtm_index* b, bwtm_index** out);

/* Host-resident inputs -> host-resident result in one call: what merge() in bwt_merge.cpp:287-299 times.
   The two uploads, the device work and the download are pipelined on the context's copy and compute
   streams (H2D of chunk k + 1 under the decode of chunk k, transcode of b under the H2D of a, D2H of
   encoded ranges under the encoder).  Pass page-locked buffers (bwtm_host_alloc) for full PCIe speed. */
typedef struct
{
  const uint8_t* data; uint64_t nbytes;      /* native run-length bytes (BWT::data) */
  uint64_t sequences, bases;                 /* NativeHeader fields */
  const uint64_t* C;                         /* Alphabet::C or NULL */
} bwtm_host_input;
/* The library asks the caller for the output buffers once their sizes are known. */
enum { BWTM_BUF_DATA = 0, BWTM_BUF_BLOCK_END = 1, BWTM_BUF_CUM = 2, BWTM_BUF_FIELDS = 3, BWTM_BUF_ANCHORS = 4 };
/* want_samples: none, the full arrays (block_end + cum), or the compact form (fields + anchors; falls back to the full
   arrays, sample_width = 8, when a block encodes 2^32 - 1 positions or more). */
enum { BWTM_SAMPLES_NONE = 0, BWTM_SAMPLES_FULL = 1, BWTM_SAMPLES_COMPACT = 2,
       BWTM_RESULT_ON_DEVICE = -1 };           /* nothing is encoded or downloaded: the result is only handed back in *keep (an
                                                  intermediate result of a chained merge); the allocator is not called */
typedef void* (*bwtm_alloc_fn)(void* user, int what, uint64_t nbytes);
typedef struct
{
  uint8_t* data; uint64_t nbytes;            /* native bytes of the merged BWT */
  uint64_t blocks, sequences, bases;
  uint64_t C[BWTM_SIGMA + 1];
  uint64_t* block_end;                       /* [blocks]            (NULL unless samples were requested) */
  uint64_t* cum;                             /* [6][blocks + 1]     (NULL unless samples were requested) */
  int sample_width;                          /* 0 = no samples; 8 = block_end + cum above; 1 / 2 / 4 = fields + anchors below */
  void* fields;                              /* [6][blocks] of sample_width bytes (bwtm_index_download_samples_compact) */
  uint64_t* anchors;                         /* [6][ceil(blocks / 64)] */
  double ms_upload, ms_search, ms_interleave, ms_encode_download, ms_samples, ms_total;
} bwtm_host_output;
/* `keep` (optional) receives the merged device index (rank structure only) for a chained merge. */
int bwtm_merge_host(const bwtm_host_input* a, const bwtm_host_input* b, bwtm_alloc_fn alloc, void* user,
                    int want_samples, bwtm_host_output* out, bwtm_index** keep);
/* Chained form: `a` is a device index kept from the previous merge (consumed), `b` comes from the host. */
int bwtm_merge_host_chained(bwtm_index* a, const bwtm_host_input* b, bwtm_alloc_fn alloc, void* user,
                            int want_samples, bwtm_host_output* out, bwtm_index** keep);

/* Pipelined chain (bwt_merge in1 in2 in3 ...; bwt_merge.cpp:167-173): while THIS merge searches, the native bytes of the NEXT
   increment travel to the device.  Exactly one of (a_device, a_host) and one of (b_host, b_pending) is given; `next` (optional)
   announces the input of the following merge: its copies are queued on the copy stream behind this merge's own uploads and the
   pending upload comes back in *next_pending, to be passed as b_pending of the next call (or released with bwtm_upload_free).
   The caller's `next` buffer must stay valid until that call returns.  A chain then costs the first two uploads, the device
   work of every merge and one download instead of the sum of all transfers and all device work. */
typedef struct bwtm_upload bwtm_upload;
int bwtm_merge_host_pipelined(bwtm_index* a_device, const bwtm_host_input* a_host, const bwtm_host_input* b_host, bwtm_upload* b_pending,
                              const bwtm_host_input* next, bwtm_upload** next_pending, bwtm_alloc_fn alloc, void* user,
                              int want_samples, bwtm_host_output* out, bwtm_index** keep);
void bwtm_upload_free(bwtm_upload* upload);
/* The same announcement on its own: the copies of `in` are queued on the copy stream NOW (behind whatever was queued before)
   and the call returns; bwtm_upload_finish() waits for them, decodes, validates the header and returns the device index
   (like bwtm_index_upload; the pending upload is consumed, also on failure).  `in->data` must stay valid until then. */
int bwtm_upload_begin(const bwtm_host_input* in, bwtm_upload** out);
int bwtm_upload_finish(bwtm_upload* upload, bwtm_index** out);

/* --- the result sharded by output range (one slice per GPU) --------------------------------------------

   After the rank-array exchange every GPU holds the whole interleaving bitvector, so each can interleave and
   encode its own range of OUTPUT RECORDS (128 positions each) of mergeBWT (bwt.cpp:215-282).  Two facts cross a
   slice boundary and are exchanged as a few words (all-gather):
     * the run RunBuffer (utils.h:121-142) is still extending at the boundary: bwtm_slice_lasthead() of every slice
       -> heads_before of slice g = max over the slices before g;
     * array.size() % 64 in Run::write (support.h:256-282): bwtm_slice_size_table() = bytes the slice emits as a
       function of the byte offset it starts at, mod 64 -> bwtm_fold_offsets() over all slices gives every slice its
       exact byte offset in the merged stream.
   The concatenation of the slices' bytes (and samples) is bit-identical to bwtm_index_encode() of the whole. */

typedef struct bwtm_slice bwtm_slice;

uint64_t bwtm_merged_records(const bwtm_index* a, const bwtm_index* b);        /* output records of merging a and b */
/* Part `part` of `parts` near-equal ranges of whole 512-record encoder segments (getBounds, utils.cpp:169-187). */
int bwtm_slice_bounds(uint64_t nrecs, int parts, int part, uint64_t* rec_first, uint64_t* rec_last);
/* The same with EQUAL ranges (the last ones shorter or empty): range g = records [g * R, (g + 1) * R) clipped to nrecs, R a multiple of 512.
   *shard_bytes = R * 16 = the bytes of the interleaving bitvector one range covers: a buffer of parts * shard_bytes bytes (zero behind
   bwtm_ra_buffer_bytes()) can be handed to a reduce-scatter, which wants equal shares. */
int bwtm_slice_bounds_equal(uint64_t nrecs, int parts, int part, uint64_t* rec_first, uint64_t* rec_last, uint64_t* shard_bytes);
/* Output-range form of bwtm_ra_finalize(), for a rank array whose bitvector is complete only inside [rec_first, rec_last) -- what a
   REDUCE-SCATTER of the shards' bitvectors by output range leaves on a GPU (half the bytes of an all-reduce, and nobody counts bits it
   never reads).  Step 1, bwtm_ra_range_counts: *ones = set bits of the range; super_local[s] (nsup = (n_out >> 25) + 1 entries, zero for
   the others) = set bits between the start of the range and the start of super block s, for the supers that start inside the range;
   tail_words[128] = the bitvector words of the range's last chunk of 64 records (the next range's encoder needs the one record before
   its own).  These few KB are what the GPUs exchange.  Step 2, bwtm_ra_finalize_range: ones_before = set bits of all earlier ranges,
   ones_total = of all ranges, super_boff[s] = set bits before super s for ALL supers (= prefix of its owner + super_local[s]),
   halo_words = tail_words of the nearest earlier non-empty range (NULL for the first).  Afterwards bwtm_interleave_range() accepts exactly
   this range. */
int bwtm_ra_range_counts(bwtm_ra* ra, uint64_t rec_first, uint64_t rec_last, uint64_t* ones, uint64_t* super_local, uint64_t* tail_words);
int bwtm_ra_finalize_range(bwtm_ra* ra, uint64_t rec_first, uint64_t rec_last, uint64_t ones_before, uint64_t ones_total,
                           const uint64_t* super_boff, const uint64_t* halo_words);
/* mergeBWT for the output records [rec_first, rec_last) (bounds from bwtm_slice_bounds / bwtm_slice_bounds_equal). */
int bwtm_interleave_range(const bwtm_index* a, const bwtm_index* b, bwtm_ra* ra, uint64_t rec_first, uint64_t rec_last,
                          bwtm_slice** out);
void bwtm_slice_free(bwtm_slice* slice);
/* (position of the slice's last run head) + 1; 0 = the slice has none. */
int bwtm_slice_lasthead(bwtm_slice* slice, uint64_t* lasthead);
/* table[o] = bytes the slice emits when the stream is at offset o (mod 64) where the slice starts. */
int bwtm_slice_size_table(bwtm_slice* slice, uint64_t heads_before, uint64_t table[64]);
/* offsets[g] = byte offset of slice g, offsets[parts] = size of the stream; tables = [parts][64].  Pure host arithmetic. */
int bwtm_fold_offsets(const uint64_t* tables, int parts, uint64_t* offsets);
/* Run::write for the slice's runs, starting at its byte offset; block starts of BWT::build for its blocks. */
int bwtm_slice_encode(bwtm_slice* slice, uint64_t byte_offset);
uint64_t bwtm_slice_byte_first(const bwtm_slice* slice);
uint64_t bwtm_slice_bytes(const bwtm_slice* slice);
uint64_t bwtm_slice_block_first(const bwtm_slice* slice);      /* blocks whose first byte the slice emitted */
uint64_t bwtm_slice_blocks(const bwtm_slice* slice);
/* Sequence position at which the slice's first block starts (~0 if it has no block): the slice before it needs
   it for the end of its last block. */
int bwtm_slice_first_block_start(bwtm_slice* slice, uint64_t* position);
int bwtm_slice_download_data(bwtm_slice* slice, uint8_t* out, uint64_t capacity);
/* block_end[blocks] and cum[6][blocks] (row-major, this slice's blocks only); next_block_start = first block
   start of the next non-empty slice, or bases of the merged index for the last one. */
int bwtm_slice_download_samples(bwtm_slice* slice, uint64_t next_block_start, uint64_t* block_end, uint64_t* cum);
/* Plain symbols of positions inside the slice. */
int bwtm_slice_extract(bwtm_slice* slice, uint64_t first, uint64_t count, uint8_t* out);

/* --- the streamed merge: the slices above, one after the other on ONE GPU ------------------------------------------

   bwtm_merge_host() interleaves and encodes the whole result before it lets go of anything.  The streamed form uploads and searches in
   the same way, then runs the second half slice by slice (interleave_range, last head, size table, encode) and hands every slice's
   bytes and samples to the caller's SINK as soon as they are on the host: at most two slices are alive on the device, so the second
   half needs records + bitvector + 2 slices instead of records + the whole stream (mergeBWT frees what it has consumed,
   BlockArray::clearUntil, bwt.cpp:224-225).

   A PIECE carries the bytes [byte_first, byte_first + nbytes) of BWT::data and the samples of the blocks whose END is known with it:
   a block's length is known with the next block start, so piece g delivers the last block of the nearest earlier piece that had one and
   all its own blocks but the last; the final piece (last != 0, always delivered, possibly empty) closes the last block.  A slice that
   lies inside one run yields no piece.  The pointers are library-owned page-locked staging, valid until the sink returns.
   sample_width: 0 = no samples were asked for; 1 / 2 / 4 = fields[6][sample_blocks] of that many bytes and anchors[6][nanchors], the
   anchors of the global groups anchor_first .. anchor_first + nanchors - 1 (group k = blocks 64 k ..; those with 64 k inside the sample
   range), the narrowest width that holds the piece's longest block (bwtm_index_samples_width's rule, per piece); 8 = block_end
   [sample_blocks] and cum[6][sample_blocks] (always with BWTM_SAMPLES_FULL; in compact mode only when a block reaches 2^32 - 1
   positions).  Laid end to end and widened to the largest width, the pieces' arrays are what bwtm_index_download_samples_compact /
   bwtm_index_download_samples give for the whole result (the latter's column behind the last block is C: cum[c][blocks] = C[c + 1] - C[c]).
   A sink that returns non-zero stops the merge: the call returns BWTM_EINVAL. */
typedef struct
{
  uint64_t byte_first, nbytes; const uint8_t* data;
  uint64_t sample_block_first, sample_blocks;
  int sample_width;
  const void* fields; const uint64_t* anchors;
  uint64_t anchor_first, nanchors;
  const uint64_t* block_end; const uint64_t* cum;
  int last;
} bwtm_piece;
typedef int (*bwtm_piece_fn)(void* user, const bwtm_piece* piece);
typedef struct
{
  uint64_t pieces;                           /* sink calls */
  uint64_t slice_records;                    /* records per slice the call ran with */
  uint64_t slice_bytes_peak;                 /* largest sum of the device buffers of the live slices and the call's device staging */
  double ms_upload, ms_search, ms_second_half, ms_total;
} bwtm_stream_stats;
/* Exactly one of a_device (a kept device index, consumed also on failure) and a_host.  slice_records: a multiple of 512, or 0 = the library
   chooses (two slices within a fixed share of the free device memory); at least the result's records = one slice.  want_samples:
   BWTM_SAMPLES_NONE / _FULL / _COMPACT.  `out` receives the header fields, C, nbytes, blocks and the timings; its pointers stay NULL.
   `stats` may be NULL.  The sink is called on the calling thread, between the library's own calls: it must not call the library on the
   same context.
   bwtm_tune("stream_upload", 1): b and then a_host go through the chunked upload (bwtm_index_upload_streamed), so that neither input's
   native stream is ever resident as a whole; ms_upload covers it, slice_bytes_peak counts its ring as well.  The pieces are the same. */
int bwtm_merge_host_streamed(bwtm_index* a_device, const bwtm_host_input* a_host, const bwtm_host_input* b_host,
                             uint64_t slice_records, int want_samples, bwtm_piece_fn sink, void* user,
                             bwtm_host_output* out, bwtm_stream_stats* stats);

/* --- the merge over PARTITIONED records: one part per GPU, nothing replicated ---------------------------------
   (the thread fan-out of fmi.cpp:351-358 and utils.cpp:189-218 as ranges of the merged ORDER instead of blocks of
   b's sequences.)  A cut is a pair (cut_a[g], cut_b[g]) = (suffixes of a below w_g, suffixes of b below w_g) for a k-mer w_g; part g owns
   a's records of [cut_a[g], cut_a[g + 1]], b's of [cut_b[g], cut_b[g + 1]) -- transcoded on its GPU from its own share of the native bytes --,
   the frontier elements and trie nodes whose b coordinate lies in that range, and the bits and records of the output range
   [cut_a[g] + cut_b[g], cut_a[g + 1] + cut_b[g + 1]) rounded to encoder segments.  Every rank query is local; the frontier's elements cross
   between GPUs as loads of peer-mapped memory inside the step kernel, everything else is a few hundred bytes per LF step.

   The parts of a merge (threads of one process, or one process per GPU) meet in a GROUP: a block of POSIX shared memory named by the caller
   (a name that begins with '/', unique per group: e.g. "/bwtm-<launcher pid>-<port>"); part 0 creates it, the others attach, and the name
   is unlinked as soon as all have.  A group serves any number of merges, one after the other.  Every part:

       bwtm_group_create(name, g, parts, &group);                                   once
       bwtm_partition_cuts_host(&a, &b, parts, 0, cut_a, cut_b);                     every part computes the same cuts (or receives them)
       bwtm_part_create(group, &a_header, &b_header, cut_a, cut_b, &part);           binds the calling thread's context
       for which in {0, 1}:  bwtm_part_window(part, which, &p0, &p1);  bwtm_window_blocks(&x, p0, p1, &b0, &b1, &first, before);
                             bwtm_part_upload(part, which, x.data + 64 b0, bytes of the blocks, first, before, 0);
       bwtm_part_search(part);                                                       collective
       bwtm_part_finish(part, &slice, &byte_offset, &total_bytes, &next_start);      collective; then bwtm_slice_download_*(slice, ...)
       bwtm_part_free(part);

   The concatenation of the parts' slices is bit-identical to bwtm_merge() of the whole inputs.  When a part fails, the others return
   BWTM_EPEER from their next collective step instead of waiting for it (and every wait has a deadline: BWTM_GROUP_TIMEOUT seconds, 300).
   A part that runs out of room -- the cuts balance positions, which does not bound the elements of a skewed collection -- returns BWTM_ENOMEM and
   the others BWTM_EPEER, all from the same step: the caller repeats the merge another way (csrc/host/multi_gpu.h: sequence blocks).  A group
   that has seen a failure stays failed: free it and create another. */

#define BWTM_MAX_PARTS 16
typedef struct bwtm_group bwtm_group;
typedef struct bwtm_part bwtm_part;

int bwtm_group_create(const char* name, int part, int parts, bwtm_group** out);     /* collective; name may be NULL when parts == 1 */
void bwtm_group_free(bwtm_group* group);
int bwtm_group_part(const bwtm_group* group);
int bwtm_group_parts(const bwtm_group* group);
int bwtm_group_barrier(bwtm_group* group);
/* all[h * nbytes ..] = part h's `mine` (host memory, any size; collective). */
int bwtm_group_allgather(bwtm_group* group, const void* mine, uint64_t nbytes, void* all);
void bwtm_group_abort(bwtm_group* group);                                           /* the caller gives up: wakes the others with BWTM_EPEER */

/* A host-resident input as the reference's loaded FMI holds it: the native bytes and the samples of BWT::build (bwt.cpp:476-512) as plain
   arrays, cum[c][k] (row-major, blocks + 1 columns) = occurrences of symbol c before block k. */
typedef struct
{
  const uint8_t* data; uint64_t nbytes, blocks;
  uint64_t sequences, bases;
  uint64_t C[BWTM_SIGMA + 1];
  const uint64_t* cum;                       /* [6][blocks + 1] */
} bwtm_host_index;
typedef struct { uint64_t bases, sequences; uint64_t C[BWTM_SIGMA + 1]; } bwtm_index_header;

/* parts - 1 cuts at k-mer boundaries (kmer = 0: 4 for up to 8 parts, else 5) that balance the parts' shares of a's + b's positions:
   insertion points by backward search on the host, sp(c w) = C[c] + rank_c(sp(w)) (utils.h:335-355, BWT::rank bwt.cpp:318-341).  cut_a,
   cut_b: parts + 1 entries each (cut[0] = 0, cut[parts] = bases).  Pure host arithmetic; every part gets the same answer. */
int bwtm_partition_cuts_host(const bwtm_host_index* a, const bwtm_host_index* b, int parts, int kmer, uint64_t* cut_a, uint64_t* cut_b);
/* The 64-byte blocks [*block_first, *block_end) of x's stream whose records cover the positions [pos_first, pos_last], the position the first
   of them begins at and the symbol counts before it (what bwtm_index_upload_window / bwtm_part_upload want); an index of 0 positions has no
   blocks: [0, 0).  Pure host arithmetic. */
int bwtm_window_blocks(const bwtm_host_index* x, uint64_t pos_first, uint64_t pos_last, uint64_t* block_first, uint64_t* block_end,
                       uint64_t* first_position, uint64_t counts_before[6]);

/* A WINDOW of an index, transcoded from its own share of the native bytes: `data` = whole 64-byte blocks of the stream (host memory; device
   memory read in place when on_device != 0: 16-byte aligned, readable 16 bytes past the end), first_position = the position the first
   block begins at, counts_before[c] = occurrences of c before it, bases / sequences / C = the header of the WHOLE index.  The handle serves
   the records that lie wholly inside the bytes, addressed by their absolute numbers; only bwtm_ra_create_range, bwtm_interleave_range (with a
   rank array finalized for a range the windows cover) and the bwtm_part_* calls take it.  An index of 0 positions is uploaded from 0 bytes. */
int bwtm_index_upload_window(const uint8_t* data, uint64_t nbytes, uint64_t first_position, const uint64_t counts_before[6],
                             uint64_t bases, uint64_t sequences, const uint64_t C[BWTM_SIGMA + 1], int on_device, bwtm_index** out);
uint64_t bwtm_index_record_bytes(const bwtm_index* index);        /* bytes of records the handle holds (a window: its share) */
/* The rank array of one part: the bits of the output positions [pos_first, pos_last) plus one 65 536-position tile on either side. */
int bwtm_ra_create_range(const bwtm_index* a, const bwtm_index* b, uint64_t pos_first, uint64_t pos_last, bwtm_ra** out);
uint64_t bwtm_ra_bytes(const bwtm_ra* ra);                         /* bytes of bitvector the handle holds */

typedef struct
{
  uint64_t steps, node_levels;               /* LF steps on elements / levels on trie nodes */
  uint64_t elements, largest;                /* elements this part advanced in all steps / in its largest step */
  uint64_t pulled_bytes;                     /* bytes of elements and table entries its step kernels read from the parts' output buffers */
  uint64_t boundary_bytes;                   /* bytes of boundary bits per pair of neighbouring parts */
  uint64_t record_bytes, bitvector_bytes;    /* what the part holds */
  double ms_search, ms_search_wait, ms_finish;   /* wall time of the two collective calls; of the search, the time spent waiting for peers */
} bwtm_part_info;

int bwtm_part_create(bwtm_group* group, const bwtm_index_header* a, const bwtm_index_header* b,
                     const uint64_t* cut_a, const uint64_t* cut_b, bwtm_part** out);
void bwtm_part_free(bwtm_part* part);
/* The positions [*pos_first, *pos_last] of input `which` (0 = a, 1 = b) this part's window must cover: its range and two encoder segments on either side. */
int bwtm_part_window(const bwtm_part* part, int which, uint64_t* pos_first, uint64_t* pos_last);
int bwtm_part_upload(bwtm_part* part, int which, const uint8_t* data, uint64_t nbytes, uint64_t first_position,
                     const uint64_t counts_before[6], int on_device);
/* buildRA (fmi.cpp:272-334) for the part's range: node levels and LF steps in lock step with the other parts. */
int bwtm_part_search(bwtm_part* part);
/* The second half: boundary bits, range counts, bwtm_ra_finalize_range, bwtm_interleave_range, the encoder's carries, bwtm_slice_encode.
   *slice = the part's encoded slice (the caller frees it), *byte_offset = where its bytes begin in the merged stream, *total_bytes = the
   stream's size, *next_block_start = what bwtm_slice_download_samples wants.  The part's windows and rank array are released. */
int bwtm_part_finish(bwtm_part* part, bwtm_slice** slice, uint64_t* byte_offset, uint64_t* total_bytes, uint64_t* next_block_start);
int bwtm_part_stats(const bwtm_part* part, bwtm_part_info* info);

/* --- ingest: reads -> index ---------------------------------------------------
   The reference merges BWTs that other tools built (RopeBWT / SGA, README.md:5,20; PlainData::read, formats.cpp:133-161,
   is the text form of such a collection).  The builder stands in for them on the GPU: reads arrive in batches, in
   collection order; every `leaf_reads` reads become a leaf BWT by suffix sort (equal suffixes in read order, the order
   bwt_merge produces), and leaves are combined by the merger itself (bwtm_search + bwtm_interleave on device records),
   level by level like a binary counter.  The result is what merging the per-read BWTs in order would give. */

typedef struct bwtm_builder bwtm_builder;

/* leaf_reads = 0: default (2^19); a leaf is also capped so that leaf_reads * (width + 1) < 2^32. */
int bwtm_builder_create(uint64_t leaf_reads, bwtm_builder** out);
/* `nreads` rows of `stride` bytes, comp values 1..5 (Alphabet, support.h:167-169); row k holds lengths[k] <= width
   symbols (lengths == NULL: every row holds `width`).  Pointers are device pointers when on_device != 0, host pointers
   otherwise.  Returns when the batch has been consumed. */
int bwtm_builder_add(bwtm_builder* builder, const uint8_t* reads, uint64_t nreads, uint32_t width, uint64_t stride,
                     const uint32_t* lengths, int on_device);
uint64_t bwtm_builder_reads(const bwtm_builder* builder);
/* Merges what is left and hands the index over (records only, like bwtm_interleave's result); frees the builder. */
int bwtm_builder_finish(bwtm_builder* builder, bwtm_index** out);
void bwtm_builder_free(bwtm_builder* builder);

/* --- the memory pool of the calling thread's context -------------------------------------------
   Large blocks live in a reserved virtual address range that is consumed and never reused; when no range
   is left they come from hipMalloc, which is correct but slow when it has to wait for deferred frees: `hipmalloc_fallbacks`
   counts those blocks, so that a long-lived process can see that it has reached that state. */
typedef struct
{
  uint64_t held_bytes, cached_bytes, peak_bytes;      /* physical memory held / idle in the pool / high-water mark */
  uint64_t mapped_blocks;                             /* blocks that live in the reserved address range (in use or idle) */
  uint64_t address_bytes_reserved;                    /* process-wide */
  int address_space_exhausted;                        /* 1: no further range can be reserved */
  uint64_t hipmalloc_fallbacks;                       /* large blocks served by hipMalloc since then */
} bwtm_pool_info;
int bwtm_pool_stats(bwtm_pool_info* info);
/* A test hook.  BWTM_POOL_POISON=<32-bit value, decimal or 0x...> in the environment (read once per process): every block of device memory
   the library hands itself is filled with that word before it is used, so that bytes no kernel wrote are never zeros or leftovers by luck.
   Reports the fills made so far and the bytes they covered, process-wide (NULL: not wanted); both stay 0 when the mode is off. */
int bwtm_pool_poison_stats(uint64_t* fills, uint64_t* bytes);

/* --- measurement ----------------------------------------------------------------------------- */

/* When enabled, every kernel launch is bracketed by HIP events on the context's compute stream. */
int bwtm_profile_enable(int on);
/* Restricts the bracketing to launches of the named kernels (a comma-separated list of the names bwtm_profile_read reports,
   e.g. "frontier_step,lf_walk"); NULL or "" = all kernels.  Two event records per launch cost a few microseconds each on the stream: a timed region that only needs the
   dominant kernel's durations brackets only that kernel. */
int bwtm_profile_only(const char* name);
int bwtm_profile_reset(void);
/* Launches of the frontier search's step kernel since the last bwtm_profile_reset (counted whether or not profiling is enabled), by the
   form of the frontier's coordinates: [0] absolute in and out, [1] absolute in and class-relative out (the first step of a search that
   takes the class-relative form), [2] class-relative in and out (bwtm_tune "frontier_rel"). */
int bwtm_frontier_step_forms(uint64_t launches[3]);
/* Launches of the kernel that builds an index's records from its native stream since the last bwtm_profile_reset (counted whether or
   not profiling is enabled), by instantiation: index 8 * chunk + 2 * w + uniform.  chunk: 0 the one-shot upload, 1 the chunked upload;
   w: the LDS window, 0 = 8192 positions, 1 = 16384, 2 = 32768, 3 = 32768 with the cooperative fill of long runs; uniform: 1 = the
   straight-line deposit (bwtm_tune "recs_window", "recs_uniform"; otherwise by the stream's average density). */
int bwtm_transcode_forms(uint64_t launches[16]);
/* Per-kernel totals since the last reset: returns the number of distinct kernels; fills up to
   `capacity` entries.  names[k] points to a static string. */
int bwtm_profile_read(const char** names, double* total_ms, uint64_t* launches, int capacity);

#ifdef __cplusplus
}
#endif

#endif /* BWTM_H */
