/*
  bwtm_api.hip -- implementation of the C ABI declared in include/bwtm.h: host-side
  orchestration of the gfx950 kernels in bwtm_kernels.hip.h.  No CPU fallback exists: every
  entry point fails with BWTM_ENODEV when no HIP device is usable.

    api/context.hip.h   contexts (device, streams, memory pool), errors, launch macros, profiling, scans
    api/index.hip.h     device index: upload steps, the blocking upload of one index, the pipelined upload of a merge's two inputs,
                        transcode, canonical encoder (EncodePasses: its one driver, for the whole index and for a slice) + pipelined
                        download, queries
    api/upload_stream.hip.h  the chunked upload: records + super table from a ring of chunk buffers, the stream never resident as a whole
    api/search.hip.h    rank array: frontier search / per-chain walk, finalize, downloads
    api/merge.hip.h     interleave, the merged header, whole-path entry points (device-resident, consuming, host-to-host)
    api/slices.hip.h    output-range-sharded interleave + encode (one slice per GPU): the encoder's passes with the two carries between slices
    api/stream.hip.h    host-to-host merge whose second half runs slice by slice on one GPU, the result handed to the caller in pieces
    api/group.hip.h     the parts of a multi-GPU merge: shared control block (barrier, small all-gathers), exported arenas (raw pointer / HIP IPC)
    api/pmerge.hip.h    the merge over PARTITIONED records, one part per GPU: windows from byte shares, cuts, the routed search, the second half
    api/sequences.hip.h sequences by id: lengths, offsets and text in batches of bounded device memory
    api/batches.hip.h   the batch scheme of the calls that take texts from the host, stated once for the files marked (b): the texts' validation, a
                        staged batch, the two rounds of a call that sizes before it fills, optional arrays to the host, a call's statistics
    api/locate.hip.h    positions to (sequence id, offset): the locator's table, positions and ranges located in batches
    api/overlap.hip.h   suffix-prefix overlaps: one backward search per query, counted, then emitted and expanded through the locator's table (b)
    api/frontier.hip.h  the host side of the level scheme the next four share: the doubling frontier of parallel arrays, a level's totals with their
                        scan and read-back
    api/kmers.hip.h     the distinct k-mers of an index with counts and ranges: the trie's levels on two ping-pong frontiers, the spectrum
    api/kmer_join.hip.h the k-mers of two indexes with their counts and insertion points in each: one joint walk, the summary of the result
    api/approx.hip.h    patterns with up to d substitutions: a batch's backward search as one frontier of ranges, the hits gathered per pattern (b); a batch of
                        patterns with its hit stream and offsets, which the next shares
    api/edit.hip.h      patterns within edit distance e: the same frontier with a band of the edit-distance matrix per node, the hits gathered per pattern and length (b)
    api/correct.hip.h   k-mer error correction of reads: the solid k-mers of a spectrum as a sorted table with a bucket directory, a wave per read,
                        on patterns from the host or on sequences extracted on the device, in batches of bounded device memory (b)
    api/unitigs.hip.h   the unitigs of the k-mer graph over the solid k-mers of a spectrum: the corrector's table with the counts beside it, the
                        phases of kernels/unitigs.hip.h, the result downloaded in slices, k-mers placed in it
    api/mem.hip.h       matching statistics and maximal exact matches of patterns: one backward search per symbol of a batch's text; for the MEMs a quad
                        per pattern that flags the ends that give one, two scans and one emit, in batches of bounded device memory (b)
    api/fslice.hip.h    one GPU's state of the sliced frontier search (only with -DBWTM_EXPERIMENTAL; include/bwtm_experimental.h)
    api/partition.hip.h the first, host-driven form of the partitioned search (same build only; kept for its tests and A/B measurements)
*/
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bwtm.h"
#include "bwtm_kernels.hip.h"

using namespace bwtm;

#include "api/context.hip.h"
#include "api/index.hip.h"
#include "api/search.hip.h"
#include "api/merge.hip.h"
#include "api/upload_stream.hip.h"
#include "api/slices.hip.h"
#include "api/stream.hip.h"
#include "api/group.hip.h"
#include "api/pmerge.hip.h"
#ifdef BWTM_EXPERIMENTAL
#include "../../include/bwtm_experimental.h"
#include "api/fslice.hip.h"
#include "api/partition.hip.h"
#endif
#include "api/ingest.hip.h"
#include "api/sequences.hip.h"
#include "api/batches.hip.h"
#include "api/locate.hip.h"
#include "api/overlap.hip.h"
#include "api/frontier.hip.h"
#include "api/kmers.hip.h"
#include "api/kmer_join.hip.h"
#include "api/approx.hip.h"
#include "api/edit.hip.h"
#include "api/correct.hip.h"
#include "api/unitigs.hip.h"
#include "api/mem.hip.h"
