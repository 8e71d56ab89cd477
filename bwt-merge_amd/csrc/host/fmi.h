/*
  fmi.h -- host facade: FMI, MergeParameters and the format-dispatching load / serialize
  (reference fmi.h:38-230, fmi.cpp:336-495).  The merging constructor runs the whole hot path
  on the GPU through the C ABI; everything else is small host code.
*/
#ifndef BWTM_HOST_FMI_H
#define BWTM_HOST_FMI_H

#include <thread>
#include "bwt.h"

namespace bwtmerge
{

class FMI;
void serialize(const FMI& fmi, const std::string& filename, const std::string& format);
void load(FMI& fmi, const std::string& filename, const std::string& format);

/*
  The reference's knobs.  Buffer sizes, merge buffers and the temp directory have nothing to
  configure on the device (no buffer hierarchy, no temp files); they are accepted, printed and
  otherwise ignored.  sequence_blocks is honoured by the two-step API (buildRA: one bwtm_search()
  call per block); the merging constructor searches all sequences in one call, which is what the
  device wants (it partitions the work itself).
  lazy_host (an addition): the merged FMI is left on the device and its host form is produced when
  something asks for it; the tool sets it for every merge but the last of a chain.
  streamed (an addition): the host-to-host merge runs its second half slice by slice (bwtm_merge_host_streamed, slice_records records
  per slice, 0 = the library chooses) and the pieces are assembled into the result's arrays here: the device never holds the whole
  encoded stream, and no device index is kept with the result.
  stream_upload (with streamed): the host inputs of that merge go through the chunked upload (bwtm_tune "stream_upload"): neither
  input's native stream is ever resident on the device as a whole.
*/
struct MergeParameters
{
  typedef range_type run_type;

  const static size_type RUN_BUFFER_SIZE = 8 * MEGABYTE;
  const static size_type THREAD_BUFFER_SIZE = 256 * MEGABYTE;
  const static size_type MERGE_BUFFERS = 6;
  const static size_type BLOCKS_PER_THREAD = 4;

  MergeParameters() :
    run_buffer_size(RUN_BUFFER_SIZE), thread_buffer_size(THREAD_BUFFER_SIZE), merge_buffers(MERGE_BUFFERS),
    threads(Parallel::max_threads), sequence_blocks(threads * BLOCKS_PER_THREAD), temp_dir("."), lazy_host(false), streamed(false), slice_records(0), stream_upload(false) {}

  void sanitize()
  {
    threads = Range::bound(threads, 1, Parallel::max_threads);
    sequence_blocks = std::max(sequence_blocks, (size_type)1);
    threads = std::min(threads, sequence_blocks);
  }

  static double defaultRB() { return inMegabytes(RUN_BUFFER_SIZE * sizeof(run_type)); }
  static double defaultTB() { return inMegabytes(THREAD_BUFFER_SIZE); }
  static size_type defaultMB() { return MERGE_BUFFERS; }
  static size_type defaultT()  { return Parallel::max_threads; }
  static size_type defaultSB() { return BLOCKS_PER_THREAD; }

  void setRB(size_type mb) { run_buffer_size = mb * MEGABYTE / sizeof(run_type); }
  void setTB(size_type mb) { thread_buffer_size = mb * MEGABYTE; }
  void setMB(size_type n)  { merge_buffers = n; }
  void setT(size_type n)   { threads = n; }
  void setSB(size_type n)  { sequence_blocks = n; }
  void setTemp(const std::string& directory)
  {
    if(directory.empty()) { temp_dir = "."; }
    else { temp_dir = (directory.back() == '/' ? directory.substr(0, directory.length() - 1) : directory); }
  }

  size_type run_buffer_size, thread_buffer_size;
  size_type merge_buffers;
  size_type threads, sequence_blocks;
  std::string temp_dir;
  bool lazy_host;
  bool streamed; size_type slice_records;
  bool stream_upload;
};

inline std::ostream& operator<<(std::ostream& out, const MergeParameters& p)
{
  out << "Run buffers:      " << inMegabytes(p.run_buffer_size * sizeof(MergeParameters::run_type)) << " MB" << std::endl;
  out << "Thread buffers:   " << inMegabytes(p.thread_buffer_size) << " MB" << std::endl;
  out << "Merge buffers:    " << p.merge_buffers << std::endl;
  out << "Threads:          " << p.threads << std::endl;
  out << "Sequence blocks:  " << p.sequence_blocks << std::endl;
  out << "Temp directory:   " << p.temp_dir << std::endl;
  return out;
}

class FMI
{
public:
  typedef BWT::size_type size_type;
  const static size_type SHORT_RANGE = 256;

  FMI() {}

  // Merges a and b, destroying them (reference fmi.h:107-110).
  FMI(FMI& a, FMI& b, MergeParameters parameters = MergeParameters());

  void swap(FMI& other) { bwt.swap(other.bwt); std::swap(alpha, other.alpha); }

  size_type size() const { return bwt.size(); }
  size_type sequences() const { return bwt.sequences(); }
  range_type charRange(comp_type comp) const { return range_type(alpha.C[comp], alpha.C[comp + 1] - 1); }

  // (LF(i), BWT[i])
  range_type LF(size_type i) const
  {
    range_type t = bwt.inverse_select(i);
    return range_type(t.first + alpha.C[t.second], t.second);
  }
  size_type LF(size_type i, comp_type comp) const { return alpha.C[comp] + bwt.rank(i, comp); }
  range_type LF(range_type range, comp_type comp) const { return range_type(LF(range.first, comp), LF(range.second + 1, comp) - 1); }
  void LF(size_type i, BWT::ranks_type& results) const
  {
    bwt.ranks(i, results);
    for(size_type c = 1; c < alpha.sigma; c++) { results[c] += alpha.C[c]; }
  }
  void LF(range_type range, BWT::ranks_type& sp, BWT::ranks_type& ep) const
  {
    bwt.ranks(range.first, sp); bwt.ranks(range.second + 1, ep);
    for(size_type c = 1; c < alpha.sigma; c++) { sp[c] += alpha.C[c]; ep[c] += alpha.C[c] - 1; }
  }
  void LF(range_type range, BWT::rank_ranges_type& results) const
  {
    bwt.ranks(range, results);
    for(size_type c = 1; c < alpha.sigma; c++) { results[c].first += alpha.C[c]; results[c].second += alpha.C[c] - 1; }
  }

  // Backward search; the pattern is given in characters.
  template<class Iterator>
  range_type find(Iterator begin, Iterator end) const
  {
    if(begin == end) { return range_type(0, size() - 1); }
    --end;
    range_type range = charRange(alpha.char2comp[(byte_type)*end]);
    while(!Range::empty(range) && end != begin)
    {
      --end;
      range = LF(range, alpha.char2comp[(byte_type)*end]);
    }
    return range;
  }
  template<class Container> range_type find(const Container& pattern) const { return find(pattern.begin(), pattern.end()); }

  // One string within max_mismatches substitutions of a pattern that occurs in the collection: its range, as find() returns it, and the
  // number of places in which it differs.
  struct ApproxHit
  {
    range_type range; size_type mismatches;
  };

  // Backward search with up to max_mismatches (0..8) substitutions of patterns given as comp values 1..5: pattern k is
  // text[offsets[k] .. offsets[k + 1]), its hits are hits[hit_offsets[k] .. hit_offsets[k + 1]), ascending when the matched strings are
  // compared from their last symbol backwards; max_hits > 0 keeps the first max_hits of every pattern.  On the device
  // (bwtm_find_approx_batch: a sizing call, then the filling one).  The index goes to the device if it is not there, and stays.
  void findApprox(const std::vector<byte_type>& text, const std::vector<uint64_t>& offsets, size_type max_mismatches, std::vector<size_type>& hit_offsets,
    std::vector<ApproxHit>& hits, size_type max_hits = 0) const
  {
    const size_type count = (offsets.empty() ? 0 : offsets.size() - 1);
    hit_offsets.assign(count + 1, 0); hits.clear();
    if(count == 0) { return; }
    bwtm_index* ix = bwt.onDevice(alpha.C);
    const uint32_t d = (uint32_t)std::min<size_type>(max_mismatches, ~(uint32_t)0);
    gpuCheck(bwtm_find_approx_batch(ix, text.data(), offsets.data(), count, d, max_hits, hit_offsets.data(), nullptr, nullptr, nullptr, 0), "FMI::findApprox()");
    const size_type total = hit_offsets[count];
    if(total == 0) { return; }
    std::vector<uint64_t> sp(total), len(total); std::vector<uint8_t> mm(total);
    gpuCheck(bwtm_find_approx_batch(ix, text.data(), offsets.data(), count, d, max_hits, hit_offsets.data(), sp.data(), len.data(), mm.data(), total), "FMI::findApprox()");
    hits.resize(total);
    for(size_type h = 0; h < total; h++) { hits[h].range = range_type(sp[h], sp[h] + len[h] - 1); hits[h].mismatches = mm[h]; }
  }

  // One string within max_edits insertions, deletions and substitutions of a pattern that occurs in the collection: its range, as find()
  // returns it, its Levenshtein distance from the pattern, and its length.
  struct EditHit
  {
    range_type range; size_type edits; size_type length;
  };

  // Backward search within edit distance max_edits (0..7) of patterns given as comp values 1..5: pattern k is
  // text[offsets[k] .. offsets[k + 1]), its hits are hits[hit_offsets[k] .. hit_offsets[k + 1]), shortest first and, within a length,
  // ascending when the matched strings are compared from their last symbol backwards; max_hits > 0 keeps the first max_hits of every
  // pattern.  On the device (bwtm_find_edit_batch: a sizing call, then the filling one).  The index goes to the device if it is not
  // there, and stays.
  void findEdit(const std::vector<byte_type>& text, const std::vector<uint64_t>& offsets, size_type max_edits, std::vector<size_type>& hit_offsets,
    std::vector<EditHit>& hits, size_type max_hits = 0) const
  {
    const size_type count = (offsets.empty() ? 0 : offsets.size() - 1);
    hit_offsets.assign(count + 1, 0); hits.clear();
    if(count == 0) { return; }
    bwtm_index* ix = bwt.onDevice(alpha.C);
    const uint32_t e = (uint32_t)std::min<size_type>(max_edits, ~(uint32_t)0);
    gpuCheck(bwtm_find_edit_batch(ix, text.data(), offsets.data(), count, e, max_hits, hit_offsets.data(), nullptr, nullptr, nullptr, nullptr, 0), "FMI::findEdit()");
    const size_type total = hit_offsets[count];
    if(total == 0) { return; }
    std::vector<uint64_t> sp(total), len(total); std::vector<uint8_t> ed(total); std::vector<uint32_t> lengths(total);
    gpuCheck(bwtm_find_edit_batch(ix, text.data(), offsets.data(), count, e, max_hits, hit_offsets.data(), sp.data(), len.data(), ed.data(), lengths.data(), total), "FMI::findEdit()");
    hits.resize(total);
    for(size_type h = 0; h < total; h++) { hits[h].range = range_type(sp[h], sp[h] + len[h] - 1); hits[h].edits = ed[h]; hits[h].length = lengths[h]; }
  }

  // The longest match that ends with one symbol of a pattern: its length (0: the symbol alone does not occur) and its range, as find()
  // returns it (empty when the length is 0).
  struct MatchStat
  {
    size_type length; range_type range;
  };

  // Matching statistics of patterns given as comp values 1..5: pattern k is text[offsets[k] .. offsets[k + 1]), and stats holds one
  // entry per symbol of the text, at offsets[k] + i - offsets[0] for symbol i of pattern k.  On the device (bwtm_matching_stats_batch).
  // The index goes to the device if it is not there, and stays.
  void matchingStats(const std::vector<byte_type>& text, const std::vector<uint64_t>& offsets, std::vector<MatchStat>& stats) const
  {
    const size_type count = (offsets.empty() ? 0 : offsets.size() - 1);
    stats.clear();
    const size_type total = (count == 0 ? 0 : offsets[count] - offsets[0]);
    if(total == 0) { return; }
    bwtm_index* ix = bwt.onDevice(alpha.C);
    std::vector<uint32_t> lengths(total); std::vector<uint64_t> sp(total), len(total);
    gpuCheck(bwtm_matching_stats_batch(ix, text.data(), offsets.data(), count, lengths.data(), sp.data(), len.data()), "FMI::matchingStats()");
    stats.resize(total);
    for(size_type h = 0; h < total; h++)
    {
      stats[h].length = lengths[h];
      stats[h].range = (lengths[h] > 0 ? range_type(sp[h], sp[h] + len[h] - 1) : range_type(1, 0));
    }
  }

  // A maximal exact match of a pattern: pattern[begin .. begin + length) occurs, and no longer substring of the pattern that contains
  // it does; its range, as find() returns it.
  struct MEM
  {
    size_type begin, length; range_type range;
  };

  // The maximal exact matches of at least min_length (>= 1) symbols of patterns given as comp values 1..5: pattern k is
  // text[offsets[k] .. offsets[k + 1]), its MEMs are mems[hit_offsets[k] .. hit_offsets[k + 1]), begins and ends ascending.  On the
  // device (bwtm_mem_batch: a sizing call, then the filling one).  The index goes to the device if it is not there, and stays.
  void mems(const std::vector<byte_type>& text, const std::vector<uint64_t>& offsets, size_type min_length, std::vector<size_type>& hit_offsets,
    std::vector<MEM>& mems) const
  {
    const size_type count = (offsets.empty() ? 0 : offsets.size() - 1);
    hit_offsets.assign(count + 1, 0); mems.clear();
    if(count == 0) { return; }
    bwtm_index* ix = bwt.onDevice(alpha.C);
    const uint32_t least = (uint32_t)std::min<size_type>(min_length, ~(uint32_t)0);
    gpuCheck(bwtm_mem_batch(ix, text.data(), offsets.data(), count, least, hit_offsets.data(), nullptr, nullptr, nullptr, nullptr, 0), "FMI::mems()");
    const size_type total = hit_offsets[count];
    if(total == 0) { return; }
    std::vector<uint32_t> begin(total), length(total); std::vector<uint64_t> sp(total), len(total);
    gpuCheck(bwtm_mem_batch(ix, text.data(), offsets.data(), count, least, hit_offsets.data(), begin.data(), length.data(), sp.data(), len.data(), total), "FMI::mems()");
    mems.resize(total);
    for(size_type h = 0; h < total; h++) { mems[h].begin = begin[h]; mems[h].length = length[h]; mems[h].range = range_type(sp[h], sp[h] + len[h] - 1); }
  }

  // The sequences with the ids [ids.first, ids.second] as comp values 1..5 in forward order, endmarkers not included: sequence k of the
  // range is text[offsets[k] .. offsets[k + 1]).  LF walks on the device (bwtm_sequences_extract: a sizing call, then the extracting one);
  // no sequence may be longer than max_len (0: 65536).  The index goes to the device if it is not there, and stays.
  void sequences(range_type ids, std::vector<size_type>& offsets, std::vector<byte_type>& text, size_type max_len = 0) const
  {
    const size_type count = (Range::empty(ids) ? 0 : Range::length(ids));
    offsets.assign(count + 1, 0); text.clear();
    if(count == 0) { return; }
    bwtm_index* ix = bwt.onDevice(alpha.C);
    gpuCheck(bwtm_sequences_extract(ix, nullptr, ids.first, count, max_len, offsets.data(), nullptr, 0), "FMI::sequences()");
    text.resize(offsets[count]);
    if(text.empty()) { return; }
    gpuCheck(bwtm_sequences_extract(ix, nullptr, ids.first, count, max_len, offsets.data(), text.data(), text.size()), "FMI::sequences()");
  }

  template<class Format> void serialize(const std::string& filename) const;
  template<class Format> void load(const std::string& filename);

  BWT      bwt;
  Alphabet alpha;
};

// From BWT positions of an FMI back to its collection: (sequence id, offset of the suffix in that sequence) for the positions of a range, as
// FMI::find returns it (bwtm_locator_create, bwtm_locate_ranges: a sizing call, then the locating one).  The index goes to the device if it
// is not there, and stays; the table of `sequences` 64-bit entries is built there by one LF walk per sequence.  The locator borrows the FMI's
// device copy: build it after the last merge that involves the FMI, and drop it before the FMI.  No sequence may be longer than max_len
// (0: 65536).
class Locator
{
public:
  typedef BWT::size_type size_type;
  typedef std::pair<size_type, size_type> hit_type;                 // (sequence, offset)

  explicit Locator(const FMI& fmi, size_type max_len = 0)
  {
    gpuCheck(bwtm_locator_create(fmi.bwt.onDevice(fmi.alpha.C), max_len, &this->handle), "Locator::Locator()");
  }
  ~Locator() { bwtm_locator_free(this->handle); }
  Locator(const Locator&) = delete; Locator& operator=(const Locator&) = delete;

  size_type bytes() const { return bwtm_locator_bytes(this->handle); }

  // The hits of one range in ascending BWT position; max_hits > 0 keeps the first max_hits.
  std::vector<hit_type> locate(range_type range, size_type max_hits = 0) const
  {
    std::vector<size_type> hit_offsets; std::vector<hit_type> hits;
    this->locate(std::vector<range_type>(1, range), hit_offsets, hits, max_hits);
    return hits;
  }

  // The hits of every range: those of range r are hits[hit_offsets[r] .. hit_offsets[r + 1]).
  void locate(const std::vector<range_type>& ranges, std::vector<size_type>& hit_offsets, std::vector<hit_type>& hits, size_type max_hits = 0) const
  {
    std::vector<uint64_t> sp(ranges.size()), ep(ranges.size());
    for(size_type r = 0; r < ranges.size(); r++) { sp[r] = ranges[r].first; ep[r] = ranges[r].second; }
    hit_offsets.assign(ranges.size() + 1, 0); hits.clear();
    gpuCheck(bwtm_locate_ranges(this->handle, sp.data(), ep.data(), ranges.size(), max_hits, hit_offsets.data(), nullptr, nullptr, 0), "Locator::locate()");
    const size_type total = hit_offsets[ranges.size()];
    if(total == 0) { return; }
    std::vector<uint64_t> ids(total), offsets(total);
    gpuCheck(bwtm_locate_ranges(this->handle, sp.data(), ep.data(), ranges.size(), max_hits, hit_offsets.data(), ids.data(), offsets.data(), total), "Locator::locate()");
    hits.resize(total);
    for(size_type h = 0; h < total; h++) { hits[h] = hit_type(ids[h], offsets[h]); }
  }

  typedef std::pair<size_type, size_type> overlap_type;             // (target sequence, length of the overlap)

  // Suffix-prefix overlaps of the sequences ids.first .. ids.second with the collection (bwtm_overlap_sequences: a sizing call, then the real
  // one): those of the k-th query are hits[hit_offsets[k] .. hit_offsets[k + 1]), the first `length` symbols of `target` being the last
  // `length` symbols of the query, length >= min_overlap; longest first, then targets in BWT order.  A query's hit with itself over its
  // whole length is among them.  max_hits > 0 keeps the first max_hits hits of every query.
  void overlaps(range_type ids, size_type min_overlap, std::vector<size_type>& hit_offsets, std::vector<overlap_type>& hits, size_type max_hits = 0) const
  {
    const size_type count = (Range::empty(ids) ? 0 : Range::length(ids));
    hit_offsets.assign(count + 1, 0); hits.clear();
    if(count == 0) { return; }
    gpuCheck(bwtm_overlap_sequences(this->handle, nullptr, ids.first, count, min_overlap, max_hits, hit_offsets.data(), nullptr, nullptr, 0), "Locator::overlaps()");
    const size_type total = hit_offsets[count];
    if(total == 0) { return; }
    std::vector<uint64_t> targets(total), lengths(total);
    gpuCheck(bwtm_overlap_sequences(this->handle, nullptr, ids.first, count, min_overlap, max_hits, hit_offsets.data(), targets.data(), lengths.data(), total), "Locator::overlaps()");
    hits.resize(total);
    for(size_type h = 0; h < total; h++) { hits[h] = overlap_type(targets[h], lengths[h]); }
  }

private:
  bwtm_locator* handle = nullptr;
};

// The distinct k-mers of an FMI's collection with their counts and ranges, ascending, on the device (bwtm_kmers_create): k-mers over the
// four comp values 1..5 other than `skip` (the comp of N), 1 <= k <= 32, kept when they occur at least min_count times.  The index goes to
// the device if it is not there, and stays; the result does not borrow it.
class Kmers
{
public:
  typedef BWT::size_type size_type;

  Kmers(const FMI& fmi, size_type k, size_type skip, size_type min_count = 1) : k(k), skip(skip)
  {
    gpuCheck(bwtm_kmers_create(fmi.bwt.onDevice(fmi.alpha.C), (uint32_t)std::min<size_type>(k, ~(uint32_t)0), (uint32_t)std::min<size_type>(skip, ~(uint32_t)0), min_count,
      &this->handle), "Kmers::Kmers()");
  }
  ~Kmers() { bwtm_kmers_free(this->handle); }
  Kmers(const Kmers&) = delete; Kmers& operator=(const Kmers&) = delete;

  size_type distinct() const { return bwtm_kmers_distinct(this->handle); }
  size_type total() const { return bwtm_kmers_total(this->handle); }
  size_type bytes() const { return bwtm_kmers_bytes(this->handle); }
  const bwtm_kmers* device() const { return this->handle; }       // for the calls of include/bwtm.h that take the k-mers (bwt_unitigs)

  // The entries [first, first + count) in ascending order; sp may be null.
  void download(size_type first, size_type count, std::vector<uint64_t>& codes, std::vector<uint64_t>& counts, std::vector<uint64_t>* sp = nullptr) const
  {
    codes.resize(count); counts.resize(count);
    if(sp) { sp->resize(count); }
    gpuCheck(bwtm_kmers_download(this->handle, first, count, codes.data(), counts.data(), (sp ? sp->data() : nullptr)), "Kmers::download()");
  }

  // hist[j] = kept k-mers of count j, the last bin those of count >= bins - 1.
  std::vector<uint64_t> histogram(size_type bins) const
  {
    std::vector<uint64_t> hist(bins, 0);
    gpuCheck(bwtm_kmers_histogram(this->handle, bins, hist.data()), "Kmers::histogram()");
    return hist;
  }

  // Symbol j (0 = first) of a code as its comp value.
  byte_type comp(uint64_t code, size_type j) const
  {
    const size_type rank = (code >> (2 * (k - 1 - j))) & 3;
    return (byte_type)(rank + 1 + (rank + 1 >= skip ? 1 : 0));
  }

  const size_type k, skip;

private:
  friend class Corrector;
  bwtm_kmers* handle = nullptr;
};

// K-mer error correction of reads against the solid k-mers of a spectrum (bwtm_corrector_create): the k-mers of count >= threshold, copied
// out of `kmers`, which may be destroyed at once.  A read is made to consist of solid k-mers by single substitutions, one per round, at
// most max_rounds of them (the rule: include/bwtm.h); status is one of BWTM_CORRECT_*.
class Corrector
{
public:
  typedef BWT::size_type size_type;

  Corrector(const Kmers& kmers, size_type threshold) : k(kmers.k), skip(kmers.skip)
  {
    gpuCheck(bwtm_corrector_create(kmers.handle, (uint32_t)std::min<size_type>(kmers.skip, ~(uint32_t)0), threshold, &this->handle), "Corrector::Corrector()");
  }
  ~Corrector() { bwtm_corrector_free(this->handle); }
  Corrector(const Corrector&) = delete; Corrector& operator=(const Corrector&) = delete;

  size_type solid() const { return bwtm_corrector_solid(this->handle); }
  size_type bytes() const { return bwtm_corrector_bytes(this->handle); }

  // Reads from the host, laid out as for FMI::findApprox: read j = text[offsets[j] .. offsets[j + 1]), comp values.  corrected has the layout of text.
  void correct(const std::vector<byte_type>& text, const std::vector<uint64_t>& offsets, size_type max_rounds, std::vector<byte_type>& corrected,
               std::vector<byte_type>& status, std::vector<uint32_t>& edits) const
  {
    const size_type count = (offsets.empty() ? 0 : offsets.size() - 1);
    corrected.assign(text.size(), 0); status.assign(count, 0); edits.assign(count, 0);
    gpuCheck(bwtm_correct_batch(this->handle, text.data(), offsets.data(), count, (uint32_t)std::min<size_type>(max_rounds, ~(uint32_t)0), corrected.data(), status.data(),
      edits.data()), "Corrector::correct()");
  }

  // The sequences ids.first .. ids.second of fmi, extracted and corrected on the device: sequence j is text[offsets[j] .. offsets[j + 1]).
  // The index goes to the device if it is not there, and stays.
  void sequences(const FMI& fmi, range_type ids, size_type max_rounds, std::vector<size_type>& offsets, std::vector<byte_type>& text, std::vector<byte_type>& status,
                 std::vector<uint32_t>& edits, size_type max_len = 0) const
  {
    const size_type count = (ids.second >= ids.first ? ids.second - ids.first + 1 : 0);
    offsets.assign(count + 1, 0); text.clear(); status.assign(count, 0); edits.assign(count, 0);
    if(count == 0) { return; }
    bwtm_index* ix = fmi.bwt.onDevice(fmi.alpha.C);
    gpuCheck(bwtm_sequences_extract(ix, nullptr, ids.first, count, max_len, offsets.data(), nullptr, 0), "Corrector::sequences()");       // the size
    text.resize(offsets[count]);
    gpuCheck(bwtm_correct_sequences(this->handle, ix, nullptr, ids.first, count, max_len, (uint32_t)std::min<size_type>(max_rounds, ~(uint32_t)0), offsets.data(),
      text.data(), text.size(), status.data(), edits.data()), "Corrector::sequences()");
  }

  const size_type k, skip;

private:
  bwtm_corrector* handle = nullptr;
};

// The k-mers of two FMIs' collections side by side, ascending, on the device (bwtm_kmer_join_create): every kept k-mer with its count and
// its insertion point in each.  A k-mer is kept when min_a <= count in a <= max_a, min_b <= count in b <= max_b and the two counts add up to
// min_sum or more; NO_BOUND is no upper bound.  Both indexes go to the device if they are not there, and stay; the result borrows neither.
// The two alphabets must be the same one: a code means the same string on both sides.
class KmerJoin
{
public:
  typedef BWT::size_type size_type;
  constexpr static size_type NO_BOUND = ~(size_type)0;
  constexpr static size_type STATS = 7;

  KmerJoin(const FMI& a, const FMI& b, size_type k, size_type skip, size_type min_a = 0, size_type max_a = NO_BOUND, size_type min_b = 0, size_type max_b = NO_BOUND,
    size_type min_sum = 1) : k(k), skip(skip)
  {
    if(a.alpha != b.alpha)
    {
      std::cerr << "KmerJoin::KmerJoin(): Cannot compare BWTs with different alphabets" << std::endl;
      std::exit(EXIT_FAILURE);
    }
    const bwtm_index* da = a.bwt.onDevice(a.alpha.C);
    const bwtm_index* db = (&a == &b ? da : b.bwt.onDevice(b.alpha.C));
    gpuCheck(bwtm_kmer_join_create(da, db, (uint32_t)std::min<size_type>(k, ~(uint32_t)0), (uint32_t)std::min<size_type>(skip, ~(uint32_t)0), min_a, max_a, min_b, max_b, min_sum,
      &this->handle), "KmerJoin::KmerJoin()");
  }
  ~KmerJoin() { bwtm_kmer_join_free(this->handle); }
  KmerJoin(const KmerJoin&) = delete; KmerJoin& operator=(const KmerJoin&) = delete;

  size_type distinct() const { return bwtm_kmer_join_distinct(this->handle); }
  size_type bytes() const { return bwtm_kmer_join_bytes(this->handle); }

  // The entries [first, first + count) in ascending order; the insertion points may be null.
  void download(size_type first, size_type count, std::vector<uint64_t>& codes, std::vector<uint64_t>& count_a, std::vector<uint64_t>& count_b,
    std::vector<uint64_t>* sp_a = nullptr, std::vector<uint64_t>* sp_b = nullptr) const
  {
    codes.resize(count); count_a.resize(count); count_b.resize(count);
    if(sp_a) { sp_a->resize(count); }
    if(sp_b) { sp_b->resize(count); }
    gpuCheck(bwtm_kmer_join_download(this->handle, first, count, codes.data(), count_a.data(), count_b.data(), (sp_a ? sp_a->data() : nullptr), (sp_b ? sp_b->data() : nullptr)),
      "KmerJoin::download()");
  }

  // k-mers only in a, only in b, in both; occurrences in a of the first, in b of the second, in a and in b of the third.
  std::vector<uint64_t> summary() const
  {
    std::vector<uint64_t> stats(STATS, 0);
    gpuCheck(bwtm_kmer_join_summary(this->handle, stats.data()), "KmerJoin::summary()");
    return stats;
  }

  // Symbol j (0 = first) of a code as its comp value.
  byte_type comp(uint64_t code, size_type j) const
  {
    const size_type rank = (code >> (2 * (k - 1 - j))) & 3;
    return (byte_type)(rank + 1 + (rank + 1 >= skip ? 1 : 0));
  }

  const size_type k, skip;

private:
  bwtm_kmer_join* handle = nullptr;
};

// Search phase (buildRA, reference fmi.cpp:272-334) as a free function: makes sure a and b are on the device and
// fills a device rank array; parameters.sequence_blocks splits the sequences of b.
inline void buildRA(const FMI& a, const FMI& b, const MergeParameters& parameters, RankArray& ra)
{
  ra.clear();
  ra.a = a.bwt.onDevice(a.alpha.C);
  ra.b = b.bwt.onDevice(b.alpha.C);
  gpuCheck(bwtm_ra_create(ra.a, ra.b, &ra.handle), "buildRA()");
  if(b.sequences() == 0) { return; }
  for(range_type block : getBounds(range_type(0, b.sequences() - 1), parameters.sequence_blocks))
  {
    gpuCheck(bwtm_search(ra.a, ra.b, block.first, block.second, ra.handle), "buildRA()");
  }
}

// The output buffers of bwtm_merge_host are the result's own page-locked arrays.
inline void* mergeSink(void* user, int what, uint64_t nbytes)
{
  BWT* bwt = (BWT*)user;
  switch(what)
  {
  case BWTM_BUF_DATA:      bwt->data.bytes.resizeUninitialized(std::max<uint64_t>(nbytes, 1)); bwt->data.bytes.resizeUninitialized(nbytes); return bwt->data.bytes.data();
  case BWTM_BUF_BLOCK_END: bwt->block_end.resizeUninitialized(std::max<uint64_t>(nbytes / sizeof(size_type), 1)); bwt->block_end.resizeUninitialized(nbytes / sizeof(size_type)); return bwt->block_end.data();
  case BWTM_BUF_CUM:       bwt->cum_flat.resizeUninitialized(nbytes / sizeof(size_type)); return bwt->cum_flat.data();
  case BWTM_BUF_ANCHORS:   bwt->anchors.resizeUninitialized(std::max<uint64_t>(nbytes / sizeof(size_type), 1)); bwt->anchors.resizeUninitialized(nbytes / sizeof(size_type)); return bwt->anchors.data();
  case BWTM_BUF_FIELDS:    bwt->fields.resizeUninitialized(std::max<uint64_t>((nbytes + 1) / 2, 1)); bwt->fields.resizeUninitialized((nbytes + 1) / 2); return bwt->fields.data();
  }
  return nullptr;
}

// The sink of bwtm_merge_host_streamed: the pieces' bytes are appended to the result's page-locked data, their fields kept per row at the
// widest width seen so far (a narrower piece is widened on the way in, a wider one widens what is there) and laid out as
// fields[6][blocks] / anchors[6][ceil(blocks / 64)] when the last piece has arrived.
struct PieceAssembler
{
  BWT* bwt = nullptr;
  int width = 1;
  size_type blocks = 0, reserved = 0;                   // (the data array grows geometrically: a piece may be a few KB)
  bool too_wide = false;                                // a piece in the full form: a block of 2^32 - 1 positions or more
  std::vector<std::uint8_t> rows[BWT::SIGMA];
  std::vector<uint64_t> anch[BWT::SIGMA];

  static uint64_t get(const void* p, int w, size_type k)
  {
    return (w == 1 ? (uint64_t)((const std::uint8_t*)p)[k] : (w == 2 ? (uint64_t)((const std::uint16_t*)p)[k] : (uint64_t)((const std::uint32_t*)p)[k]));
  }
  static void put(std::uint8_t* p, int w, size_type k, uint64_t v)
  {
    if(w == 1) { p[k] = (std::uint8_t)v; } else if(w == 2) { ((std::uint16_t*)p)[k] = (std::uint16_t)v; } else { ((std::uint32_t*)p)[k] = (std::uint32_t)v; }
  }
  void widen(int to)
  {
    for(size_type c = 0; c < BWT::SIGMA; c++)
    {
      std::vector<std::uint8_t> wide(blocks * (size_type)to);
      for(size_type k = 0; k < blocks; k++) { put(wide.data(), to, k, get(rows[c].data(), width, k)); }
      rows[c].swap(wide);
    }
    width = to;
  }
  static int sink(void* user, const bwtm_piece* piece)
  {
    PieceAssembler& self = *(PieceAssembler*)user;
    HostArray<byte_type>& bytes = self.bwt->data.bytes;
    const size_type old = bytes.size();
    if(piece->nbytes > 0)
    {
      if(old + piece->nbytes > self.reserved) { self.reserved = std::max<size_type>(old + piece->nbytes, 2 * self.reserved); bytes.reserve(self.reserved); }
      bytes.resizeUninitialized(old + piece->nbytes);
      std::memcpy(bytes.data() + old, piece->data, piece->nbytes);
    }
    const size_type ns = piece->sample_blocks;
    if(ns == 0) { return 0; }
    if(piece->sample_width == 8) { self.too_wide = true; return 1; }
    if(piece->sample_width > self.width) { self.widen(piece->sample_width); }
    for(size_type c = 0; c < BWT::SIGMA; c++)
    {
      self.rows[c].resize((self.blocks + ns) * (size_type)self.width);
      for(size_type k = 0; k < ns; k++) { put(self.rows[c].data(), self.width, self.blocks + k, get(piece->fields, piece->sample_width, c * ns + k)); }
      self.anch[c].insert(self.anch[c].end(), piece->anchors + c * piece->nanchors, piece->anchors + (c + 1) * piece->nanchors);
    }
    self.blocks += ns;
    return 0;
  }
  void finish()
  {
    const size_type nanch = (blocks + 63) / 64, row_bytes = blocks * (size_type)width;
    bwt->data.bytes.reserve(1);
    bwt->anchors.resizeUninitialized(std::max<size_type>(BWT::SIGMA * nanch, 1)); bwt->anchors.resizeUninitialized(BWT::SIGMA * nanch);
    bwt->fields.resizeUninitialized(std::max<size_type>((BWT::SIGMA * row_bytes + 1) / 2, 1)); bwt->fields.resizeUninitialized((BWT::SIGMA * row_bytes + 1) / 2);
    for(size_type c = 0; c < BWT::SIGMA; c++)
    {
      if(row_bytes > 0) { std::memcpy((std::uint8_t*)bwt->fields.data() + c * row_bytes, rows[c].data(), row_bytes); }
      std::copy(anch[c].begin(), anch[c].end(), bwt->anchors.begin() + c * nanch);
    }
  }
};

inline FMI::FMI(FMI& a, FMI& b, MergeParameters parameters)
{
  if(a.alpha != b.alpha)
  {
    std::cerr << "FMI::FMI(): Cannot merge BWTs with different alphabets" << std::endl;
    std::exit(EXIT_FAILURE);
  }
#ifdef VERBOSE_STATUS_INFO
  // the reference's progress lines on stderr (fmi.cpp:344-364, bwt.cpp:300-313), with the device's phases behind them
  std::cerr << "bwt_merge: " << a.sequences() << " sequences of total length " << a.size() << std::endl;
  std::cerr << "bwt_merge: Adding " << b.sequences() << " sequences of total length " << b.size() << std::endl;
  std::cerr << "bwt_merge: Memory usage before merging: " << inGigabytes(memoryUsage()) << " GB" << std::endl;
  double verbose_start = readTimer();
#endif
  Alphabet merged = a.alpha;
  for(size_type c = 0; c <= merged.sigma; c++) { merged.C[c] += b.alpha.C[c]; }
  this->bwt.header.sequences = a.sequences() + b.sequences();
  this->bwt.header.bases = a.size() + b.size();
  this->bwt.header.setOrder(a.bwt.header.order());
  if(parameters.lazy_host)
  {
    // Device only: the result is the next merge's first input; nothing is encoded or downloaded now.
    bwtm_index* A = a.bwt.onDevice(a.alpha.C); bwtm_index* B = b.bwt.onDevice(b.alpha.C);
    bwtm_ra* ra = nullptr; bwtm_index* M = nullptr;
    gpuCheck(bwtm_ra_create(A, B, &ra), "FMI::FMI()");
    if(b.sequences() > 0) { gpuCheck(bwtm_search(A, B, 0, b.sequences() - 1, ra), "FMI::FMI()"); }
    gpuCheck(bwtm_ra_finalize(ra), "FMI::FMI()");
#ifdef VERBOSE_STATUS_INFO
    double verbose_mid = readTimer();
    std::cerr << "bwt_merge: RA built in " << (verbose_mid - verbose_start) << " seconds" << std::endl;
#endif
    gpuCheck(bwtm_interleave(A, B, ra, &M), "FMI::FMI()");
    bwtm_ra_free(ra);
    a.bwt.clear(); b.bwt.clear();
    this->bwt.adopt(M);
#ifdef VERBOSE_STATUS_INFO
    gpuCheck(bwtm_synchronize(), "FMI::FMI()");
    std::cerr << "bwt_merge: BWTs merged in " << (readTimer() - verbose_mid) << " seconds (the result stays on the device)" << std::endl;
#endif
  }
  else if(parameters.streamed)
  {
    // Host to host with the second half in slices (bwtm_merge_host_streamed): the pieces are assembled into this object's arrays.
    std::vector<uint64_t> cb(b.alpha.C.begin(), b.alpha.C.end()), ca(a.alpha.C.begin(), a.alpha.C.end());
    const BlockArray& bdata = b.bwt.hostData();
    bwtm_host_input hb = { bdata.data(), bdata.size(), b.sequences(), b.size(), cb.data() };
    b.bwt.dropDevice();                                   // an announced upload of b is not used by this form
    bwtm_host_output out;
    bwtm_stream_stats stats;
    PieceAssembler pieces; pieces.bwt = &this->bwt;
    this->bwt.data.bytes.resizeUninitialized(0);
    int rc = BWTM_OK;
    gpuCheck(bwtm_tune("stream_upload", parameters.stream_upload ? 1 : 0), "FMI::FMI()");
    if(a.bwt.deviceResident())
    {
      rc = bwtm_merge_host_streamed(a.bwt.releaseDevice(), nullptr, &hb, parameters.slice_records, BWTM_SAMPLES_COMPACT, PieceAssembler::sink, &pieces, &out, &stats);
    }
    else
    {
      const BlockArray& adata = a.bwt.hostData();
      bwtm_host_input ha = { adata.data(), adata.size(), a.sequences(), a.size(), ca.data() };
      rc = bwtm_merge_host_streamed(nullptr, &ha, &hb, parameters.slice_records, BWTM_SAMPLES_COMPACT, PieceAssembler::sink, &pieces, &out, &stats);
    }
    if(pieces.too_wide)
    {
      std::cerr << "FMI::FMI(): a block of the result encodes 2^32 - 1 positions or more; merge without MergeParameters::streamed" << std::endl;
      std::exit(EXIT_FAILURE);
    }
    gpuCheck(rc, "FMI::FMI()");
    pieces.finish();
    this->bwt.adoptHost(nullptr, out.blocks, pieces.width);
    a.bwt.clear(); b.bwt.clear();
#ifdef VERBOSE_STATUS_INFO
    std::cerr << "bwt_merge: RA built in " << (stats.ms_upload + stats.ms_search) / 1000.0 << " seconds" << std::endl;
    std::cerr << "bwt_merge: BWTs merged in " << stats.ms_second_half / 1000.0 << " seconds (" << stats.pieces << " pieces, slices of " << stats.slice_records
              << " records, at most " << stats.slice_bytes_peak << " bytes of slices on the device)" << std::endl;
#endif
  }
  else
  {
    // Host to host in one pipelined call (bwtm_merge_host): b is uploaded from its page-locked bytes, a likewise unless it
    // is already on the device (the result of the previous merge); data and samples land in this object's arrays.
    std::vector<uint64_t> cb(b.alpha.C.begin(), b.alpha.C.end()), ca(a.alpha.C.begin(), a.alpha.C.end());
    const BlockArray& bdata = b.bwt.hostData();
    bwtm_host_input hb = { bdata.data(), bdata.size(), b.sequences(), b.size(), cb.data() };
    bwtm_host_output out;
    bwtm_index* kept = nullptr;
    bwtm_upload* b_pending = (b.bwt.deviceResident() ? nullptr : b.bwt.releasePending());   // announced while the previous merge ran
    b.bwt.dropDevice();
    if(a.bwt.deviceResident() && b_pending)
    {
      gpuCheck(bwtm_merge_host_pipelined(a.bwt.releaseDevice(), nullptr, nullptr, b_pending, nullptr, nullptr, mergeSink, &this->bwt, BWTM_SAMPLES_COMPACT, &out, &kept),
        "FMI::FMI()");
    }
    else if(a.bwt.deviceResident())
    {
      gpuCheck(bwtm_merge_host_chained(a.bwt.releaseDevice(), &hb, mergeSink, &this->bwt, BWTM_SAMPLES_COMPACT, &out, &kept), "FMI::FMI()");
    }
    else
    {
      const BlockArray& adata = a.bwt.hostData();
      bwtm_host_input ha = { adata.data(), adata.size(), a.sequences(), a.size(), ca.data() };
      if(b_pending) { gpuCheck(bwtm_merge_host_pipelined(nullptr, &ha, nullptr, b_pending, nullptr, nullptr, mergeSink, &this->bwt, BWTM_SAMPLES_COMPACT, &out, &kept), "FMI::FMI()"); }
      else { gpuCheck(bwtm_merge_host(&ha, &hb, mergeSink, &this->bwt, BWTM_SAMPLES_COMPACT, &out, &kept), "FMI::FMI()"); }
    }
    this->bwt.adoptHost(kept, out.blocks, out.sample_width);
    a.bwt.clear(); b.bwt.clear();
#ifdef VERBOSE_STATUS_INFO
    std::cerr << "bwt_merge: RA built in " << (out.ms_upload + out.ms_search) / 1000.0 << " seconds" << std::endl;
    std::cerr << "bwt_merge: BWTs merged in " << (out.ms_interleave + out.ms_encode_download) / 1000.0 << " seconds" << std::endl;
    std::cerr << "bwt_merge: rank/select built in " << out.ms_samples / 1000.0 << " seconds" << std::endl;
#endif
  }
  this->alpha = merged;
  warnIfPoolExhausted("FMI::FMI()");
}

//------------------------------------------------------------------------------
// Formats.

template<>
inline void FMI::serialize<NativeFormat>(const std::string& filename) const
{
  std::ofstream out(filename.c_str(), std::ios_base::binary);
  if(!out) { std::cerr << "FMI::serialize(): Cannot open output file " << filename << std::endl; return; }
  bwt.serialize(out);
  // Alphabet: char2comp int_vector<8>, comp2char int_vector<8>, C int_vector<64>, u64 sigma.
  sdsl_compat::PackedVector c2c(alpha.char2comp.size(), 8), c2ch(alpha.comp2char.size(), 8), cc(alpha.C.size(), 64);
  for(size_type k = 0; k < alpha.char2comp.size(); k++) { c2c.set(k, alpha.char2comp[k]); }
  for(size_type k = 0; k < alpha.comp2char.size(); k++) { c2ch.set(k, alpha.comp2char[k]); }
  for(size_type k = 0; k < alpha.C.size(); k++) { cc.set(k, alpha.C[k]); }
  c2c.serialize(out, false); c2ch.serialize(out, false); cc.serialize(out, false);
  sdsl_compat::write_member(alpha.sigma, out);
}

template<>
inline void FMI::load<NativeFormat>(const std::string& filename)
{
  std::ifstream stream(filename.c_str(), std::ios_base::binary);
  if(!stream) { std::cerr << "FMI::load(): Cannot open input file " << filename << std::endl; std::exit(EXIT_FAILURE); }
  Source in(stream, filename, "FMI::load()");
  bwt.load(in);
  sdsl_compat::PackedVector c2c, c2ch, cc;
  c2c.load(in, false, 8, "char2comp"); c2ch.load(in, false, 8, "comp2char"); cc.load(in, false, 64, "the C array");
  alpha.sigma = in.get<size_type>("sigma");
  if(in.remaining() != 0) { in.refuse(std::to_string(in.remaining()) + " bytes behind the last member"); }
  // The alphabet is this format's: 256 / 6 / 7 entries, C the prefix sums of what the samples count, the header's order flag its order.
  if(alpha.sigma != BWT::SIGMA || c2c.count != Alphabet::MAX_SIGMA || c2ch.count != BWT::SIGMA || cc.count != BWT::SIGMA + 1)
  {
    in.refuse("the alphabet is not one of " + std::to_string(BWT::SIGMA) + " symbols");
  }
  alpha.char2comp.resize(c2c.count); alpha.comp2char.resize(c2ch.count); alpha.C.resize(cc.count);
  for(size_type k = 0; k < c2c.count; k++) { alpha.char2comp[k] = (byte_type)c2c.get(k); }
  for(size_type k = 0; k < c2ch.count; k++) { alpha.comp2char[k] = (byte_type)c2ch.get(k); }
  for(size_type k = 0; k < cc.count; k++) { alpha.C[k] = cc.get(k); }
  size_type before = 0;
  for(size_type c = 0; c < BWT::SIGMA; c++)
  {
    if(alpha.C[c] != before) { in.refuse("the C array is not the prefix sums of the symbol counts"); }
    before += bwt.count((comp_type)c);
  }
  if(alpha.C[BWT::SIGMA] != before) { in.refuse("the C array is not the prefix sums of the symbol counts"); }
  for(size_type k = 0; k < Alphabet::MAX_SIGMA; k++) { if(alpha.char2comp[k] >= BWT::SIGMA) { in.refuse("char2comp maps a character outside the alphabet"); } }
  if(bwt.header.flags != (std::uint32_t)identifyAlphabet(alpha)) { in.refuse("the header's flags are not the alphabetic order of the alphabet"); }
}

// Foreign formats (reference FMI::load / serialize<Format>, fmi.h:114-134; BWT::load<Format>, bwt.h:90-104).
// The file's items become maximal runs first (RunBuffer) and are mapped to comp values afterwards, like the
// reference does (formats.cpp:147-156: 'a' next to 'A' stays two runs); comp values outside the alphabet map to 0
// (the identity alphabet of formats.cpp:228, support.cpp:100-104).
template<class Format>
inline void FMI::load(const std::string& filename)
{
  std::ifstream stream(filename.c_str(), std::ios_base::binary);
  if(!stream) { std::cerr << "BWT::load(): Cannot open input file " << filename << std::endl; std::exit(EXIT_FAILURE); }
  Source in(stream, filename, std::string(Format::name()) + " loader");
  const Alphabet order_alpha = createAlphabet(Format::order());
  bwt.data.clear();
  RunBuffer run_buffer;
  auto emit_run = [&](range_type run)
  {
    size_type comp = (Format::characters ? order_alpha.char2comp[run.first & 0xFF] : (run.first < BWT::SIGMA ? run.first : 0));
    Run::write(bwt.data, (comp_type)comp, run.second);
  };
  Format::decode(in, [&](size_type value, size_type length) { if(run_buffer.add(value, length)) { emit_run(run_buffer.run); } });
  run_buffer.flush(); emit_run(run_buffer.run);
  bwt.buildFromData(Format::order());
  std::vector<size_type> counts(BWT::SIGMA);
  for(size_type c = 0; c < BWT::SIGMA; c++) { counts[c] = bwt.count(c); }
  alpha = Alphabet(counts, order_alpha.char2comp, order_alpha.comp2char);
  bwt.header.setOrder(identifyAlphabet(alpha));
}

template<class Format>
inline void FMI::serialize(const std::string& filename) const
{
  if(!compatible(alpha, Format::order()))
  {
    std::cerr << "FMI::serialize(): Warning: " << Format::name() << " is not compatible with "
              << alphabetName(identifyAlphabet(alpha)) << " alphabets!" << std::endl;
  }
  std::ofstream out(filename.c_str(), std::ios_base::binary);
  if(!out) { std::cerr << "BWT::serialize(): Cannot open output file " << filename << std::endl; return; }
  const Alphabet order_alpha = createAlphabet(Format::order());
  Format::encode(out, bwt.header, [&](auto&& f)
  {
    const BlockArray& data = bwt.hostData();
    size_type left = bwt.size();
    for(size_type rle_pos = 0; rle_pos < data.size(); )
    {
      range_type run = Run::read(data, rle_pos);
      if(run.second > left)                                 // damaged data: a run of 2^60 positions must not be written out
      {
        std::cerr << "FMI::serialize(): " << filename << ": the data decodes to more than the header's " << bwt.size() << " bases" << std::endl;
        std::exit(EXIT_FAILURE);
      }
      left -= run.second;
      f((size_type)(Format::characters ? order_alpha.comp2char[run.first] : run.first), run.second);
    }
  });
}

inline void serialize(const FMI& fmi, const std::string& filename, const std::string& format)
{
  if(!withFormat(format, [&](auto f) { fmi.serialize<decltype(f)>(filename); }))
  {
    std::cerr << "serialize(): Invalid BWT format: " << format << std::endl; std::exit(EXIT_FAILURE);
  }
}

inline void load(FMI& fmi, const std::string& filename, const std::string& format)
{
  if(!withFormat(format, [&](auto f) { fmi.load<decltype(f)>(filename); }))
  {
    std::cerr << "load(): Invalid BWT format: " << format << std::endl; std::exit(EXIT_FAILURE);
  }
}

// Bytes the native serialization takes (stands in for sdsl::size_in_bytes in the size report).
inline size_type sizeInBytes(const FMI& fmi)
{
  struct Counter : std::streambuf { size_type n = 0; std::streamsize xsputn(const char*, std::streamsize k) override { n += k; return k; } int overflow(int c) override { n++; return c; } };
  // Exact for data, header and alphabet; the Elias-Fano samples are estimated from their parameters
  // (2 + log2(n / m) bits per block), serializing them only to count bytes would take seconds.
  size_type blocks = fmi.bwt.blocks();
  size_type total = 24 + 8 + fmi.bwt.hostData().blocks() * BlockArray::BLOCK_SIZE + 256 + 6 + 7 * 8 + 8 + 3 * 8;
  for(size_type c = 0; c <= BWT::SIGMA; c++)
  {
    size_type universe = (c < BWT::SIGMA ? fmi.bwt.count((comp_type)c) + blocks : fmi.size());
    size_type per = 2 + (blocks > 0 && universe > blocks ? bit_length(universe / blocks) : 1);
    total += blocks * per / 8 + 64;
  }
  return total;
}

} // namespace bwtmerge

#endif // BWTM_HOST_FMI_H
