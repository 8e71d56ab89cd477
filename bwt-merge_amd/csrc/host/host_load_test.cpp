/*
  host_load_test FILE FORMAT -- loads a file through the facade's load(fmi, file, format) and uses the index the way the tools do:
  the scalar queries, one decode of the whole run stream, and a re-serialisation as native and as plain_default (to /dev/null).
  It then prints ONE line that describes everything the load produced, and recomputes the consistency of the samples on its own.

  Exit codes: 0 = loaded (the line is on stdout), 1 = refused (the facade's own exit(EXIT_FAILURE), its message on stderr); anything
  else -- a signal, an uncaught exception, a sanitizer's exit code -- is a failure of the code under test.

  Host code only, and built to stay that way: it is linked against host_load_stubs.cpp instead of libbwtm.so, so no call can reach a
  device and HostArray takes its memory from malloc, where a sanitized build (make host_load_test_san) sees every access.
  tests/test_loaders_host.py runs it on truncated and corrupted files.
*/
#include "fmi.h"

using namespace bwtmerge;

size_type Parallel::max_threads = 1;

template<class Array>
static size_type hashOf(const Array& array, size_type seed = FNV_OFFSET_BASIS)
{
  const byte_type* p = (const byte_type*)array.data();
  for(size_type k = 0; k < array.size() * sizeof(typename Array::value_type); k++) { seed = fnv1a_hash(p[k], seed); }
  return seed;
}

// The checks a loaded index must pass whatever the file said, from the public arrays alone; the first that fails, or "ok".
static const char* consistency(const FMI& fmi)
{
  const BWT& bwt = fmi.bwt;
  if(bwt.sample_width != 8) { return "compact_samples"; }
  const size_type blocks = bwt.blocks();
  if(blocks != (bwt.data.size() + 63) / 64) { return "blocks_vs_bytes"; }
  if(bwt.block_end.size() != blocks || bwt.cum_flat.size() != BWT::SIGMA * (blocks + 1)) { return "array_sizes"; }
  size_type total = 0;
  for(size_type c = 0; c < BWT::SIGMA; c++)
  {
    std::vector<size_type> row = bwt.cumulative(c);
    if(row.size() != blocks + 1 || row[0] != 0) { return "row_start"; }
    for(size_type k = 0; k < blocks; k++) { if(row[k + 1] < row[k]) { return "row_decreases"; } }
    if(row[blocks] > bwt.size() - total) { return "totals_exceed_bases"; }
    total += row[blocks];
    if(fmi.alpha.C.size() != BWT::SIGMA + 1 || fmi.alpha.C[c + 1] - fmi.alpha.C[c] != row[blocks]) { return "C_vs_totals"; }
  }
  if(total != bwt.size()) { return "totals_vs_bases"; }
  if(bwt.count(0) != bwt.sequences()) { return "endmarkers_vs_sequences"; }
  if(fmi.alpha.C[0] != 0) { return "C_start"; }
  for(size_type k = 1; k < blocks; k++) { if(bwt.block_end[k] <= bwt.block_end[k - 1]) { return "block_end_order"; } }
  if(blocks > 0 && bwt.block_end[blocks - 1] != bwt.size() - 1) { return "block_end_last"; }
  if(blocks == 0 && bwt.size() != 0) { return "bases_without_blocks"; }
  if(fmi.alpha.sigma != BWT::SIGMA || fmi.alpha.char2comp.size() != 256 || fmi.alpha.comp2char.size() != BWT::SIGMA) { return "alphabet_sizes"; }
  return "ok";
}

int main(int argc, char** argv)
{
  if(argc != 3) { std::cerr << "Usage: host_load_test FILE FORMAT" << std::endl; return 2; }
  FMI fmi; load(fmi, argv[1], argv[2]);
  const BWT& bwt = fmi.bwt;

  const char* verdict = consistency(fmi);

  // the queries of the tools, at a spread of positions (their results feed one hash)
  size_type queries = FNV_OFFSET_BASIS;
  auto mix = [&](size_type v) { for(size_type b = 0; b < 8; b++) { queries = fnv1a_hash((byte_type)(v >> (8 * b)), queries); } };
  for(size_type c = 0; c < BWT::SIGMA; c++) { mix(bwt.count((comp_type)c)); }
  const size_type n = bwt.size();
  for(size_type k = 0; k <= 16; k++)
  {
    const size_type pos = (n / 16) * k + (k % 3);
    for(size_type c = 0; c < BWT::SIGMA; c++) { mix(bwt.rank(pos, (comp_type)c)); }
    range_type t = bwt.inverse_select(pos); mix(t.first); mix(t.second);
  }
  mix(bwt.rank(n, 0)); mix(bwt.rank(n + 1, 5)); mix(bwt.inverse_select(n ? n - 1 : 0).first);

  // one decode of the whole stream
  size_type runs = 0, decoded = 0, stream = FNV_OFFSET_BASIS;
  for(size_type rle_pos = 0; rle_pos < bwt.data.size(); )
  {
    range_type run = Run::read(bwt.data, rle_pos);
    runs++; decoded += run.second;
    stream = fnv1a_hash((byte_type)run.first, stream);
    for(size_type b = 0; b < 8; b++) { stream = fnv1a_hash((byte_type)(run.second >> (8 * b)), stream); }
  }

  serialize(fmi, "/dev/null", "native");
  serialize(fmi, "/dev/null", "plain_default");

  size_type cum = FNV_OFFSET_BASIS;
  for(size_type c = 0; c < BWT::SIGMA; c++) { cum = hashOf(bwt.cumulative(c), cum); }
  std::cout << std::hex << "loaded flags=" << bwt.header.flags << std::dec << " sequences=" << bwt.sequences() << " bases=" << bwt.size()
            << " bytes=" << bwt.data.size() << std::hex << " data=" << hashOf(bwt.data.bytes) << std::dec << " blocks=" << bwt.blocks()
            << std::hex << " block_end=" << hashOf(bwt.block_end) << " cum=" << cum
            << " char2comp=" << hashOf(fmi.alpha.char2comp) << " comp2char=" << hashOf(fmi.alpha.comp2char) << " C=" << hashOf(fmi.alpha.C)
            << std::dec << " sigma=" << fmi.alpha.sigma << " runs=" << runs << " decoded=" << decoded << std::hex << " stream=" << stream
            << " queries=" << queries << std::dec << " consistent=" << verdict << std::endl;
  return 0;
}
