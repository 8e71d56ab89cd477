/*
  host_sequences_test -- FMI::sequences on the GPU against the reads an index was built from (tests/test_gpu_facade_sequences.py).
  Usage: host_sequences_test index.bwt reads.txt     (native index; reads.txt: one read per line in the index's characters)
  Exit status 0 and "sequences ok" when every checked range equals the lines of the file.
*/
#include "fmi.h"

using namespace bwtmerge;

size_type Parallel::max_threads = 1;

static size_type failures = 0;

static void checkRange(const FMI& fmi, const std::vector<std::string>& reads, size_type first, size_type last, size_type max_len)
{
  std::vector<size_type> offsets(3, 77); std::vector<byte_type> text(5, 9);     // left-overs of an earlier use must not survive
  fmi.sequences(range_type(first, last), offsets, text, max_len);
  const size_type count = (first + 1 > last + 1 ? 0 : last + 1 - first);
  bool ok = (offsets.size() == count + 1 && offsets[0] == 0 && offsets[count] == text.size());
  for(size_type k = 0; ok && k < count; k++)
  {
    const std::string& want = reads[first + k];
    ok = (offsets[k + 1] - offsets[k] == want.size());
    for(size_type j = 0; ok && j < want.size(); j++)
    {
      const byte_type comp = text[offsets[k] + j];
      ok = (comp >= 1 && comp <= 5 && (char)fmi.alpha.comp2char[comp] == want[j]);
    }
    if(!ok) { std::cerr << "sequences [" << first << ", " << last << "]: sequence " << (first + k) << " differs from the read" << std::endl; }
  }
  if(!ok) { failures++; }
}

int main(int argc, char** argv)
{
  if(argc < 3) { std::cerr << "Usage: host_sequences_test index.bwt reads.txt" << std::endl; return 2; }
  gpuCheck(bwtm_init(0), "host_sequences_test");
  FMI fmi; load(fmi, argv[1], NativeFormat::tag());
  std::vector<std::string> reads;
  {
    std::ifstream in(argv[2], std::ios_base::binary);
    if(!in) { std::cerr << "host_sequences_test: Cannot open " << argv[2] << std::endl; return 2; }
    for(std::string line; std::getline(in, line); ) { reads.push_back(line); }
  }
  const size_type m = fmi.sequences();
  if(m != reads.size() || m < 8) { std::cerr << "host_sequences_test: " << m << " sequences, " << reads.size() << " reads" << std::endl; return 1; }
  size_type longest = 0;
  for(const std::string& r : reads) { longest = std::max<size_type>(longest, r.size()); }

  checkRange(fmi, reads, 0, m - 1, 0);                         // everything, the default bound
  checkRange(fmi, reads, 0, m - 1, longest);                   // the tightest bound that still holds
  checkRange(fmi, reads, m / 3, m / 3 + 6, 0);                 // a range that is no multiple of a quad
  checkRange(fmi, reads, m - 1, m - 1, 0);                     // the last sequence alone
  checkRange(fmi, reads, 5, 4, 0);                             // the empty range
  // the index is still the one that was loaded, and serves the facade's other queries
  if(!fmi.bwt.deviceResident()) { std::cerr << "the index did not stay on the device" << std::endl; failures++; }

  if(failures > 0) { std::cerr << failures << " checks failed" << std::endl; return 1; }
  std::cout << "sequences ok" << std::endl;
  return 0;
}
