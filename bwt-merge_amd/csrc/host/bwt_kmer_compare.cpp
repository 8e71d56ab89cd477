/*
  bwt_kmer_compare -- the k-mers of the reads of two BWT files side by side: which k-mers the two collections share and which only one of
  them holds (sample against sample, reads against a reference, a new batch against the index it is about to be merged into).  The
  reference has no such tool.  The suffix tries of both indexes are walked down together to depth k on the GPU (KmerJoin,
  bwtm_kmer_join_create): neither list of k-mers comes to the host on its own, and nothing is joined there.  A k-mer is a string of k
  characters other than N that occurs inside a read of either input.
  The output holds one line per kept k-mer,
      kmer <TAB> count in input1 <TAB> count in input2
  in ascending order of the k-mers (the order of the files' alphabet); with -S the seven numbers of the summary, one
      name <TAB> value
  per line.  The list is written in slices, so the host never holds the whole of it.
*/
#include <unistd.h>

#include "fmi.h"

using namespace bwtmerge;

size_type Parallel::max_threads = std::max(1u, std::thread::hardware_concurrency());

// entries per download
static const size_type SLICE = size_type(1) << 22;

static const char* const STAT_NAMES[KmerJoin::STATS] =
{
  "kmers_only_in_1", "kmers_only_in_2", "kmers_in_both", "occurrences_in_1_of_only_in_1", "occurrences_in_2_of_only_in_2", "occurrences_in_1_of_in_both",
  "occurrences_in_2_of_in_both"
};

static void printUsage()
{
  std::cerr << "Usage: bwt_kmer_compare [options] input1 input2 output" << std::endl << std::endl;
  std::cerr << "Options:" << std::endl;
  std::cerr << "  -g N           Use GPU N (default: 0)" << std::endl;
  std::cerr << "  -i format      Read the inputs in the given format (default: native)" << std::endl;
  std::cerr << "  -k N           Length of the k-mers, 1 to 32 (default: 21)" << std::endl;
  std::cerr << "  -a N           Keep the k-mers that occur at least N times in input1 (default: 0, may be absent)" << std::endl;
  std::cerr << "  -A N           Keep the k-mers that occur at most N times in input1 (default: no bound)" << std::endl;
  std::cerr << "  -b N           Keep the k-mers that occur at least N times in input2 (default: 0, may be absent)" << std::endl;
  std::cerr << "  -B N           Keep the k-mers that occur at most N times in input2 (default: no bound)" << std::endl;
  std::cerr << "  -s N           Keep the k-mers that occur at least N times in both inputs together (default: 1)" << std::endl;
  std::cerr << "  -S             Write the summary of the kept k-mers instead of the k-mers" << std::endl << std::endl;
  printFormats(std::cerr);
}

int main(int argc, char** argv)
{
  if(argc < 2) { printUsage(); std::exit(EXIT_SUCCESS); }

  std::cout << "BWT k-mer comparison" << std::endl << std::endl;

  int device = 0;
  std::string input_tag = NativeFormat::tag();
  size_type k = 21, min_a = 0, max_a = KmerJoin::NO_BOUND, min_b = 0, max_b = KmerJoin::NO_BOUND, min_sum = 1;
  bool summary = false;
  for(int c = 0; (c = getopt(argc, argv, "g:i:k:a:A:b:B:s:S")) != -1; )
  {
    switch(c)
    {
    case 'g': device = std::stoi(optarg); break;
    case 'i':
      input_tag = optarg;
      if(!formatExists(input_tag)) { std::cerr << "bwt_kmer_compare: Invalid input format: " << input_tag << std::endl; std::exit(EXIT_FAILURE); }
      break;
    case 'k': k = std::stoull(optarg); break;
    case 'a': min_a = std::stoull(optarg); break;
    case 'A': max_a = std::stoull(optarg); break;
    case 'b': min_b = std::stoull(optarg); break;
    case 'B': max_b = std::stoull(optarg); break;
    case 's': min_sum = std::stoull(optarg); break;
    case 'S': summary = true; break;
    default: std::exit(EXIT_FAILURE);
    }
  }
  if(optind + 2 >= argc) { std::cerr << "bwt_kmer_compare: Two input files and an output file must be specified" << std::endl; std::exit(EXIT_FAILURE); }
  if(k < 1 || k > 32) { std::cerr << "bwt_kmer_compare: The length of the k-mers must be 1 to 32" << std::endl; std::exit(EXIT_FAILURE); }
  if(min_a > max_a || min_b > max_b) { std::cerr << "bwt_kmer_compare: A minimum count (-a, -b) exceeds its maximum (-A, -B)" << std::endl; std::exit(EXIT_FAILURE); }
  std::string name_a = argv[optind], name_b = argv[optind + 1], output_name = argv[optind + 2];
  std::cout << "Input 1:  " << name_a << " (" << input_tag << ")" << std::endl;
  std::cout << "Input 2:  " << name_b << " (" << input_tag << ")" << std::endl;
  std::cout << "Output:   " << output_name << (summary ? " (name, value)" : " (k-mer, count 1, count 2)") << std::endl << std::endl;

  double start = readTimer();
  gpuCheck(bwtm_init(device), "bwt_kmer_compare");
  FMI a; load(a, name_a, input_tag);
  printSize("FMI 1", sizeInBytes(a), a.size());
  FMI b; load(b, name_b, input_tag);
  printSize("FMI 2", sizeInBytes(b), b.size());
  std::cout << std::endl;
  if(a.alpha != b.alpha) { std::cerr << "bwt_kmer_compare: The alphabets of " << name_a << " and " << name_b << " differ" << std::endl; std::exit(EXIT_FAILURE); }

  // N is the symbol that no k-mer holds: an alphabet without it leaves five symbols for a code of two bits each
  const size_type skip = a.alpha.char2comp[(byte_type)'N'];
  if(skip < 1 || skip >= a.alpha.sigma || a.alpha.comp2char[skip] != (byte_type)'N')
  {
    std::cerr << "bwt_kmer_compare: The alphabet of the inputs has no N: k-mers are strings over the four other symbols" << std::endl;
    std::exit(EXIT_FAILURE);
  }

  std::ofstream out(output_name.c_str(), std::ios_base::binary);
  if(!out) { std::cerr << "bwt_kmer_compare: Cannot open output file " << output_name << std::endl; std::exit(EXIT_FAILURE); }
  KmerJoin join(a, b, k, skip, min_a, max_a, min_b, max_b, min_sum);
  const size_type distinct = join.distinct();
  const std::vector<uint64_t> stats = join.summary();
  std::string lines;
  if(summary)
  {
    for(size_type s = 0; s < KmerJoin::STATS; s++) { lines += STAT_NAMES[s]; lines += '\t'; lines += std::to_string(stats[s]); lines += '\n'; }
    out.write(lines.data(), (std::streamsize)lines.size());
  }
  else
  {
    std::vector<uint64_t> codes, count_a, count_b;
    for(size_type done = 0; done < distinct; done += SLICE)
    {
      const size_type nb = std::min(SLICE, distinct - done);
      join.download(done, nb, codes, count_a, count_b);
      lines.clear();
      for(size_type e = 0; e < nb; e++)
      {
        for(size_type j = 0; j < k; j++) { lines += (char)a.alpha.comp2char[join.comp(codes[e], j)]; }
        lines += '\t'; lines += std::to_string(count_a[e]); lines += '\t'; lines += std::to_string(count_b[e]); lines += '\n';
      }
      out.write(lines.data(), (std::streamsize)lines.size());
    }
  }
  out.close();
  if(!out) { std::cerr << "bwt_kmer_compare: Writing to " << output_name << " failed" << std::endl; std::exit(EXIT_FAILURE); }
  double seconds = readTimer() - start;

  std::cout << "Kept " << distinct << " distinct " << k << "-mers: " << stats[0] << " only in input 1, " << stats[1] << " only in input 2, " << stats[2] << " in both" << std::endl << std::endl;
  std::cout << "K-mers compared in " << seconds << " seconds" << std::endl << std::endl;
  std::cout << "Memory usage: " << inGigabytes(memoryUsage()) << " GB" << std::endl << std::endl;
  return 0;
}
