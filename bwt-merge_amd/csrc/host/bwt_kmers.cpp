/*
  bwt_kmers -- the distinct k-mers of the reads of a BWT file with their counts, or the spectrum of those counts: what an assembler or a QC
  step asks of a read collection before anything else (coverage peak, genome size, the solid / weak threshold of error correction).  The
  reference has no such tool.  The suffix trie of the index is expanded down to depth k on the GPU (Kmers, bwtm_kmers_create): no read comes
  to the host, and no k-mer is searched on its own.  A k-mer is a string of k characters other than N that occurs inside a read.
  Without -H the output holds one line per kept k-mer,
      kmer <TAB> count
  in ascending order of the k-mers (the order of the file's alphabet); with -H one line per non-empty bin of the spectrum,
      count <TAB> k-mers of that count        (the last bin, bins - 1, collects every larger count)
  The list is written in slices, so the host never holds the whole of it.
*/
#include <unistd.h>

#include "fmi.h"

using namespace bwtmerge;

size_type Parallel::max_threads = std::max(1u, std::thread::hardware_concurrency());

// entries per download
static const size_type SLICE = size_type(1) << 22;

static void printUsage()
{
  std::cerr << "Usage: bwt_kmers [options] input output" << std::endl << std::endl;
  std::cerr << "Options:" << std::endl;
  std::cerr << "  -g N           Use GPU N (default: 0)" << std::endl;
  std::cerr << "  -i format      Read the input in the given format (default: native)" << std::endl;
  std::cerr << "  -k N           Length of the k-mers, 1 to 32 (default: 21)" << std::endl;
  std::cerr << "  -c N           Keep the k-mers that occur at least N times, min_count (default: 1)" << std::endl;
  std::cerr << "  -H N           Write the spectrum in N bins instead of the k-mers (at least 2)" << std::endl << std::endl;
  printFormats(std::cerr);
}

int main(int argc, char** argv)
{
  if(argc < 2) { printUsage(); std::exit(EXIT_SUCCESS); }

  std::cout << "BWT k-mers" << std::endl << std::endl;

  int device = 0;
  std::string input_tag = NativeFormat::tag();
  size_type k = 21, min_count = 1, bins = 0;
  bool spectrum = false;
  for(int c = 0; (c = getopt(argc, argv, "g:i:k:c:H:")) != -1; )
  {
    switch(c)
    {
    case 'g': device = std::stoi(optarg); break;
    case 'i':
      input_tag = optarg;
      if(!formatExists(input_tag)) { std::cerr << "bwt_kmers: Invalid input format: " << input_tag << std::endl; std::exit(EXIT_FAILURE); }
      break;
    case 'k': k = std::stoull(optarg); break;
    case 'c': min_count = std::stoull(optarg); break;
    case 'H': bins = std::stoull(optarg); spectrum = true; break;
    default: std::exit(EXIT_FAILURE);
    }
  }
  if(optind + 1 >= argc) { std::cerr << "bwt_kmers: Input and output files must be specified" << std::endl; std::exit(EXIT_FAILURE); }
  if(k < 1 || k > 32) { std::cerr << "bwt_kmers: The length of the k-mers must be 1 to 32" << std::endl; std::exit(EXIT_FAILURE); }
  if(spectrum && bins < 2) { std::cerr << "bwt_kmers: The spectrum needs at least 2 bins" << std::endl; std::exit(EXIT_FAILURE); }
  std::string input_name = argv[optind], output_name = argv[optind + 1];
  std::cout << "Input:    " << input_name << " (" << input_tag << ")" << std::endl;
  std::cout << "Output:   " << output_name << (spectrum ? " (count, k-mers)" : " (k-mer, count)") << std::endl << std::endl;

  double start = readTimer();
  gpuCheck(bwtm_init(device), "bwt_kmers");
  FMI fmi; load(fmi, input_name, input_tag);
  printSize("FMI", sizeInBytes(fmi), fmi.size());
  std::cout << std::endl;

  // N is the symbol that no k-mer holds: an alphabet without it leaves five symbols for a code of two bits each
  const size_type skip = fmi.alpha.char2comp[(byte_type)'N'];
  if(skip < 1 || skip >= fmi.alpha.sigma || fmi.alpha.comp2char[skip] != (byte_type)'N')
  {
    std::cerr << "bwt_kmers: The alphabet of " << input_name << " has no N: k-mers are strings over the four other symbols" << std::endl;
    std::exit(EXIT_FAILURE);
  }

  std::ofstream out(output_name.c_str(), std::ios_base::binary);
  if(!out) { std::cerr << "bwt_kmers: Cannot open output file " << output_name << std::endl; std::exit(EXIT_FAILURE); }
  Kmers kmers(fmi, k, skip, min_count);
  const size_type distinct = kmers.distinct();
  std::string lines;
  if(spectrum)
  {
    const std::vector<uint64_t> hist = kmers.histogram(bins);
    for(size_type j = 0; j < bins; j++)
    {
      if(hist[j] > 0) { lines += std::to_string(j); lines += '\t'; lines += std::to_string(hist[j]); lines += '\n'; }
    }
    out.write(lines.data(), (std::streamsize)lines.size());
  }
  else
  {
    std::vector<uint64_t> codes, counts;
    for(size_type done = 0; done < distinct; done += SLICE)
    {
      const size_type nb = std::min(SLICE, distinct - done);
      kmers.download(done, nb, codes, counts);
      lines.clear();
      for(size_type e = 0; e < nb; e++)
      {
        for(size_type j = 0; j < k; j++) { lines += (char)fmi.alpha.comp2char[kmers.comp(codes[e], j)]; }
        lines += '\t'; lines += std::to_string(counts[e]); lines += '\n';
      }
      out.write(lines.data(), (std::streamsize)lines.size());
    }
  }
  out.close();
  if(!out) { std::cerr << "bwt_kmers: Writing to " << output_name << " failed" << std::endl; std::exit(EXIT_FAILURE); }
  double seconds = readTimer() - start;

  std::cout << "Found " << distinct << " distinct " << k << "-mers of count " << std::max<size_type>(min_count, 1) << " or more, " << kmers.total() << " occurrences" << std::endl << std::endl;
  std::cout << "K-mers enumerated in " << seconds << " seconds" << std::endl << std::endl;
  std::cout << "Memory usage: " << inGigabytes(memoryUsage()) << " GB" << std::endl << std::endl;
  return 0;
}
