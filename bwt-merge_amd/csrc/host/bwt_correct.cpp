/*
  bwt_correct -- writes the sequences of a BWT file as text, one per line like bwt_extract, after k-mer error correction: the step of a
  string-graph assembler between counting k-mers and computing overlaps.  The reference has no such tool.  The k-mers of the index are
  counted on the GPU (Kmers, bwtm_kmers_create with min_count = the threshold), the solid ones become a lookup table (Corrector,
  bwtm_corrector_create), and the reads are extracted and corrected on the device, a range of ids at a time (bwtm_correct_sequences): no
  k-mer and no uncorrected read comes to the host.  The output is what bwt_ingest reads: ingesting it gives the corrected index.
  The last line on stderr is "clean=<n> corrected=<n> failed=<n> short=<n> edits=<n> solid=<n>".
*/
#include <unistd.h>

#include "fmi.h"

using namespace bwtmerge;

size_type Parallel::max_threads = std::max(1u, std::thread::hardware_concurrency());

// ids per call of Corrector::sequences: the library's default batch (the correct_batch knob)
static const size_type ID_RANGE = (size_type)1 << 20;

static void printUsage()
{
  std::cerr << "Usage: bwt_correct [options] input output" << std::endl << std::endl;
  std::cerr << "Options:" << std::endl;
  std::cerr << "  -g N           Use GPU N (default: 0)" << std::endl;
  std::cerr << "  -i format      Read the input in the given format (default: native)" << std::endl;
  std::cerr << "  -k N           Length of the k-mers, 1 to 32 (default: 21)" << std::endl;
  std::cerr << "  -t N           A k-mer is solid when it occurs at least N times (default: 3)" << std::endl;
  std::cerr << "  -r N           Substitutions tried per read, one per round, at most 65535 (default: 10)" << std::endl;
  std::cerr << "  -f N           First sequence to write (default: 0)" << std::endl;
  std::cerr << "  -n N           Number of sequences to write (default: all from the first)" << std::endl;
  std::cerr << "  -m N           Longest sequence the input may hold (default: 65536, at most 16777216)" << std::endl;
  std::cerr << "  -x             Do not write the reads that could not be corrected" << std::endl << std::endl;
  printFormats(std::cerr);
}

int main(int argc, char** argv)
{
  if(argc < 2) { printUsage(); std::exit(EXIT_SUCCESS); }

  std::cout << "BWT correct" << std::endl << std::endl;

  int device = 0;
  std::string input_tag = NativeFormat::tag();
  size_type k = 21, threshold = 3, rounds = 10, first = 0, wanted = ~(size_type)0, max_len = 0;
  bool drop_failed = false;
  for(int c = 0; (c = getopt(argc, argv, "g:i:k:t:r:f:n:m:x")) != -1; )
  {
    switch(c)
    {
    case 'g': device = std::stoi(optarg); break;
    case 'i':
      input_tag = optarg;
      if(!formatExists(input_tag)) { std::cerr << "bwt_correct: Invalid input format: " << input_tag << std::endl; std::exit(EXIT_FAILURE); }
      break;
    case 'k': k = std::stoull(optarg); break;
    case 't': threshold = std::stoull(optarg); break;
    case 'r': rounds = std::stoull(optarg); break;
    case 'f': first = std::stoull(optarg); break;
    case 'n': wanted = std::stoull(optarg); break;
    case 'm': max_len = std::stoull(optarg); break;
    case 'x': drop_failed = true; break;
    default: std::exit(EXIT_FAILURE);
    }
  }
  if(optind + 1 >= argc) { std::cerr << "bwt_correct: Input and output files must be specified" << std::endl; std::exit(EXIT_FAILURE); }
  if(k < 1 || k > 32) { std::cerr << "bwt_correct: The length of the k-mers must be 1 to 32" << std::endl; std::exit(EXIT_FAILURE); }
  if(rounds > 65535) { std::cerr << "bwt_correct: At most 65535 rounds" << std::endl; std::exit(EXIT_FAILURE); }
  if(threshold == 0) { threshold = 1; }
  std::string input_name = argv[optind], output_name = argv[optind + 1];
  std::cout << "Input:   " << input_name << " (" << input_tag << ")" << std::endl;
  std::cout << "Output:  " << output_name << " (reads, one per line)" << std::endl;
  std::cout << "k = " << k << ", threshold = " << threshold << ", rounds = " << rounds << std::endl << std::endl;

  double start = readTimer();
  gpuCheck(bwtm_init(device), "bwt_correct");
  FMI fmi; load(fmi, input_name, input_tag);
  printSize("FMI", sizeInBytes(fmi), fmi.size());
  std::cout << std::endl;
  if(first > fmi.sequences()) { std::cerr << "bwt_correct: First sequence " << first << " out of range (" << fmi.sequences() << " sequences)" << std::endl; std::exit(EXIT_FAILURE); }
  const size_type count = std::min(wanted, fmi.sequences() - first);

  // N is the symbol that no k-mer holds (bwt_kmers)
  const size_type skip = fmi.alpha.char2comp[(byte_type)'N'];
  if(skip < 1 || skip >= fmi.alpha.sigma || fmi.alpha.comp2char[skip] != (byte_type)'N')
  {
    std::cerr << "bwt_correct: The alphabet of " << input_name << " has no N: k-mers are strings over the four other symbols" << std::endl;
    std::exit(EXIT_FAILURE);
  }

  std::ofstream out(output_name.c_str(), std::ios_base::binary);
  if(!out) { std::cerr << "bwt_correct: Cannot open output file " << output_name << std::endl; std::exit(EXIT_FAILURE); }
  size_type solid = 0;
  size_type by_status[4] = {0, 0, 0, 0}, total_edits = 0, symbols = 0, written = 0;
  {
    std::unique_ptr<Kmers> kmers(new Kmers(fmi, k, skip, threshold));         // the k-mers below the threshold are not needed
    Corrector corrector(*kmers, threshold);
    kmers.reset();                                                            // the corrector has copied what it needs
    solid = corrector.solid();
    std::vector<size_type> offsets; std::vector<byte_type> text, status; std::vector<uint32_t> edits;
    std::string lines;
    for(size_type done = 0; done < count; done += ID_RANGE)
    {
      const size_type n = std::min(ID_RANGE, count - done);
      corrector.sequences(fmi, range_type(first + done, first + done + n - 1), rounds, offsets, text, status, edits, max_len);
      lines.resize(text.size() + n);
      size_type at = 0;
      for(size_type j = 0; j < n; j++)
      {
        by_status[status[j] & 3]++; total_edits += edits[j];
        if(drop_failed && status[j] == BWTM_CORRECT_FAILED) { continue; }
        for(size_type p = offsets[j]; p < offsets[j + 1]; p++) { lines[at++] = (char)fmi.alpha.comp2char[text[p]]; }
        lines[at++] = '\n';
        written++; symbols += offsets[j + 1] - offsets[j];
      }
      out.write(lines.data(), (std::streamsize)at);
    }
  }
  out.close();
  if(!out) { std::cerr << "bwt_correct: Writing to " << output_name << " failed" << std::endl; std::exit(EXIT_FAILURE); }
  double seconds = readTimer() - start;

  std::cout << "Wrote " << written << " of " << count << " reads, total length " << symbols << std::endl << std::endl;
  std::cout << "Reads corrected in " << seconds << " seconds (" << (inMegabytes(symbols) / seconds) << " MB/s)" << std::endl << std::endl;
  std::cout << "Memory usage: " << inGigabytes(memoryUsage()) << " GB" << std::endl << std::endl;
  std::cout.flush();
  std::cerr << "clean=" << by_status[BWTM_CORRECT_CLEAN] << " corrected=" << by_status[BWTM_CORRECT_CORRECTED] << " failed=" << by_status[BWTM_CORRECT_FAILED]
            << " short=" << by_status[BWTM_CORRECT_SHORT] << " edits=" << total_edits << " solid=" << solid << std::endl;
  return 0;
}
