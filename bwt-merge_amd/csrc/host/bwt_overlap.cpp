/*
  bwt_overlap -- the suffix-prefix overlaps between the reads of a BWT file, the overlap step of a string-graph assembler: for every read,
  the reads whose prefix equals a suffix of it, at least min_overlap symbols long.  The reference has no such tool.  Every read is searched
  backwards on the GPU once, and the whole-sequence suffixes inside the ranges of that search become read numbers through the locator's
  table (Locator::overlaps, bwtm_overlap_sequences): no read and no BWT position comes to the host.  The output holds one line per hit,
      query <TAB> target <TAB> length        (all 0-based)
  in the order of the queries and, within a query, longest overlap first, then targets in BWT order (ascending as strings, a prefix before
  its extensions, equal reads by number): two runs compare with cmp.  A read contained as a suffix of the query is a hit (length = its own
  length), and so is the query itself over its whole length unless -s is given.  The reads are paged through in chunks, so neither the host
  nor the device ever holds the whole result.
  Sequence k of an index built by bwt_ingest, or merged from such indexes by bwt_merge, is read k of the input(s) in order.
*/
#include <unistd.h>

#include "fmi.h"

using namespace bwtmerge;

size_type Parallel::max_threads = std::max(1u, std::thread::hardware_concurrency());

// queries per call of Locator::overlaps: the library's default batch (the overlap_batch knob)
static const size_type CHUNK = size_type(1) << 20;

static void printUsage()
{
  std::cerr << "Usage: bwt_overlap [options] input output" << std::endl << std::endl;
  std::cerr << "Options:" << std::endl;
  std::cerr << "  -g N           Use GPU N (default: 0)" << std::endl;
  std::cerr << "  -i format      Read the input in the given format (default: native)" << std::endl;
  std::cerr << "  -t N           Shortest overlap to report, min_overlap (default: 30)" << std::endl;
  std::cerr << "  -x N           Write at most N hits per query: the longest overlaps (default: all)" << std::endl;
  std::cerr << "  -f N           First query sequence (default: 0)" << std::endl;
  std::cerr << "  -n N           Number of query sequences (default: up to the last one)" << std::endl;
  std::cerr << "  -m N           Longest sequence the input may hold (default: 65536, at most 16777216)" << std::endl;
  std::cerr << "  -s             Skip the hit of a query with itself over its whole length (applied after -x)" << std::endl << std::endl;
  printFormats(std::cerr);
}

int main(int argc, char** argv)
{
  if(argc < 2) { printUsage(); std::exit(EXIT_SUCCESS); }

  std::cout << "BWT overlap" << std::endl << std::endl;

  int device = 0;
  std::string input_tag = NativeFormat::tag();
  size_type min_overlap = 30, max_hits = 0, first = 0, count = ~size_type(0), max_len = 0;
  bool skip_self = false;
  for(int c = 0; (c = getopt(argc, argv, "g:i:t:x:f:n:m:s")) != -1; )
  {
    switch(c)
    {
    case 'g': device = std::stoi(optarg); break;
    case 'i':
      input_tag = optarg;
      if(!formatExists(input_tag)) { std::cerr << "bwt_overlap: Invalid input format: " << input_tag << std::endl; std::exit(EXIT_FAILURE); }
      break;
    case 't': min_overlap = std::stoull(optarg); break;
    case 'x': max_hits = std::stoull(optarg); break;
    case 'f': first = std::stoull(optarg); break;
    case 'n': count = std::stoull(optarg); break;
    case 'm': max_len = std::stoull(optarg); break;
    case 's': skip_self = true; break;
    default: std::exit(EXIT_FAILURE);
    }
  }
  if(optind + 1 >= argc) { std::cerr << "bwt_overlap: Input and output files must be specified" << std::endl; std::exit(EXIT_FAILURE); }
  if(min_overlap == 0) { std::cerr << "bwt_overlap: The shortest overlap must be at least 1" << std::endl; std::exit(EXIT_FAILURE); }
  std::string input_name = argv[optind], output_name = argv[optind + 1];
  std::cout << "Input:    " << input_name << " (" << input_tag << ")" << std::endl;
  std::cout << "Output:   " << output_name << " (query, target, length)" << std::endl << std::endl;

  double start = readTimer();
  gpuCheck(bwtm_init(device), "bwt_overlap");
  FMI fmi; load(fmi, input_name, input_tag);
  printSize("FMI", sizeInBytes(fmi), fmi.size());
  std::cout << std::endl;

  if(first > fmi.sequences()) { first = fmi.sequences(); }
  if(count > fmi.sequences() - first) { count = fmi.sequences() - first; }

  std::ofstream out(output_name.c_str(), std::ios_base::binary);
  if(!out) { std::cerr << "bwt_overlap: Cannot open output file " << output_name << std::endl; std::exit(EXIT_FAILURE); }
  size_type with_hits = 0, total = 0;
  if(count > 0)
  {
    Locator locator(fmi, max_len);
    std::vector<size_type> hit_offsets; std::vector<Locator::overlap_type> hits;
    std::string lines;
    for(size_type done = 0; done < count; done += CHUNK)
    {
      const size_type nb = std::min(CHUNK, count - done);
      locator.overlaps(range_type(first + done, first + done + nb - 1), min_overlap, hit_offsets, hits, max_hits);
      lines.clear();
      for(size_type k = 0; k < nb; k++)
      {
        const size_type query = first + done + k;
        size_type written = 0;
        for(size_type h = hit_offsets[k]; h < hit_offsets[k + 1]; h++)
        {
          // a query that has hits at all hits itself over its whole length, and no hit is longer: its first hit has that length
          if(skip_self && hits[h].first == query && hits[h].second == hits[hit_offsets[k]].second) { continue; }
          lines += std::to_string(query); lines += '\t'; lines += std::to_string(hits[h].first); lines += '\t'; lines += std::to_string(hits[h].second); lines += '\n';
          written++;
        }
        if(written > 0) { with_hits++; total += written; }
      }
      out.write(lines.data(), (std::streamsize)lines.size());
    }
  }
  out.close();
  if(!out) { std::cerr << "bwt_overlap: Writing to " << output_name << " failed" << std::endl; std::exit(EXIT_FAILURE); }
  double seconds = readTimer() - start;

  std::cout << "Searched " << count << " sequences: " << with_hits << " with overlaps, " << total << " hits" << std::endl << std::endl;
  std::cout << "Overlaps found in " << seconds << " seconds" << std::endl << std::endl;
  std::cout << "Memory usage: " << inGigabytes(memoryUsage()) << " GB" << std::endl << std::endl;
  return 0;
}
