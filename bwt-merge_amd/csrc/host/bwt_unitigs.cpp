/*
  bwt_unitigs -- writes the compacted de Bruijn graph of the reads of a BWT file as GFA 1: the step of an assembler behind counting and
  correcting.  The reference has no such tool.  The k-mers of the index are counted on the GPU (bwtm_kmers_create with min_count = the
  threshold), the unitigs over the solid ones, their coverage and the links between them are built there (bwtm_unitigs_create), and the
  result is downloaded a slice of unitigs at a time (bwtm_unitigs_download): no k-mer comes to the host.  All segments and links are on
  the plus strand (reverse complements are not looked at: an index that holds both strands gives them):
      H  VN:Z:1.0
      S  <unitig>  <text>  KC:i:<occurrences>  [TP:Z:circular]
      L  <unitig>  +  <unitig>  +  <k - 1>M
  The last line on stderr is "nodes=<n> unitigs=<n> circular=<n> links=<n> longest=<n>".
*/
#include <unistd.h>

#include "fmi.h"

using namespace bwtmerge;

size_type Parallel::max_threads = std::max(1u, std::thread::hardware_concurrency());

// unitigs per call of bwtm_unitigs_download
static const size_type SLICE = (size_type)1 << 20;

static void printUsage()
{
  std::cerr << "Usage: bwt_unitigs [options] input output" << std::endl << std::endl;
  std::cerr << "Options:" << std::endl;
  std::cerr << "  -g N           Use GPU N (default: 0)" << std::endl;
  std::cerr << "  -i format      Read the input in the given format (default: native)" << std::endl;
  std::cerr << "  -k N           Length of the k-mers, 1 to 32 (default: 21)" << std::endl;
  std::cerr << "  -t N           A k-mer is a node when it occurs at least N times (default: 3)" << std::endl << std::endl;
  printFormats(std::cerr);
}

int main(int argc, char** argv)
{
  if(argc < 2) { printUsage(); std::exit(EXIT_SUCCESS); }

  std::cout << "BWT unitigs" << std::endl << std::endl;

  int device = 0;
  std::string input_tag = NativeFormat::tag();
  size_type k = 21, threshold = 3;
  for(int c = 0; (c = getopt(argc, argv, "g:i:k:t:")) != -1; )
  {
    switch(c)
    {
    case 'g': device = std::stoi(optarg); break;
    case 'i':
      input_tag = optarg;
      if(!formatExists(input_tag)) { std::cerr << "bwt_unitigs: Invalid input format: " << input_tag << std::endl; std::exit(EXIT_FAILURE); }
      break;
    case 'k': k = std::stoull(optarg); break;
    case 't': threshold = std::stoull(optarg); break;
    default: std::exit(EXIT_FAILURE);
    }
  }
  if(optind + 1 >= argc) { std::cerr << "bwt_unitigs: Input and output files must be specified" << std::endl; std::exit(EXIT_FAILURE); }
  if(k < 1 || k > 32) { std::cerr << "bwt_unitigs: The length of the k-mers must be 1 to 32" << std::endl; std::exit(EXIT_FAILURE); }
  if(threshold == 0) { threshold = 1; }
  std::string input_name = argv[optind], output_name = argv[optind + 1];
  std::cout << "Input:   " << input_name << " (" << input_tag << ")" << std::endl;
  std::cout << "Output:  " << output_name << " (GFA 1)" << std::endl;
  std::cout << "k = " << k << ", threshold = " << threshold << std::endl << std::endl;

  double start = readTimer();
  gpuCheck(bwtm_init(device), "bwt_unitigs");
  FMI fmi; load(fmi, input_name, input_tag);
  printSize("FMI", sizeInBytes(fmi), fmi.size());
  std::cout << std::endl;

  // N is the symbol that no k-mer holds (bwt_kmers)
  const size_type skip = fmi.alpha.char2comp[(byte_type)'N'];
  if(skip < 1 || skip >= fmi.alpha.sigma || fmi.alpha.comp2char[skip] != (byte_type)'N')
  {
    std::cerr << "bwt_unitigs: The alphabet of " << input_name << " has no N: k-mers are strings over the four other symbols" << std::endl;
    std::exit(EXIT_FAILURE);
  }

  std::ofstream out(output_name.c_str(), std::ios_base::binary);
  if(!out) { std::cerr << "bwt_unitigs: Cannot open output file " << output_name << std::endl; std::exit(EXIT_FAILURE); }
  bwtm_unitigs* graph = nullptr;
  {
    std::unique_ptr<Kmers> kmers(new Kmers(fmi, k, skip, threshold));         // the k-mers below the threshold are not needed
    gpuCheck(bwtm_unitigs_create(kmers->device(), (uint32_t)skip, threshold, &graph), "bwt_unitigs");
  }                                                                           // the graph has copied what it needs
  const size_type unitigs = bwtm_unitigs_count(graph), nodes = bwtm_unitigs_nodes(graph);
  uint64_t stats[4] = {0, 0, 0, 0};
  gpuCheck(bwtm_unitigs_stats(stats), "bwt_unitigs");
  size_type circular = 0, link_count = 0, symbols = 0;
  out << "H\tVN:Z:1.0\n";
  std::vector<uint64_t> offsets, occurrences, links;
  std::vector<byte_type> text, flags;
  std::string lines;
  // the segments, then the links: two passes over the slices
  for(int pass = 0; pass < 2; pass++)
  {
    for(size_type done = 0; done < unitigs; done += SLICE)
    {
      const size_type n = std::min(SLICE, unitigs - done);
      lines.clear();
      if(pass == 0)
      {
        offsets.assign(n + 1, 0); occurrences.assign(n, 0); flags.assign(n, 0);
        gpuCheck(bwtm_unitigs_download(graph, done, n, offsets.data(), nullptr, 0, nullptr, nullptr, nullptr, nullptr), "bwt_unitigs");       // the size
        text.assign(offsets[n], 0);
        gpuCheck(bwtm_unitigs_download(graph, done, n, offsets.data(), text.data(), text.size(), nullptr, occurrences.data(), flags.data(), nullptr), "bwt_unitigs");
        for(size_type j = 0; j < n; j++)
        {
          lines += "S\t"; lines += std::to_string(done + j); lines += '\t';
          for(size_type p = offsets[j]; p < offsets[j + 1]; p++) { lines += (char)fmi.alpha.comp2char[text[p]]; }
          lines += "\tKC:i:"; lines += std::to_string(occurrences[j]);
          if(flags[j] & BWTM_UNITIG_CIRCULAR) { lines += "\tTP:Z:circular"; circular++; }
          lines += '\n';
        }
        symbols += offsets[n];
      }
      else
      {
        links.assign(4 * n, 0);
        gpuCheck(bwtm_unitigs_download(graph, done, n, nullptr, nullptr, 0, nullptr, nullptr, nullptr, links.data()), "bwt_unitigs");
        for(size_type j = 0; j < n; j++)
        {
          for(size_type r = 0; r < 4; r++)
          {
            if(links[4 * j + r] == ~(uint64_t)0) { continue; }
            lines += "L\t"; lines += std::to_string(done + j); lines += "\t+\t"; lines += std::to_string(links[4 * j + r]);
            lines += "\t+\t"; lines += std::to_string(k - 1); lines += "M\n";
            link_count++;
          }
        }
      }
      out.write(lines.data(), (std::streamsize)lines.size());
    }
  }
  bwtm_unitigs_free(graph);
  out.close();
  if(!out) { std::cerr << "bwt_unitigs: Writing to " << output_name << " failed" << std::endl; std::exit(EXIT_FAILURE); }
  double seconds = readTimer() - start;

  std::cout << "Wrote " << unitigs << " unitigs of " << nodes << " k-mers, total length " << symbols << std::endl << std::endl;
  std::cout << "Graph built in " << seconds << " seconds" << std::endl << std::endl;
  std::cout << "Memory usage: " << inGigabytes(memoryUsage()) << " GB" << std::endl << std::endl;
  std::cout.flush();
  std::cerr << "nodes=" << nodes << " unitigs=" << unitigs << " circular=" << circular << " links=" << link_count << " longest=" << stats[1] << std::endl;
  return 0;
}
