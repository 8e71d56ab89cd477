/*
  bwt_extract -- writes the sequences of a BWT file as text, one per line: the inverse of bwt_ingest's input format.  The reference has
  no such tool.  The sequences come back by LF walks on the GPU (FMI::sequences, bwtm_sequences_extract), a range of ids at a time, so
  the host holds the text of one range and the device the buffers of one batch, whatever the size of the collection.
  Sequence k of an index built by bwt_ingest, or merged from such indexes by bwt_merge, is read k of the input(s) in order.
*/
#include <unistd.h>

#include "fmi.h"

using namespace bwtmerge;

size_type Parallel::max_threads = std::max(1u, std::thread::hardware_concurrency());

// ids per call of FMI::sequences: the library's default batch (the extract_batch knob)
static const size_type ID_RANGE = (size_type)1 << 20;

static void printUsage()
{
  std::cerr << "Usage: bwt_extract [options] input output" << std::endl << std::endl;
  std::cerr << "Options:" << std::endl;
  std::cerr << "  -g N           Use GPU N (default: 0)" << std::endl;
  std::cerr << "  -i format      Read the input in the given format (default: native)" << std::endl;
  std::cerr << "  -f N           First sequence to write (default: 0)" << std::endl;
  std::cerr << "  -n N           Number of sequences to write (default: all from the first)" << std::endl;
  std::cerr << "  -m N           Longest sequence the input may hold (default: 65536, at most 16777216)" << std::endl << std::endl;
  printFormats(std::cerr);
}

int main(int argc, char** argv)
{
  if(argc < 2) { printUsage(); std::exit(EXIT_SUCCESS); }

  std::cout << "BWT extract" << std::endl << std::endl;

  int device = 0;
  std::string input_tag = NativeFormat::tag();
  size_type first = 0, wanted = ~(size_type)0, max_len = 0;
  for(int c = 0; (c = getopt(argc, argv, "g:i:f:n:m:")) != -1; )
  {
    switch(c)
    {
    case 'g': device = std::stoi(optarg); break;
    case 'i':
      input_tag = optarg;
      if(!formatExists(input_tag)) { std::cerr << "bwt_extract: Invalid input format: " << input_tag << std::endl; std::exit(EXIT_FAILURE); }
      break;
    case 'f': first = std::stoull(optarg); break;
    case 'n': wanted = std::stoull(optarg); break;
    case 'm': max_len = std::stoull(optarg); break;
    default: std::exit(EXIT_FAILURE);
    }
  }
  if(optind + 1 >= argc) { std::cerr << "bwt_extract: Output file not specified" << std::endl; std::exit(EXIT_FAILURE); }
  std::string input_name = argv[optind], output_name = argv[optind + 1];
  std::cout << "Input:   " << input_name << " (" << input_tag << ")" << std::endl;
  std::cout << "Output:  " << output_name << " (reads, one per line)" << std::endl << std::endl;

  double start = readTimer();
  gpuCheck(bwtm_init(device), "bwt_extract");
  FMI fmi; load(fmi, input_name, input_tag);
  printSize("FMI", sizeInBytes(fmi), fmi.size());
  std::cout << std::endl;
  if(first > fmi.sequences()) { std::cerr << "bwt_extract: First sequence " << first << " out of range (" << fmi.sequences() << " sequences)" << std::endl; std::exit(EXIT_FAILURE); }
  const size_type count = std::min(wanted, fmi.sequences() - first);

  std::ofstream out(output_name.c_str(), std::ios_base::binary);
  if(!out) { std::cerr << "bwt_extract: Cannot open output file " << output_name << std::endl; std::exit(EXIT_FAILURE); }
  std::vector<size_type> offsets; std::vector<byte_type> text;
  std::string lines;
  size_type symbols = 0;
  for(size_type done = 0; done < count; done += ID_RANGE)
  {
    const size_type n = std::min(ID_RANGE, count - done);
    fmi.sequences(range_type(first + done, first + done + n - 1), offsets, text, max_len);
    lines.resize(text.size() + n);
    size_type at = 0;
    for(size_type k = 0; k < n; k++)
    {
      for(size_type j = offsets[k]; j < offsets[k + 1]; j++) { lines[at++] = (char)fmi.alpha.comp2char[text[j]]; }
      lines[at++] = '\n';
    }
    out.write(lines.data(), (std::streamsize)lines.size());
    symbols += text.size();
  }
  out.close();
  if(!out) { std::cerr << "bwt_extract: Writing to " << output_name << " failed" << std::endl; std::exit(EXIT_FAILURE); }
  double seconds = readTimer() - start;

  std::cout << "Wrote " << count << " reads of total length " << symbols << std::endl << std::endl;
  std::cout << "Reads extracted in " << seconds << " seconds (" << (inMegabytes(symbols) / seconds) << " MB/s)" << std::endl << std::endl;
  std::cout << "Memory usage: " << inGigabytes(memoryUsage()) << " GB" << std::endl << std::endl;
  return 0;
}
