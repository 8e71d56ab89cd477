/*
  bwt_locate -- the occurrences of patterns in the reads of a BWT file: for every pattern, the sequences that contain it and the offsets
  at which it starts.  The reference has no such tool.  The backward searches run on the GPU in one batch (bwtm_find_batch), and the
  positions of every range become (sequence, offset) by LF walks on the GPU (Locator, bwtm_locate_ranges).  Patterns are read, one per
  line, and mapped exactly as `bwt_merge -v` reads them.  The output holds one line per hit,
      pattern_number <TAB> sequence <TAB> offset        (all 0-based)
  in the order of the patterns and, within a pattern, sorted by (sequence, offset): two runs compare with cmp.
  With -d N the search allows up to N substitutions (bwtm_find_approx_batch: no reverse complements) and every line gains a
  fourth column, the number of places in which the occurrence differs from the pattern; -x then bounds the occurrences written per
  matched string.  With -e N it allows up to N insertions, deletions and substitutions (bwtm_find_edit_batch) and every line gains
  two columns, the edit distance of the occurrence from the pattern and its length.  With -M N the pattern is not searched as a whole:
  its maximal exact matches of at least N symbols are (bwtm_mem_batch: the substrings of the pattern that occur and lie in no longer
  one that occurs), every one located, and every line is
      pattern_number <TAB> sequence <TAB> offset <TAB> begin <TAB> length
  with the match pattern[begin .. begin + length) at `offset` of `sequence`; -x then bounds the occurrences written per match.  The
  lines of a pattern are sorted by (begin, sequence, offset).  Without -d, -e and -M the output is what it always was.
  Sequence k of an index built by bwt_ingest, or merged from such indexes by bwt_merge, is read k of the input(s) in order.
*/
#include <unistd.h>

#include "fmi.h"

using namespace bwtmerge;

size_type Parallel::max_threads = std::max(1u, std::thread::hardware_concurrency());

static void printUsage()
{
  std::cerr << "Usage: bwt_locate [options] input patterns output" << std::endl << std::endl;
  std::cerr << "Options:" << std::endl;
  std::cerr << "  -g N           Use GPU N (default: 0)" << std::endl;
  std::cerr << "  -i format      Read the input in the given format (default: native)" << std::endl;
  std::cerr << "  -m N           Longest sequence the input may hold (default: 65536, at most 16777216)" << std::endl;
  std::cerr << "  -x N           Write at most N hits per pattern: the first N positions of its range (default: all)" << std::endl;
  std::cerr << "  -d N           Allow up to N substitutions, 0 to 8, and write the mismatches of every hit as a fourth column;" << std::endl;
  std::cerr << "                 -x then applies to every matched string (default: exact search, three columns)" << std::endl;
  std::cerr << "  -e N           Allow up to N edits (insertions, deletions, substitutions), 0 to 7, and write the edit distance and the" << std::endl;
  std::cerr << "                 length of every hit as a fourth and fifth column; -x as with -d; not together with -d" << std::endl;
  std::cerr << "  -M N           Locate the maximal exact matches of at least N symbols (N >= 1) of every pattern and write the begin and the" << std::endl;
  std::cerr << "                 length of the match as a fourth and fifth column; -x then applies to every match; not together with -d or -e" << std::endl << std::endl;
  printFormats(std::cerr);
}

// One pattern per line, empty lines skipped (readRows of bwt_merge.cpp).
static size_type readRows(const std::string& filename, std::vector<std::string>& rows)
{
  std::ifstream in(filename.c_str(), std::ios_base::binary);
  if(!in) { std::cerr << "bwt_locate: Cannot open pattern file " << filename << std::endl; std::exit(EXIT_FAILURE); }
  size_type chars = 0;
  for(std::string line; std::getline(in, line); ) { if(!line.empty()) { rows.push_back(line); chars += line.length(); } }
  return chars;
}

int main(int argc, char** argv)
{
  if(argc < 2) { printUsage(); std::exit(EXIT_SUCCESS); }

  std::cout << "BWT locate" << std::endl << std::endl;

  int device = 0;
  std::string input_tag = NativeFormat::tag();
  size_type max_len = 0, max_hits = 0, mismatches = 0, edits = 0, min_length = 0;
  bool approx = false, edit = false, mem = false;
  for(int c = 0; (c = getopt(argc, argv, "g:i:m:x:d:e:M:")) != -1; )
  {
    switch(c)
    {
    case 'g': device = std::stoi(optarg); break;
    case 'i':
      input_tag = optarg;
      if(!formatExists(input_tag)) { std::cerr << "bwt_locate: Invalid input format: " << input_tag << std::endl; std::exit(EXIT_FAILURE); }
      break;
    case 'm': max_len = std::stoull(optarg); break;
    case 'x': max_hits = std::stoull(optarg); break;
    case 'd':
      approx = true; mismatches = std::stoull(optarg);
      if(mismatches > 8) { std::cerr << "bwt_locate: -d takes 0 to 8 mismatches" << std::endl; std::exit(EXIT_FAILURE); }
      break;
    case 'e':
      edit = true; edits = std::stoull(optarg);
      if(edits > 7) { std::cerr << "bwt_locate: -e takes 0 to 7 edits" << std::endl; std::exit(EXIT_FAILURE); }
      break;
    case 'M':
      mem = true; min_length = std::stoull(optarg);
      if(min_length < 1) { std::cerr << "bwt_locate: -M takes a length of at least 1" << std::endl; std::exit(EXIT_FAILURE); }
      break;
    default: std::exit(EXIT_FAILURE);
    }
  }
  if(mem && (approx || edit)) { std::cerr << "bwt_locate: -M cannot be used together with -d or -e" << std::endl; std::exit(EXIT_FAILURE); }
  if(approx && edit) { std::cerr << "bwt_locate: -d and -e cannot be used together" << std::endl; std::exit(EXIT_FAILURE); }
  if(optind + 2 >= argc) { std::cerr << "bwt_locate: Input, pattern and output files must be specified" << std::endl; std::exit(EXIT_FAILURE); }
  std::string input_name = argv[optind], pattern_name = argv[optind + 1], output_name = argv[optind + 2];
  std::cout << "Input:    " << input_name << " (" << input_tag << ")" << std::endl;
  std::cout << "Patterns: " << pattern_name << std::endl;
  std::cout << "Output:   " << output_name << (mem ? " (pattern, sequence, offset, begin, length)" : edit ? " (pattern, sequence, offset, edits, length)" : approx ? " (pattern, sequence, offset, mismatches)" : " (pattern, sequence, offset)") << std::endl;
  if(approx) { std::cout << "Search:   up to " << mismatches << " substitutions" << std::endl; }
  if(edit) { std::cout << "Search:   up to " << edits << " edits" << std::endl; }
  if(mem) { std::cout << "Search:   maximal exact matches of at least " << min_length << " symbols" << std::endl; }
  std::cout << std::endl;

  double start = readTimer();
  gpuCheck(bwtm_init(device), "bwt_locate");
  std::vector<std::string> patterns;
  const size_type chars = readRows(pattern_name, patterns);
  FMI fmi; load(fmi, input_name, input_tag);
  printSize("FMI", sizeInBytes(fmi), fmi.size());
  std::cout << std::endl;

  std::ofstream out(output_name.c_str(), std::ios_base::binary);
  if(!out) { std::cerr << "bwt_locate: Cannot open output file " << output_name << std::endl; std::exit(EXIT_FAILURE); }
  size_type found = 0, total = 0;
  if(!patterns.empty())
  {
    std::vector<byte_type> text; text.reserve(chars);
    std::vector<uint64_t> offsets(patterns.size() + 1, 0), sp(patterns.size()), ep(patterns.size());
    for(size_type k = 0; k < patterns.size(); k++)
    {
      for(char ch : patterns[k]) { text.push_back(fmi.alpha.char2comp[(byte_type)ch]); }
      offsets[k + 1] = text.size();
    }
    if(approx)
    {
      // every matched string of a pattern is a range of its own: located like the others, its mismatches written with every occurrence
      std::vector<size_type> string_offsets; std::vector<FMI::ApproxHit> strings;
      fmi.findApprox(text, offsets, mismatches, string_offsets, strings);
      std::vector<range_type> ranges(strings.size());
      for(size_type s = 0; s < strings.size(); s++) { ranges[s] = strings[s].range; }
      Locator locator(fmi, max_len);
      std::vector<size_type> hit_offsets; std::vector<Locator::hit_type> hits;
      locator.locate(ranges, hit_offsets, hits, max_hits);
      total = hits.size();
      std::vector<std::pair<Locator::hit_type, size_type>> rows;
      std::string lines;
      for(size_type k = 0; k < patterns.size(); k++)
      {
        rows.clear();
        for(size_type s = string_offsets[k]; s < string_offsets[k + 1]; s++)
        {
          for(size_type h = hit_offsets[s]; h < hit_offsets[s + 1]; h++) { rows.push_back(std::make_pair(hits[h], strings[s].mismatches)); }
        }
        if(rows.empty()) { continue; }
        found++;
        std::sort(rows.begin(), rows.end());
        lines.clear();
        for(const auto& row : rows)
        {
          lines += std::to_string(k); lines += '\t'; lines += std::to_string(row.first.first); lines += '\t'; lines += std::to_string(row.first.second); lines += '\t';
          lines += std::to_string(row.second); lines += '\n';
        }
        out.write(lines.data(), (std::streamsize)lines.size());
      }
    }
    else if(edit)
    {
      // as with -d: every matched string is a range of its own, its distance and length written with every occurrence
      std::vector<size_type> string_offsets; std::vector<FMI::EditHit> strings;
      fmi.findEdit(text, offsets, edits, string_offsets, strings);
      std::vector<range_type> ranges(strings.size());
      for(size_type s = 0; s < strings.size(); s++) { ranges[s] = strings[s].range; }
      Locator locator(fmi, max_len);
      std::vector<size_type> hit_offsets; std::vector<Locator::hit_type> hits;
      locator.locate(ranges, hit_offsets, hits, max_hits);
      total = hits.size();
      std::vector<std::pair<Locator::hit_type, std::pair<size_type, size_type>>> rows;
      std::string lines;
      for(size_type k = 0; k < patterns.size(); k++)
      {
        rows.clear();
        for(size_type s = string_offsets[k]; s < string_offsets[k + 1]; s++)
        {
          for(size_type h = hit_offsets[s]; h < hit_offsets[s + 1]; h++) { rows.push_back(std::make_pair(hits[h], std::make_pair(strings[s].edits, strings[s].length))); }
        }
        if(rows.empty()) { continue; }
        found++;
        std::sort(rows.begin(), rows.end());
        lines.clear();
        for(const auto& row : rows)
        {
          lines += std::to_string(k); lines += '\t'; lines += std::to_string(row.first.first); lines += '\t'; lines += std::to_string(row.first.second); lines += '\t';
          lines += std::to_string(row.second.first); lines += '\t'; lines += std::to_string(row.second.second); lines += '\n';
        }
        out.write(lines.data(), (std::streamsize)lines.size());
      }
    }
    else if(mem)
    {
      // every maximal exact match of a pattern is a range of its own: located like the others, its begin and length written with every occurrence
      std::vector<size_type> mem_offsets; std::vector<FMI::MEM> mems;
      fmi.mems(text, offsets, min_length, mem_offsets, mems);
      std::vector<range_type> ranges(mems.size());
      for(size_type s = 0; s < mems.size(); s++) { ranges[s] = mems[s].range; }
      Locator locator(fmi, max_len);
      std::vector<size_type> hit_offsets; std::vector<Locator::hit_type> hits;
      locator.locate(ranges, hit_offsets, hits, max_hits);
      total = hits.size();
      std::string lines;
      for(size_type k = 0; k < patterns.size(); k++)
      {
        if(mem_offsets[k + 1] == mem_offsets[k]) { continue; }
        found++;
        lines.clear();
        for(size_type s = mem_offsets[k]; s < mem_offsets[k + 1]; s++)                          // begins ascending
        {
          std::sort(hits.begin() + hit_offsets[s], hits.begin() + hit_offsets[s + 1]);
          for(size_type h = hit_offsets[s]; h < hit_offsets[s + 1]; h++)
          {
            lines += std::to_string(k); lines += '\t'; lines += std::to_string(hits[h].first); lines += '\t'; lines += std::to_string(hits[h].second); lines += '\t';
            lines += std::to_string(mems[s].begin); lines += '\t'; lines += std::to_string(mems[s].length); lines += '\n';
          }
        }
        out.write(lines.data(), (std::streamsize)lines.size());
      }
    }
    else
    {
      bwtm_index* ix = fmi.bwt.onDevice(fmi.alpha.C);
      gpuCheck(bwtm_find_batch(ix, text.data(), offsets.data(), patterns.size(), sp.data(), ep.data()), "bwt_locate");
      std::vector<range_type> ranges(patterns.size());
      for(size_type k = 0; k < patterns.size(); k++) { ranges[k] = range_type(sp[k], ep[k]); }

      Locator locator(fmi, max_len);
      std::vector<size_type> hit_offsets; std::vector<Locator::hit_type> hits;
      locator.locate(ranges, hit_offsets, hits, max_hits);
      total = hits.size();
      std::string lines;
      for(size_type k = 0; k < patterns.size(); k++)
      {
        if(hit_offsets[k + 1] == hit_offsets[k]) { continue; }
        found++;
        std::sort(hits.begin() + hit_offsets[k], hits.begin() + hit_offsets[k + 1]);
        lines.clear();
        for(size_type h = hit_offsets[k]; h < hit_offsets[k + 1]; h++)
        {
          lines += std::to_string(k); lines += '\t'; lines += std::to_string(hits[h].first); lines += '\t'; lines += std::to_string(hits[h].second); lines += '\n';
        }
        out.write(lines.data(), (std::streamsize)lines.size());
      }
    }
  }
  out.close();
  if(!out) { std::cerr << "bwt_locate: Writing to " << output_name << " failed" << std::endl; std::exit(EXIT_FAILURE); }
  double seconds = readTimer() - start;

  std::cout << "Located " << patterns.size() << " patterns: " << found << " found, " << total << " hits" << std::endl << std::endl;
  std::cout << "Patterns located in " << seconds << " seconds" << std::endl << std::endl;
  std::cout << "Memory usage: " << inGigabytes(memoryUsage()) << " GB" << std::endl << std::endl;
  return 0;
}
