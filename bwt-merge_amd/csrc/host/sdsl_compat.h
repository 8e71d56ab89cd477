/*
  sdsl_compat.h -- the few SDSL container encodings the native file format embeds
  (int_vector<8/64/1/0>, sd_vector<> with its two select_support_mcl members), written from the
  published description of sdsl-lite.

  UNVERIFIED AGAINST REAL SDSL OUTPUT: sdsl-lite is not available in this environment, so files
  written here round-trip through this reader (tests) but byte compatibility with SDSL-built
  files is unpinned.  Only serialization is provided; queries use plain arrays (bwt.h).
  The payload the hot path computes (header, BWT::data, the sample VALUES, C) is pinned against the
  oracle; what is unpinned is the bit layout of sd_vector / select_support_mcl around those values.
  The select supports follow sdsl-lite's two construction paths as recalled: vectors below 100 000
  bits take init_slow (every superblock, the last partial one included, is long or mini by its span),
  larger ones init_fast (the last partial superblock is always stored long, with the width of the
  vector's last position, and its entry in the superblock array is left 0).
*/
#ifndef BWTM_HOST_SDSL_COMPAT_H
#define BWTM_HOST_SDSL_COMPAT_H

#include <istream>
#include <ostream>
#include <sstream>
#include "utils.h"

namespace bwtmerge
{

/*
  An input file as the loaders read it.  The stream's length is measured once, every read is checked against what is left and against
  what arrived, and a file that cannot be what it claims to be is refused the way the "Invalid header!" paths refuse: one line on
  std::cerr -- LOADER: FILE: what is wrong -- and exit(EXIT_FAILURE).  Nothing a file states (a size, a width, a count) sizes an
  allocation before it has been compared with remaining().
*/
class Source
{
public:
  Source(std::istream& stream, const std::string& file, const std::string& loader) : in(stream), name(file), where(loader), left(0)
  {
    in.seekg(0, std::ios_base::end);
    const std::streamoff end = in.tellg();
    in.seekg(0, std::ios_base::beg);
    if(!in || end < 0) { refuse("cannot determine the size of the input (not a regular file?)"); }
    left = (size_type)end;
  }

  [[noreturn]] void refuse(const std::string& what) const
  {
    std::cerr << where << ": " << name << ": " << what << std::endl;
    std::exit(EXIT_FAILURE);
  }
  [[noreturn]] void truncated(const char* what, size_type wanted) const
  {
    std::ostringstream msg; msg << "truncated in " << what << " (" << wanted << " bytes wanted, " << left << " left)";
    refuse(msg.str());
  }

  size_type remaining() const { return left; }

  void read(void* to, size_type n, const char* what)
  {
    if(n > left) { truncated(what, n); }
    if(n == 0) { return; }
    in.read((char*)to, (std::streamsize)n);
    if(!in || (size_type)in.gcount() != n) { truncated(what, n); }
    left -= n;
  }
  // At most n bytes; the number that arrived (the byte-per-item formats read in chunks).
  size_type readSome(void* to, size_type n)
  {
    n = std::min(n, left);
    if(n == 0) { return 0; }
    in.read((char*)to, (std::streamsize)n);
    const size_type got = (size_type)in.gcount();
    left -= got;
    return got;
  }
  void skip(size_type n, const char* what)
  {
    if(n > left) { truncated(what, n); }
    if(n == 0) { return; }
    in.seekg((std::streamoff)n, std::ios_base::cur);
    if(!in) { truncated(what, n); }
    left -= n;
  }
  template<class T> T get(const char* what) { T v = T(); read(&v, sizeof(T), what); return v; }

  std::istream& in;
  const std::string name, where;

private:
  size_type left;
};

namespace sdsl_compat
{

inline size_type hi(size_type x) { return (x == 0 ? 0 : 63 - (size_type)__builtin_clzll(x)); }   // sdsl::bits::hi

template<class T> void write_member(const T& v, std::ostream& out) { out.write((const char*)&v, sizeof(T)); }
template<class T> void read_member(T& v, std::istream& in) { in.read((char*)&v, sizeof(T)); }

// Bit-packed vector of fixed-width integers (int_vector<0> when `dynamic_width`).
struct PackedVector
{
  size_type width = 64, count = 0;
  std::vector<std::uint64_t> words;

  PackedVector() {}
  PackedVector(size_type n, size_type w) : width(w == 0 ? 1 : w), count(n), words((n * (w == 0 ? 1 : w) + 63) / 64 + 1, 0) {}

  void set(size_type i, size_type v)
  {
    size_type bit = i * width, word = bit / 64, off = bit % 64;
    if(width < 64) { v &= ((size_type)1 << width) - 1; }
    words[word] |= v << off;
    if(off + width > 64) { words[word + 1] |= v >> (64 - off); }
  }
  size_type get(size_type i) const
  {
    size_type bit = i * width, word = bit / 64, off = bit % 64;
    size_type v = words[word] >> off;
    if(off + width > 64) { v |= words[word + 1] << (64 - off); }
    if(width < 64) { v &= ((size_type)1 << width) - 1; }
    return v;
  }
  size_type bit_size() const { return count * width; }

  // int_vector<w>::serialize: u64 size in bits, [u8 width when dynamic], ceil(bits / 64) words.
  void serialize(std::ostream& out, bool dynamic_width) const
  {
    size_type bits = bit_size();
    write_member(bits, out);
    if(dynamic_width) { std::uint8_t w = (std::uint8_t)width; write_member(w, out); }
    out.write((const char*)words.data(), ((bits + 63) / 64) * 8);
  }

  // The size fields of a serialized vector, checked: the width is 1 to 64, the bits are whole entries, the words are in the file.
  struct Frame { size_type bits, width, count, bytes; };
  static Frame frame(Source& in, bool dynamic_width, size_type fixed_width, const char* what)
  {
    Frame f;
    f.bits = in.get<size_type>(what);
    f.width = fixed_width;
    if(dynamic_width) { f.width = in.get<std::uint8_t>(what); }
    if(f.width == 0 || f.width > 64) { refuse(in, what, "has a width of", f.width, "bits"); }
    if(f.bits % f.width != 0) { refuse(in, what, "is not a whole number of entries:", f.bits, "bits"); }
    f.count = f.bits / f.width;
    f.bytes = (f.bits / 64 + (f.bits % 64 != 0 ? 1 : 0)) * 8;
    if(f.bytes > in.remaining()) { in.truncated(what, f.bytes); }
    return f;
  }
  [[noreturn]] static void refuse(const Source& in, const char* what, const char* problem, size_type value, const char* unit)
  {
    std::ostringstream msg; msg << what << " " << problem << " " << value << " " << unit;
    in.refuse(msg.str());
  }

  void load(Source& in, bool dynamic_width, size_type fixed_width, const char* what)
  {
    const Frame f = frame(in, dynamic_width, fixed_width, what);
    width = f.width; count = f.count;
    words.assign(f.bytes / 8 + 1, 0);
    in.read(words.data(), f.bytes, what);
  }
  // The same checks without keeping the entries; the number of entries.
  static size_type skip(Source& in, bool dynamic_width, size_type fixed_width, const char* what)
  {
    const Frame f = frame(in, dynamic_width, fixed_width, what);
    in.skip(f.bytes, what);
    return f.count;
  }
};

// select_support_mcl<b, 1> over a bit vector: serialization only.
struct SelectMCL
{
  static void serialize(std::ostream& out, const PackedVector& bits, bool select_ones)
  {
    const size_type SUPER = 4096;
    size_type n = bits.bit_size();
    // positions of the selected bits, word by word (width-1 vector: bit i of the vector is bit i % 64 of word i / 64)
    std::vector<size_type> args;
    for(size_type w = 0; w * 64 < n; w++)
    {
      std::uint64_t word = (select_ones ? bits.words[w] : ~bits.words[w]);
      if((w + 1) * 64 > n) { word &= (~(std::uint64_t)0) >> (64 - (n - w * 64)); }
      while(word != 0) { args.push_back(w * 64 + (size_type)__builtin_ctzll(word)); word &= word - 1; }
    }
    size_type arg_cnt = args.size();
    write_member(arg_cnt, out);
    if(arg_cnt == 0) { return; }
    size_type capacity = ((n + 63) / 64) * 64;
    size_type logn = hi(capacity) + 1, logn4 = logn * logn * logn * logn;
    size_type sb = (arg_cnt + SUPER - 1) / SUPER;
    const bool fast = (n >= 100000);                                   // select_support_mcl's constructor: init_slow below, init_fast from there on
    const bool tail_long = (fast && arg_cnt % SUPER != 0);             // init_fast: "handle last block: append long superblock"
    PackedVector superblock(sb, logn);
    std::vector<bool> is_long(sb, false);
    bool any_long = false;
    for(size_type s = 0; s < sb; s++)
    {
      size_type first = args[s * SUPER], last = args[std::min(arg_cnt, (s + 1) * SUPER) - 1];
      if(tail_long && s + 1 == sb) { is_long[s] = true; any_long = true; continue; }   // its superblock entry stays 0
      superblock.set(s, first);
      if(last - first > logn4) { is_long[s] = true; any_long = true; }
    }
    superblock.serialize(out, true);
    PackedVector mini_or_long(any_long ? sb : 0, 1);
    if(any_long) { for(size_type s = 0; s < sb; s++) { if(!is_long[s]) { mini_or_long.set(s, 1); } } }
    mini_or_long.serialize(out, false);
    for(size_type s = 0; s < sb; s++)
    {
      size_type begin = s * SUPER, end = std::min(arg_cnt, (s + 1) * SUPER);
      if(is_long[s])
      {
        PackedVector block(SUPER, (tail_long && s + 1 == sb ? hi(n - 1) : hi(args[end - 1])) + 1);
        for(size_type k = begin; k < end; k++) { block.set(k - begin, args[k]); }
        block.serialize(out, true);
      }
      else
      {
        PackedVector block(64, hi(args[end - 1] - args[begin]) + 1);
        for(size_type k = begin; k < end; k += 64) { block.set((k - begin) / 64, args[k] - args[begin]); }
        block.serialize(out, true);
      }
    }
  }

  // Skips a serialized select support over a vector with `expected` selected bits (the facade rebuilds nothing from it): its
  // framing is checked -- the argument count, one superblock entry per 4096 arguments, mini_or_long empty or one bit per
  // superblock, 64 or 4096 entries per block -- its contents are not.
  static void skip(Source& in, size_type expected, const char* what)
  {
    const size_type arg_cnt = in.get<size_type>(what);
    if(arg_cnt != expected) { PackedVector::refuse(in, what, "counts", arg_cnt, "arguments, the vector has another number"); }
    if(arg_cnt == 0) { return; }
    const size_type sb = (arg_cnt + 4095) / 4096;
    if(PackedVector::skip(in, true, 0, what) != sb) { in.refuse(std::string(what) + " does not have one superblock entry per 4096 arguments"); }
    const size_type flagged = PackedVector::skip(in, false, 1, what);
    if(flagged != 0 && flagged != sb) { in.refuse(std::string(what) + " does not have one mini_or_long bit per superblock"); }
    for(size_type s = 0; s < sb; s++)
    {
      const size_type entries = PackedVector::skip(in, true, 0, what);
      if(entries != 64 && entries != 4096) { PackedVector::refuse(in, what, "has a block of", entries, "entries (64 or 4096 expected)"); }
    }
  }
};

// sd_vector<>: Elias-Fano over `ones` (strictly increasing) in a universe of `size` bits.
struct SDVector
{
  static void serialize(std::ostream& out, size_type size, const std::vector<size_type>& ones)
  {
    size_type m = ones.size();
    size_type logm = hi(m) + 1, logn = hi(size) + 1;
    if(logm == logn) { logm--; }
    std::uint8_t wl = (std::uint8_t)(logn - logm);
    PackedVector low(m, wl), high(m + ((size_type)1 << logm), 1);
    for(size_type k = 0; k < m; k++)
    {
      low.set(k, ones[k]);
      high.set((ones[k] >> wl) + k, 1);
    }
    write_member(size, out);
    write_member(wl, out);
    low.serialize(out, true);
    high.serialize(out, false);
    SelectMCL::serialize(out, high, true);
    SelectMCL::serialize(out, high, false);
  }

  // `what` names the member in messages.  What sd_vector's builder guarantees is checked: wl < 64 is the width of the m low
  // parts, wl = logn - logm by the rule above, high has m + 2^logm bits of which exactly m are set, and the positions are
  // strictly increasing below `size`; so are the argument counts of the two select supports.
  static void load(Source& in, size_type& size, std::vector<size_type>& ones, const char* what)
  {
    size = in.get<size_type>(what);
    const size_type wl = in.get<std::uint8_t>(what);
    if(wl >= 64) { PackedVector::refuse(in, what, "has low parts of", wl, "bits"); }
    PackedVector low, high;
    low.load(in, true, 0, what);
    const size_type m = low.count;
    size_type logm = hi(m) + 1, logn = hi(size) + 1;
    if(logm == logn) { logm--; }
    if(low.width != wl || wl != logn - logm) { PackedVector::refuse(in, what, "has low parts of", low.width, "bits that do not follow from its size fields"); }
    high.load(in, false, 1, what);
    const size_type nbits = high.bit_size();
    if(nbits != m + ((size_type)1 << logm)) { PackedVector::refuse(in, what, "has", nbits, "high bits that do not follow from its size fields"); }
    ones.assign(m, 0);
    size_type k = 0, disorder = 0, before = 0;            // (the order is checked on the way, without a branch per entry)
    for(size_type w = 0; w * 64 < nbits; w++)
    {
      std::uint64_t word = high.words[w];
      if((w + 1) * 64 > nbits) { word &= (~(std::uint64_t)0) >> (64 - (nbits - w * 64)); }
      if(k + (size_type)__builtin_popcountll(word) > m) { k = m + 1; break; }
      while(word != 0)
      {
        const size_type pos = w * 64 + (size_type)__builtin_ctzll(word); word &= word - 1;
        const size_type value = ((pos - k) << wl) | low.get(k);
        disorder |= (size_type)(value < before) | (size_type)(value >= size);
        ones[k] = value; before = value + 1; k++;
      }
    }
    if(k != m) { PackedVector::refuse(in, what, "does not have one high bit for each of its", m, "low parts"); }
    if(disorder != 0) { PackedVector::refuse(in, what, "is not strictly increasing below its size of", size, ""); }
    SelectMCL::skip(in, m, what); SelectMCL::skip(in, nbits - m, what);
  }
};

} // namespace sdsl_compat
} // namespace bwtmerge

#endif // BWTM_HOST_SDSL_COMPAT_H
