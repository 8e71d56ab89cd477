/*
  host_cpu_test -- the parts of the C++ facade that need no GPU: Run / ByteCode / RunBuffer / getBounds, BWT queries on the full
  and on the COMPACT form of the samples (the form a merge downloads: 8- / 16- / 32-bit per-block fields + anchors every 64 blocks),
  expandSamples(), native serialization round trip; and the plain C++ of the library's batch scheme (../api/batches.hip.h: validate_texts,
  two_round_call, CallStats) over a fail() that keeps the message.  Exit code 0 = every check passed.
*/
#include <cstdarg>
#include <cstdio>
#include <random>
#include "fmi.h"

using namespace bwtmerge;
size_type Parallel::max_threads = 2;

static int failures = 0;
#define CHECK(cond) do { if(!(cond)) { std::fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__); failures++; } } while(0)

// What api/batches.hip.h takes from api/context.hip.h and the kernels' header.
typedef std::uint8_t u8; typedef std::uint32_t u32; typedef std::uint64_t u64;
static std::string g_error;
static int fail(int code, const char* fmt, ...)
{
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
  g_error = buf;
  return code;
}
#define TRY(expr) do { int rc_ = (expr); if(rc_ != BWTM_OK) { return rc_; } } while(0)
#include "../api/batches.hip.h"

static bool refused(int rc, const char* text) { return rc == BWTM_EINVAL && g_error == text; }

static void testValidateTexts()
{
  const u8 text[] = {1, 2, 3, 4, 5, 5, 1};
  const u64 off[] = {0, 3, 3, 7};
  CHECK(validate_texts("f", "pattern", text, off, 3, 4) == BWTM_OK);
  CHECK(validate_texts("f", "pattern", text, off, 3, 0) == BWTM_OK);                    // 0: no limit
  CHECK(refused(validate_texts("f", "pattern", text, off, 3, 3), "f: pattern 2 has 4 symbols (at most 3)"));
  const u64 empty[] = {5, 5, 5};
  CHECK(validate_texts("f", "query", nullptr, empty, 2, 0) == BWTM_OK);                 // an empty text may be null
  CHECK(refused(validate_texts("f", "query", nullptr, off, 3, 0), "f: null query text"));
  CHECK(refused(validate_texts("f", "pattern", nullptr, off, 3, 0), "f: null pattern text"));
  const u64 back[] = {0, 3, 2, 7};
  CHECK(refused(validate_texts("f", "pattern", text, back, 3, 0), "f: offsets must not decrease (pattern 1)"));
  CHECK(refused(validate_texts("f", "query", text, back, 3, 0), "f: offsets must not decrease (query 1)"));
  const u8 zero[] = {1, 2, 3, 4, 0, 5, 1}, six[] = {1, 2, 3, 4, 5, 5, 6};
  CHECK(refused(validate_texts("f", "pattern", zero, off, 3, 0), "f: pattern 2 holds the symbol 0 at offset 1 (comp values 1..5)"));
  CHECK(refused(validate_texts("f", "query", six, off, 3, 0), "f: query 2 holds the symbol 6 at offset 3 (comp values 1..5)"));
  // two faults: the offsets are looked at first, whichever text comes first, and no text is read through them
  const u8 bad0[] = {0, 2, 3, 4, 5, 5, 1};
  const u64 late[] = {0, 3, 5, 4};
  CHECK(refused(validate_texts("f", "pattern", bad0, late, 3, 2), "f: offsets must not decrease (pattern 2)"));
  CHECK(refused(validate_texts("f", "query", nullptr, late, 3, 0), "f: offsets must not decrease (query 2)"));
  const u64 far[] = {0, ~0ull, 1};                                                       // nothing at text[2^64 - 1] is touched
  CHECK(refused(validate_texts("f", "pattern", text, far, 2, 0), "f: offsets must not decrease (pattern 1)"));
  // a null text comes before a length, a length before a symbol of the same text, an earlier text's symbol before a later one's length
  CHECK(refused(validate_texts("f", "pattern", nullptr, off, 3, 3), "f: null pattern text"));
  CHECK(refused(validate_texts("f", "pattern", zero, off, 3, 3), "f: pattern 2 has 4 symbols (at most 3)"));
  CHECK(refused(validate_texts("f", "pattern", bad0, off, 3, 3), "f: pattern 0 holds the symbol 0 at offset 0 (comp values 1..5)"));
}

// A model batch for two_round_call: per[k] things per text, batches of `batch` texts (or as `cuts` says), and a log of what ran.
struct ModelCall
{
  std::vector<u64> per, cuts;                           // cuts: the batch sizes in order (empty: `batch` each)
  u64 batch = 1;
  std::vector<std::string> log;
  std::vector<u64> filled;                              // the caller's array
  CallStats stats;
  u64 staged = ~0ull;                                   // the batch whose state is held: the first text of the last size()
  u64 fail_fill_at = ~0ull;

  u64 batchAt(u64 done) const
  {
    if(cuts.empty()) { return std::min<u64>(batch, per.size() - done); }
    u64 at = 0;
    for(u64 c : cuts) { if(at == done) { return c; } at += c; }
    return 0;
  }
  int run(bool wanted, u64 capacity, std::vector<u64>& offsets)
  {
    offsets.assign(per.size() + 1, 777); offsets[0] = 0;
    filled.assign(capacity, 999);
    log.clear(); stats.reset();
    return two_round_call("f", "hits", per.size(), offsets.data(), wanted, capacity, &stats,
      [&](u64 done) { return batchAt(done); },
      [&](u64 done, u64 nb, u64* out) -> int
      {
        log.push_back("size " + std::to_string(done) + "+" + std::to_string(nb));
        for(u64 k = 0; k < nb; k++) { out[k + 1] = out[k] + per[done + k]; stats[0] += per[done + k] + 1; }
        stats[1] = std::max(stats[1], nb); stats[3]++;
        staged = done;
        return BWTM_OK;
      },
      [&](u64 done, u64 nb, u64 at) -> int
      {
        log.push_back("fill " + std::to_string(done) + "+" + std::to_string(nb) + "@" + std::to_string(at));
        if(done == fail_fill_at) { return fail(BWTM_EINVAL, "f: fill of batch %llu", (unsigned long long)done); }
        CHECK(staged == done);                                                          // the state filled from is this batch's
        u64 slot = at;
        for(u64 k = 0; k < nb; k++) { for(u64 j = 0; j < per[done + k]; j++) { CHECK(slot < filled.size()); if(slot < filled.size()) { filled[slot++] = 100 * (done + k) + j; } } }
        return BWTM_OK;
      });
  }
};

static void testTwoRoundCall()
{
  typedef std::vector<std::string> Log;
  ModelCall m;
  m.per = {2, 0, 3, 0, 0, 0, 1, 4};                                                     // 10 things; batches of 3: {2,0,3} {0,0,0} {1,4}
  m.batch = 3;
  const std::vector<u64> want_offsets = {0, 2, 2, 5, 5, 5, 5, 6, 10};
  const Log sizes = {"size 0+3", "size 3+3", "size 6+2"};
  std::vector<u64> off;
  // sizes only: no array, no capacity
  CHECK(m.run(false, 10, off) == BWTM_OK && off == want_offsets && m.log == sizes);
  CHECK(m.run(true, 0, off) == BWTM_OK && off == want_offsets && m.log == sizes);
  u64 sized[4]; CHECK(m.stats.get("s", sized) == BWTM_OK);
  CHECK(sized[0] == 18 && sized[1] == 3 && sized[3] == 3);
  // one short: refused after the sizes and before anything is written
  CHECK(refused(m.run(true, 9, off), "f: capacity 9 is too small (10 hits)"));
  CHECK(off == want_offsets && m.log == sizes && m.filled == std::vector<u64>(9, 999));
  // exact: every batch sized a second time, filled at its slot; the flat batch in the middle moves nothing; the statistics count once
  CHECK(m.run(true, 10, off) == BWTM_OK && off == want_offsets);
  CHECK(m.log == Log({"size 0+3", "size 3+3", "size 6+2", "size 0+3", "fill 0+3@0", "size 3+3", "fill 3+3@5", "size 6+2", "fill 6+2@5"}));
  CHECK(m.filled == std::vector<u64>({0, 1, 200, 201, 202, 600, 700, 701, 702, 703}));
  u64 after[4]; CHECK(m.stats.get("s", after) == BWTM_OK);
  for(int j = 0; j < 4; j++) { CHECK(after[j] == sized[j]); }
  CHECK(refused(m.stats.get("s", nullptr), "s: null argument"));
  // room to spare: the slots behind the last thing are untouched
  CHECK(m.run(true, 12, off) == BWTM_OK && m.filled[9] == 703 && m.filled[10] == 999 && m.filled[11] == 999);
  // a fill that fails ends the call with its own message
  m.fail_fill_at = 3;
  CHECK(refused(m.run(true, 10, off), "f: fill of batch 3") && m.log.back() == "fill 3+3@5" && m.filled[5] == 999);
  m.fail_fill_at = ~0ull;
  // one batch covers the call: sized once, its state kept for the fill
  m.batch = 8;
  CHECK(m.run(true, 10, off) == BWTM_OK && off == want_offsets && m.log == Log({"size 0+8", "fill 0+8@0"}));
  CHECK(m.filled == std::vector<u64>({0, 1, 200, 201, 202, 600, 700, 701, 702, 703}));
  m.batch = 100;                                                                        // a knob above the count: batch_at(0) is what is left
  CHECK(m.run(true, 10, off) == BWTM_OK && m.log == Log({"size 0+8", "fill 0+8@0"}));
  // batches of unequal sizes (the cut at a symbol limit), the last of one text
  m.cuts = {4, 1, 2, 1};
  CHECK(m.run(true, 10, off) == BWTM_OK && off == want_offsets);
  CHECK(m.log == Log({"size 0+4", "size 4+1", "size 5+2", "size 7+1", "size 0+4", "fill 0+4@0", "size 4+1", "fill 4+1@5", "size 5+2", "fill 5+2@5", "size 7+1", "fill 7+1@6"}));
  CHECK(m.filled == std::vector<u64>({0, 1, 200, 201, 202, 600, 700, 701, 702, 703}));
  // nothing found: no second round whatever the capacity
  m.cuts.clear(); m.batch = 3; m.per.assign(8, 0);
  CHECK(m.run(true, 5, off) == BWTM_OK && off == std::vector<u64>(9, 0) && m.log == sizes);
  // without statistics
  u64 two[3] = {0, 7, 7}; int fills = 0;
  CHECK(two_round_call("f", "MEMs", 2, two, true, 1, nullptr, [](u64) { return (u64)1; }, [](u64, u64, u64* out) { out[1] = out[0] + 1; return BWTM_OK; },
    [&](u64, u64, u64) { fills++; return BWTM_OK; }) == BWTM_EINVAL && g_error == "f: capacity 1 is too small (2 MEMs)" && fills == 0);
  CHECK(two_round_call("f", "MEMs", 2, two, true, 2, nullptr, [](u64) { return (u64)1; }, [](u64, u64, u64* out) { out[1] = out[0] + 1; return BWTM_OK; },
    [&](u64, u64, u64 at) { CHECK(at == (u64)fills); fills++; return BWTM_OK; }) == BWTM_OK && fills == 2);
}

// Installs the compact form of `full`'s samples into `target` (what bwtm_index_download_samples_compact delivers).
static void installCompact(const BWT& full, BWT& target, int width)
{
  const size_type nb = full.blocks(), nanch = (nb + 63) / 64;
  target.cum_stride = nb + 1; target.sample_width = width;
  target.anchors.resize(BWT::SIGMA * nanch);
  target.fields.resize((BWT::SIGMA * nb * (size_type)width + 1) / 2);
  for(size_type k = 0; k < nb; k++)
  {
    size_type start = (k == 0 ? 0 : full.block_end[k - 1] + 1), length = full.block_end[k] + 1 - start;
    for(size_type c = 0; c < BWT::SIGMA; c++)
    {
      size_type value = (c == 0 ? length : full.cum(c, k + 1) - full.cum(c, k));
      if(width == 1) { ((std::uint8_t*)target.fields.data())[c * nb + k] = (std::uint8_t)value; }
      else if(width == 2) { target.fields[c * nb + k] = (std::uint16_t)value; }
      else { ((std::uint32_t*)target.fields.data())[c * nb + k] = (std::uint32_t)value; }
      if(k % 64 == 0) { target.anchors[c * nanch + k / 64] = (c == 0 ? start : full.cum(c, k)); }
    }
  }
  target.block_end.clear(); target.cum_flat.clear();
}

int main()
{
  testValidateTexts();
  testTwoRoundCall();

  // Run::write block rule against the reference's vectors: len 170 at offset 62, len 16426 at offset 61.
  {
    BlockArray a; for(int k = 0; k < 62; k++) { a.push_back(0); }
    Run::write(a, 3, 170);
    CHECK(a.size() == 65 && a[62] == 0xf9 && a[63] == 0x7f && a[64] == 0x03);
    BlockArray b; for(int k = 0; k < 61; k++) { b.push_back(0); }
    Run::write(b, 3, 16426);
    CHECK(b.size() == 65 && b[61] == 0xf9 && b[62] == 0xff && b[63] == 0x7f && b[64] == 0x03);
    size_type pos = 61; range_type r1 = Run::read(b, pos), r2 = Run::read(b, pos);
    CHECK(r1 == range_type(3, 16425) && r2 == range_type(3, 1) && pos == 65);
  }
  CHECK(getBounds(range_type(0, 9), 4) == std::vector<range_type>({range_type(0, 1), range_type(2, 3), range_type(4, 6), range_type(7, 9)}));

  std::mt19937_64 rng(5);
  for(int variant = 0; variant < 4; variant++)
  {
    // a run-structured string: short runs (variant 0), runs up to 70000 (variant 1: needs 32-bit fields), tiny (variant 2)
    FMI full;
    std::vector<byte_type> symbols;
    size_type nruns = (variant == 2 ? 5 : 30000);
    comp_type previous = 6;
    for(size_type k = 0; k < nruns; k++)
    {
      comp_type c = (comp_type)(rng() % 6); if(c == previous) { c = (comp_type)((c + 1) % 6); } previous = c;
      size_type choices0[] = {1, 1, 2, 3, 41, 42, 170}, choices1[] = {1, 2, 50, 70000, 3};
      size_type len = (variant == 1 ? choices1[rng() % 5] : (variant == 3 ? choices0[rng() % 4] : choices0[rng() % 7]));   // variant 3: runs of 1 .. 3, 8-bit fields
      Run::write(full.bwt.data, c, len);
      if(symbols.size() < 400000) { for(size_type j = 0; j < len && symbols.size() < 400000; j++) { symbols.push_back(c); } }
    }
    full.bwt.buildFromData();
    const size_type n = full.bwt.size();
    int width = (variant == 1 ? 4 : (variant == 3 ? 1 : 2));
    FMI compact; compact.bwt.header = full.bwt.header; compact.bwt.data = full.bwt.data;
    installCompact(full.bwt, compact.bwt, width);
    CHECK(compact.bwt.blocks() == full.bwt.blocks() && compact.bwt.blockEnds() == full.bwt.blockEnds());
    for(size_type c = 0; c < 6; c++) { CHECK(compact.bwt.cumulative(c) == full.bwt.cumulative(c)); CHECK(compact.bwt.count((comp_type)c) == full.bwt.count((comp_type)c)); }
    // queries on both forms against each other and against the plain prefix of the string
    size_type seen[6] = {};
    for(size_type i = 0; i <= std::min<size_type>(n, symbols.size()); i++)
    {
      if(i % 97 == 0 || i + 1 >= symbols.size())
      {
        for(comp_type c = 0; c < 6; c++) { CHECK(full.bwt.rank(i, c) == seen[c]); CHECK(compact.bwt.rank(i, c) == seen[c]); }
        if(i < n && i < symbols.size())
        {
          CHECK(compact.bwt[i] == symbols[i] && compact.bwt.inverse_select(i) == full.bwt.inverse_select(i));
          CHECK(compact.bwt.select(seen[symbols[i]] + 1, symbols[i]) == i);
        }
      }
      if(i < symbols.size()) { seen[symbols[i]]++; }
    }
    for(size_type t = 0; t < 2000; t++)
    {
      size_type i = rng() % (n + 1); comp_type c = (comp_type)(rng() % 6);
      CHECK(compact.bwt.rank(i, c) == full.bwt.rank(i, c));
      size_type cnt = full.bwt.count(c);
      if(cnt > 0) { size_type k = 1 + rng() % cnt; CHECK(compact.bwt.select(k, c) == full.bwt.select(k, c)); }
    }
    // expansion gives back the full arrays; serialization of either form gives the same file
    FMI expanded = compact; expanded.bwt.expandSamples();
    CHECK(expanded.bwt.sample_width == 8 && expanded.bwt.block_end == full.bwt.block_end && expanded.bwt.cum_flat == full.bwt.cum_flat);
    std::vector<size_type> counts(6); for(size_type c = 0; c < 6; c++) { counts[c] = full.bwt.count((comp_type)c); }
    full.alpha = Alphabet(counts); compact.alpha = full.alpha;
    std::string f1 = "/tmp/bwtm_host_cpu_test_full.native", f2 = "/tmp/bwtm_host_cpu_test_compact.native";
    serialize(full, f1, "native"); serialize(compact, f2, "native");
    std::ifstream i1(f1, std::ios_base::binary), i2(f2, std::ios_base::binary);
    std::vector<char> b1((std::istreambuf_iterator<char>(i1)), std::istreambuf_iterator<char>()), b2((std::istreambuf_iterator<char>(i2)), std::istreambuf_iterator<char>());
    CHECK(!b1.empty() && b1 == b2);
    FMI back; load(back, f2, "native");
    CHECK(back.bwt.data.bytes == full.bwt.data.bytes && back.bwt.block_end == full.bwt.block_end && back.bwt.cum_flat == full.bwt.cum_flat && back.alpha.C == full.alpha.C);
    std::remove(f1.c_str()); std::remove(f2.c_str());
  }

  if(failures == 0) { std::printf("host_cpu_test: all checks passed\n"); return 0; }
  std::fprintf(stderr, "host_cpu_test: %d checks failed\n", failures);
  return 1;
}
