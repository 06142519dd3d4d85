// field_names.cpp — kx_field_names.h (the parser of `--field` lists with names, the cutter of a header record's cells and the
// resolver of names) over seeded random headers against a plain reference written here, in a stand-alone program that is built
// with AddressSanitizer and UBSan (tests/test_records_header.py).  `field_names CASES` prints "CASES cases" and exits 0; it fails if
// a result differs or if one of the populations the cases must cover was never drawn.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../include/kxhip.h"
#include "../../kleenexlang_amd/csrc/engine/kx_field_names.h"

namespace {

typedef std::vector<uint8_t> Bytes;

[[noreturn]] void fail(const char* what, uint64_t c) {
  fprintf(stderr, "case %llu: %s\n", (unsigned long long)c, what);
  exit(1);
}

// ---- the reference: liveness first, then the cuts, then the values ------------------------------------------------------------
std::vector<bool> refLive(const Bytes& b, int quote, int escape, bool words, uint8_t fs) {
  std::vector<bool> live(b.size(), false);
  bool inside = false;
  for (size_t i = 0; i < b.size(); ++i) {
    if (escape >= 0 && b[i] == escape) { ++i; continue; }   // the escape byte and the byte it takes are data
    if (quote >= 0 && b[i] == quote) { inside = !inside; continue; }
    if (inside) continue;
    live[i] = words ? (b[i] == ' ' || b[i] == '\t') : b[i] == fs;
  }
  return live;
}

std::string refValue(const Bytes& raw, int quote, int escape) {
  std::string v;
  int state = 0;   // 0 outside, 1 inside quotes, 2 just closed
  for (size_t i = 0; i < raw.size(); ++i) {
    if (escape >= 0 && raw[i] == escape) {
      if (i + 1 < raw.size()) v.push_back((char)raw[++i]);
      if (state == 2) state = 0;
      continue;
    }
    if (quote >= 0 && raw[i] == quote) {
      if (state == 1) state = 2;
      else { if (state == 2) v.push_back((char)quote); state = 1; }
      continue;
    }
    v.push_back((char)raw[i]);
    if (state == 2) state = 0;
  }
  return v;
}

std::vector<std::string> refCells(Bytes b, uint8_t fs, int quote, int escape, bool words, bool first) {
  if (first && b.size() >= 3 && b[0] == 0xEF && b[1] == 0xBB && b[2] == 0xBF) b.erase(b.begin(), b.begin() + 3);
  const std::vector<bool> live = refLive(b, quote, escape, words, fs);
  std::vector<Bytes> raw;
  Bytes cur;
  bool open = !words;   // a cell is being collected (with a separator: always)
  for (size_t i = 0; i < b.size(); ++i) {
    if (live[i]) {
      if (open) raw.push_back(cur);
      cur.clear();
      open = !words;
    } else {
      cur.push_back(b[i]);
      open = true;
    }
  }
  if (open) raw.push_back(cur);
  std::vector<std::string> cells;
  for (const Bytes& r : raw) cells.push_back(quote >= 0 || escape >= 0 ? refValue(r, quote, escape) : std::string(r.begin(), r.end()));
  return cells;
}

// a name spelled for the command line: commas and backslashes escaped, other bytes sometimes as \xHH
std::string spell(const std::string& name, std::mt19937_64& rnd) {
  static const char* const digits = "0123456789abcdef";
  std::string s;
  for (const unsigned char c : name) {
    if (c == ',') s += "\\,";
    else if (c == '\\') s += "\\\\";
    else if (c == '\n') s += "\\n";
    else if (c == '\t') s += rnd() % 2 ? "\\t" : "\t";
    else if (c == 0) s += "\\0";
    else if (c < 0x20 || c >= 0x7F || rnd() % 8 == 0) { s += "\\x"; s.push_back(digits[c >> 4]); s.push_back(digits[c & 15]); }
    else s.push_back((char)c);
  }
  return s;
}

bool allNumberChars(const std::string& s) {
  for (const char c : s) if (!((c >= '0' && c <= '9') || c == '-')) return false;
  return true;
}

void refusals() {
  std::vector<KxFieldNameItem> it;
  const std::string long_name(256, 'a'), ok_name(255, 'a');
  std::string seventeen = "a";
  for (int i = 0; i < 16; ++i) seventeen += ",1";
  for (const std::string& bad : {std::string("a,,b"), std::string("a\\q"), std::string("a\\"), std::string("a\\x4"), std::string("a\\xg1"), long_name,
                                 seventeen, std::string("a,0"), std::string("a,5-2"), std::string("a,-3"), std::string("a,1-2-3"), std::string("a,4294967296"),
                                 std::string(""), std::string("a,")}) {
    it.clear();
    if (!kxParseFieldNames(bad.c_str(), &it)) { fprintf(stderr, "accepted: %s\n", bad.c_str()); exit(1); }
  }
  it.clear();
  if (kxParseFieldNames(ok_name.c_str(), &it) || it.size() != 1 || it[0].name != ok_name) fail("a 255-byte name", 0);
  it.clear();
  if (kxParseFieldNames("user-id,a\\,b,\\x2c,2,5-7,9-", &it) || it.size() != 6 || it[0].name != "user-id" || it[1].name != "a,b" || it[2].name != "," ||
      it[3].is_name || it[3].lo != 2 || it[3].hi != 2 || it[4].lo != 5 || it[4].hi != 7 || it[5].lo != 9 || it[5].hi != 1ull << 32)
    fail("the example list", 0);
  if (!kxFieldTextHasName("2,x") || kxFieldTextHasName("2,5-7,9-") || !kxFieldTextHasName("\\,")) fail("kxFieldTextHasName", 0);
  if (kxPrintableName(std::string("a\0\xff b", 5)) != "a\\x00\\xFF b") fail("kxPrintableName", 0);
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20000;
  refusals();
  std::mt19937_64 rnd(20240607);
  uint64_t seen_quoted = 0, seen_escaped = 0, seen_doubled = 0, seen_dup = 0, seen_bom = 0, seen_missing = 0, seen_ranges = 0, seen_words = 0;
  for (uint64_t c = 0; c < cases; ++c) {
    const int mode = (int)(rnd() % 4);   // plain, quote, quote + escape, escape
    const int quote = mode == 1 || mode == 2 ? '"' : -1, escape = mode >= 2 ? '\\' : -1;
    const bool words = rnd() % 4 == 0, first = rnd() % 2 == 0, bom = rnd() % 8 == 0;
    const uint8_t fs = ',';
    // a header body of random cells over a small alphabet; many cells so that more than 8 ranges can come
    const size_t ncells = 1 + rnd() % 24;
    static const char alphabet[] = "abc,\" \t\\;-1\xc3\xa9";
    Bytes body;
    if (bom) { body.push_back(0xEF); body.push_back(0xBB); body.push_back(0xBF); }
    for (size_t k = 0; k < ncells; ++k) {
      if (k) body.push_back(words ? (rnd() % 2 ? ' ' : '\t') : fs);
      const int kind = (int)(rnd() % 6);
      const size_t len = rnd() % 4;
      if (kind == 0 && quote >= 0) {   // a quoted cell, with "" and separators inside
        body.push_back('"');
        for (size_t j = 0; j < len; ++j) {
          const int what = (int)(rnd() % 5);
          if (what == 0) { body.push_back('"'); body.push_back('"'); ++seen_doubled; }
          else if (what == 1) body.push_back(words ? ' ' : fs);
          else body.push_back((uint8_t)('a' + rnd() % 3));
        }
        body.push_back('"');
        ++seen_quoted;
      } else if (kind == 1 && escape >= 0) {
        body.push_back('x'); body.push_back('\\'); body.push_back(words ? ' ' : fs); body.push_back('y');
        ++seen_escaped;
      } else if (kind == 2) {
        body.push_back((uint8_t)('a' + rnd() % 2));   // short names: duplicates
      } else {
        for (size_t j = 0; j <= len; ++j) body.push_back((uint8_t)alphabet[rnd() % (sizeof alphabet - 1)]);
      }
    }
    if (bom && first) ++seen_bom;
    if (words) ++seen_words;
    std::vector<std::string> got, want = refCells(body, fs, quote, escape, words, first);
    kxHeaderCellNames(body.data(), body.size(), fs, quote, escape, words, first, &got);
    if (got != want) fail("the cells' names differ", c);
    std::map<std::string, uint32_t> lowest;
    for (size_t k = want.size(); k-- > 0;) lowest[want[k]] = (uint32_t)k + 1;
    if (lowest.size() < want.size()) ++seen_dup;
    // a list of names of cells (every second cell now and then, for many ranges), numbers and now and then a name no cell has
    std::string text;
    std::vector<KxFieldNameItem> written;
    const size_t nitems = 1 + rnd() % 16;
    const bool spread = rnd() % 6 == 0;
    bool has_missing = false;
    for (size_t j = 0; j < nitems; ++j) {
      KxFieldNameItem it;
      const int kind = (int)(rnd() % 8);
      if (spread && j) {
        it.lo = it.hi = 3 * j;   // (single fields two apart: nine of them and the union has too many ranges)
      } else if (kind == 0) {
        it.lo = 1 + rnd() % 30; it.hi = rnd() % 3 == 0 ? 1ull << 32 : it.lo + rnd() % 3;
      } else {
        it.is_name = true;
        if (kind == 1 || want.empty()) it.name = "zz" + std::to_string(rnd() % 10);
        else it.name = want[spread ? (2 * j) % want.size() : rnd() % want.size()];
        if (it.name.empty() || it.name.size() > KX_FIELD_NAME_MAX || allNumberChars(it.name)) { it.is_name = false; it.lo = it.hi = 1 + j; }
      }
      if (j) text += ",";
      if (it.is_name) text += spell(it.name, rnd);
      else text += std::to_string(it.lo) + (it.hi == it.lo ? "" : it.hi == 1ull << 32 ? "-" : "-" + std::to_string(it.hi));
      if (it.is_name && !lowest.count(it.name)) has_missing = true;
      written.push_back(it);
    }
    bool any_name = false;
    for (const auto& it : written) any_name |= it.is_name;
    if (!any_name) continue;
    std::vector<KxFieldNameItem> parsed;
    if (const char* why = kxParseFieldNames(text.c_str(), &parsed)) { fprintf(stderr, "%s: %s\n", text.c_str(), why); fail("the parser refused a good list", c); }
    if (parsed.size() != written.size()) fail("the parser's item count", c);
    for (size_t j = 0; j < parsed.size(); ++j)
      if (parsed[j].is_name != written[j].is_name || (parsed[j].is_name ? parsed[j].name != written[j].name : parsed[j].lo != written[j].lo || parsed[j].hi != written[j].hi))
        fail("a parsed item differs", c);
    // the resolver against the map
    kx_field_range items[KX_FIELD_ITEMS] = {}, out[KX_FIELD_ITEMS] = {}, ranges[KX_FIELD_RANGES] = {};
    std::vector<std::string> names;
    for (size_t j = 0; j < parsed.size(); ++j) {
      if (parsed[j].is_name) { items[j] = kx_field_range{0u, (uint32_t)names.size()}; names.push_back(parsed[j].name); }
      else items[j] = kx_field_range{(uint32_t)parsed[j].lo, parsed[j].hi == 1ull << 32 ? 0u : (uint32_t)parsed[j].hi};
    }
    uint32_t n_ranges = 0, missing = 0;
    const int rc = kxResolveFieldNames(items, (uint32_t)parsed.size(), names, got, out, ranges, &n_ranges, &missing);
    if (has_missing) {
      ++seen_missing;
      if (rc != 1 || missing >= names.size() || lowest.count(names[missing])) fail("a missing name was not reported", c);
      continue;
    }
    if (rc == 1) fail("a name that a cell has was reported missing", c);
    std::vector<bool> member(64, false);   // the selected set below 64, and whether it is open
    uint64_t open_from = 0;
    for (size_t j = 0; j < parsed.size(); ++j) {
      const uint64_t lo = parsed[j].is_name ? lowest[parsed[j].name] : parsed[j].lo;
      const uint64_t hi = parsed[j].is_name ? lo : parsed[j].hi;
      if (out[j].lo != lo || out[j].hi != (hi == 1ull << 32 ? 0u : (uint32_t)hi)) fail("a resolved item differs", c);
      for (uint64_t k = lo; k < 64 && k <= hi; ++k) member[k] = true;
      if (hi == 1ull << 32) open_from = open_from ? std::min(open_from, lo) : lo;
    }
    if (open_from) for (uint64_t k = open_from; k < 64; ++k) member[k] = true;
    uint32_t runs = 0;
    for (uint64_t k = 1; k < 64; ++k) if (member[k] && !member[k - 1]) ++runs;
    if (runs > KX_FIELD_RANGES) {
      ++seen_ranges;
      if (rc != 2) fail("more than 8 ranges were not refused", c);
      continue;
    }
    if (rc != 0 || n_ranges != runs || !kxFieldListIsNormal(ranges, n_ranges)) fail("the union is not the normal form", c);
    std::vector<bool> covered(64, false);
    for (uint32_t j = 0; j < n_ranges; ++j)
      for (uint64_t k = ranges[j].lo; k < 64 && (ranges[j].hi == 0 || k <= ranges[j].hi); ++k) covered[k] = true;
    if (covered != member) fail("the union selects other fields", c);
  }
  const uint64_t floor = cases / 2000;
  for (const auto& pop : {std::make_pair("quoted cells", seen_quoted), std::make_pair("escaped bytes", seen_escaped), std::make_pair("doubled quotes", seen_doubled),
                          std::make_pair("duplicate names", seen_dup), std::make_pair("byte-order marks", seen_bom), std::make_pair("missing names", seen_missing),
                          std::make_pair("more than 8 ranges", seen_ranges), std::make_pair("words", seen_words)})
    if (pop.second <= floor) { fprintf(stderr, "population never drawn (or too rarely): %s (%llu)\n", pop.first, (unsigned long long)pop.second); return 1; }
  printf("%llu cases\n", (unsigned long long)cases);
  return 0;
}
