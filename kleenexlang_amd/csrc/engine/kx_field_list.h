// kx_field_list.h — the LIST of `--field=LIST` (2,5-7,9-): its parser, its normal form and the check of a normal form.  Host
// code without a dependency beyond include/kxhip.h (kx_field_range): kxrun.cpp parses the option text with it before the engine
// library is loaded, and the library checks a kx_batch_field_list with it (kx_field_list_host.inc).  The Python restatement is
// host.parse_field_list.
//
// LIST = item (',' item)*;  item = K | A-B (A <= B) | A- (A and everything behind it).  A number is 1 to 10 decimal digits with a
// value from 1 to 4294967295.  The NORMAL FORM is the selected set as ranges that are sorted, disjoint and not adjacent:
// 3,2 -> 2-3;  4-,2,6 -> 2,4-.  Only its last range can be open (hi = 0).  At most KX_FIELD_RANGES ranges.  With `--only` the
// list is also kept AS WRITTEN, at most KX_FIELD_ITEMS items (kxParseFieldOrder; host.parse_field_order): the output's order.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

constexpr uint32_t KX_FIELD_RANGES = 8;

// an option text that is one plain number: `--field=K`, the single-field path
inline bool kxFieldIsPlainNumber(const char* text) {
  if (!*text) return false;
  for (const char* p = text; *p; ++p) if (*p < '0' || *p > '9') return false;
  return true;
}

// the list a kx_field_range array must hold: lo >= 1; hi == 0 (open) or hi >= lo; a gap of at least one field between two
// ranges; only the last one open
inline bool kxFieldListIsNormal(const kx_field_range* r, uint32_t n) {
  if (n < 1 || n > KX_FIELD_RANGES) return false;
  for (uint32_t j = 0; j < n; ++j) {
    if (r[j].lo < 1 || (r[j].hi != 0 && r[j].hi < r[j].lo)) return false;
    if (j + 1 < n && (r[j].hi == 0 || (uint64_t)r[j + 1].lo <= (uint64_t)r[j].hi + 1)) return false;
  }
  return true;
}

constexpr uint32_t KX_FIELD_ITEMS = 16;   // the items of a list kept as written (`--only`)

// the text's items as written, (A, B) with B = 2^32 for an open one.  Returns null, or what is wrong with the text (a static string).
inline const char* kxParseFieldItems(const char* text, std::vector<std::pair<uint64_t, uint64_t>>* items) {
  constexpr uint64_t OPEN = 1ull << 32;   // (above every field number)
  auto number = [](const char*& p, uint64_t* v) {   // 1 to 10 digits, 1 to 2^32 - 1
    const char* b = p;
    uint64_t x = 0;
    while (*p >= '0' && *p <= '9' && p - b <= 10) x = x * 10 + (uint64_t)(*p++ - '0');
    *v = x;
    return p > b && p - b <= 10 && x >= 1 && x <= 0xFFFFFFFFull;
  };
  const char* p = text;
  for (;;) {
    uint64_t a = 0, b = 0;
    if (*p == '-') return "there is no -B form: a range starts with a number";
    if (!number(p, &a)) return "a field is a number from 1 to 4294967295";
    b = a;
    if (*p == '-') {
      ++p;
      if (*p == ',' || !*p) b = OPEN;
      else if (!number(p, &b)) return "a field is a number from 1 to 4294967295";
      else if (b < a) return "a range A-B needs A <= B";
    }
    items->emplace_back(a, b);
    if (!*p) break;
    if (*p != ',') return "items are K, A-B or A-, joined by commas";
    ++p;
  }
  return nullptr;
}

// items (taken by value: sorted here) -> out[0, *n), the normal form of their union.  Returns null, or what is wrong.
inline const char* kxNormalFieldItems(std::vector<std::pair<uint64_t, uint64_t>> items, kx_field_range out[KX_FIELD_RANGES], uint32_t* n) {
  constexpr uint64_t OPEN = 1ull << 32;
  *n = 0;
  std::sort(items.begin(), items.end());
  std::vector<std::pair<uint64_t, uint64_t>> norm;
  for (const auto& it : items) {
    if (!norm.empty() && it.first <= norm.back().second + 1) norm.back().second = std::max(norm.back().second, it.second);
    else norm.push_back(it);
  }
  if (norm.size() > KX_FIELD_RANGES) return "more than 8 ranges in its normal form";
  for (const auto& r : norm) out[(*n)++] = kx_field_range{(uint32_t)r.first, r.second == OPEN ? 0u : (uint32_t)r.second};
  return nullptr;
}

// text -> out[0, *n), the normal form.  Returns null, or what is wrong with the text (a static string).
inline const char* kxParseFieldList(const char* text, kx_field_range out[KX_FIELD_RANGES], uint32_t* n) {
  *n = 0;
  std::vector<std::pair<uint64_t, uint64_t>> items;
  if (const char* why = kxParseFieldItems(text, &items)) return why;
  return kxNormalFieldItems(std::move(items), out, n);
}

// the items a kx_field_project must hold: 1 to 16 of them, lo >= 1, hi == 0 (open) or hi >= lo
inline bool kxFieldItemsAreValid(const kx_field_range* it, uint32_t n) {
  if (n < 1 || n > KX_FIELD_ITEMS) return false;
  for (uint32_t j = 0; j < n; ++j) if (it[j].lo < 1 || (it[j].hi != 0 && it[j].hi < it[j].lo)) return false;
  return true;
}

// valid items -> out[0, *n), the normal form of their union: the selected set of a projection.  Returns null, or what is wrong.
inline const char* kxFieldItemsUnion(const kx_field_range* it, uint32_t n_items, kx_field_range out[KX_FIELD_RANGES], uint32_t* n) {
  std::vector<std::pair<uint64_t, uint64_t>> items;
  for (uint32_t j = 0; j < n_items; ++j) items.emplace_back(it[j].lo, it[j].hi == 0 ? 1ull << 32 : (uint64_t)it[j].hi);
  return kxNormalFieldItems(std::move(items), out, n);
}

// the list of `--field=LIST --only`: text -> items[0, *n_items) as written — in any order, overlapping, repeated — and
// out[0, *n), the normal form of their union.  Returns null, or what is wrong with the text (a static string).
inline const char* kxParseFieldOrder(const char* text, kx_field_range items[KX_FIELD_ITEMS], uint32_t* n_items,
                                     kx_field_range out[KX_FIELD_RANGES], uint32_t* n) {
  *n_items = *n = 0;
  std::vector<std::pair<uint64_t, uint64_t>> parsed;
  if (const char* why = kxParseFieldItems(text, &parsed)) return why;
  if (parsed.size() > KX_FIELD_ITEMS) return "more than 16 items with --only";
  for (const auto& it : parsed) items[(*n_items)++] = kx_field_range{(uint32_t)it.first, it.second == 1ull << 32 ? 0u : (uint32_t)it.second};
  return kxNormalFieldItems(std::move(parsed), out, n);
}
