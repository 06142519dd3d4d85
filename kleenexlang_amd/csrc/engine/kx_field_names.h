// kx_field_names.h — `--header[=N]` and the NAMES of `--field=LIST`: the parser of a list that may hold names, the cutter of a
// header record's cells and the resolver that turns names into field numbers.  Host code beside kx_field_list.h, whose item parser
// and normaliser it builds on: kxrun.cpp parses the option text with it before the engine library is loaded, and the library cuts
// and resolves with it when header record N is in hand (kx_records_host.inc).  The Python restatements are host.parse_field_names,
// host.header_names_model and host.resolve_field_names.
//
// LIST = item (',' item)*, cut at the commas that no backslash takes with it (a backslash always takes the next character).  An
// item made only of digits and '-' is a NUMBER item, kx_field_list.h's K | A-B | A- with its refusals.  Every other item is a
// NAME: its bytes spelled as themselves or as \n \t \r \0 \\ \, \xHH, 1 to 255 of them.  A list that holds a name has at most
// KX_FIELD_ITEMS items.
//
// The CELLS of a header record's body lie between its live `fs` bytes — every one; with a quote byte those at even parity of the
// quote bytes before them; with an escape byte those that are unescaped and at even parity of the unescaped quotes — or, with
// `words`, are the maximal runs of bytes that are no live blanks.  A cell's NAME is its bytes; with a quote or an escape byte it is
// the cell's value (host.unquote_field_model).  With `first` (the record is the stream's first) a leading EF BB BF is no part of
// the first cell.  A name selects the lowest-numbered cell that has it.
#pragma once

#include <string>

#include "kx_field_list.h"

constexpr size_t KX_FIELD_NAME_MAX = 255;

struct KxFieldNameItem {
  bool is_name = false;
  uint64_t lo = 0, hi = 0;   // a number item: (A, B) with B = 2^32 for an open one, as kxParseFieldItems gives it
  std::string name;          // a name item: its decoded bytes
};

// the text holds an item that is no number item: a character that is neither a digit, a '-' nor a cutting comma
inline bool kxFieldTextHasName(const char* text) {
  for (const char* p = text; *p; ++p) if (!((*p >= '0' && *p <= '9') || *p == '-' || *p == ',')) return true;
  return false;
}

// the text's items as written.  Returns null, or what is wrong with the text (a static string).
inline const char* kxParseFieldNames(const char* text, std::vector<KxFieldNameItem>* items) {
  auto hex = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
  bool named = false;
  const char* p = text;
  for (;;) {
    const char* b = p;
    while (*p && *p != ',') { if (*p == '\\' && p[1]) ++p; ++p; }
    bool number = true;
    for (const char* q = b; q < p; ++q) if (!((*q >= '0' && *q <= '9') || *q == '-')) number = false;
    KxFieldNameItem it;
    if (number) {
      const std::string s(b, p);
      std::vector<std::pair<uint64_t, uint64_t>> one;
      if (const char* why = kxParseFieldItems(s.c_str(), &one)) return why;
      it.lo = one[0].first; it.hi = one[0].second;
    } else {
      it.is_name = named = true;
      for (const char* q = b; q < p;) {
        if (*q != '\\') { it.name.push_back(*q++); continue; }
        if (q + 1 >= p) return "a backslash in a name starts \\n \\t \\r \\0 \\\\ \\, or \\xHH";
        switch (q[1]) {
          case 'n': it.name.push_back('\n'); q += 2; break;
          case 't': it.name.push_back('\t'); q += 2; break;
          case 'r': it.name.push_back('\r'); q += 2; break;
          case '0': it.name.push_back('\0'); q += 2; break;
          case '\\': it.name.push_back('\\'); q += 2; break;
          case ',': it.name.push_back(','); q += 2; break;
          case 'x':
            if (q + 3 >= p || hex(q[2]) < 0 || hex(q[3]) < 0) return "a backslash in a name starts \\n \\t \\r \\0 \\\\ \\, or \\xHH";
            it.name.push_back((char)(hex(q[2]) * 16 + hex(q[3])));
            q += 4;
            break;
          default: return "a backslash in a name starts \\n \\t \\r \\0 \\\\ \\, or \\xHH";
        }
      }
      if (it.name.size() > KX_FIELD_NAME_MAX) return "a name has at most 255 bytes";
    }
    items->push_back(std::move(it));
    if (!*p) break;
    ++p;
  }
  if (named && items->size() > KX_FIELD_ITEMS) return "more than 16 items in a list with a name";
  return nullptr;
}

// the value of a cell spelled raw[0, n): host.unquote_field_model (quote, escape: a byte value, or -1 for none)
inline std::string kxUnquoteCell(const uint8_t* raw, size_t n, int quote, int escape) {
  std::string out;
  bool inq = false, pc = false;   // inside quotes; the previous byte was a closing quote
  for (size_t i = 0; i < n;) {
    const int b = raw[i];
    if (escape >= 0 && b == escape) {
      if (i + 1 < n) out.push_back((char)raw[i + 1]);
      i += 2;
      pc = false;
      continue;
    }
    if (quote >= 0 && b == quote) {
      if (inq) { inq = false; pc = true; }
      else { inq = true; if (pc) out.push_back((char)quote); pc = false; }
      ++i;
      continue;
    }
    out.push_back((char)b);
    pc = false;
    ++i;
  }
  return out;
}

// the names of the cells of the header record body[0, n), in cell order (fs is not used with `words`)
inline void kxHeaderCellNames(const uint8_t* body, size_t n, uint8_t fs, int quote, int escape, bool words, bool first,
                              std::vector<std::string>* cells) {
  cells->clear();
  if (first && n >= 3 && body[0] == 0xEF && body[1] == 0xBB && body[2] == 0xBF) { body += 3; n -= 3; }
  const bool values = quote >= 0 || escape >= 0;
  auto cell = [&](size_t b, size_t e) {
    cells->push_back(values ? kxUnquoteCell(body + b, e - b, quote, escape) : std::string((const char*)body + b, e - b));
  };
  bool esc = false, parity = false, in_word = false;
  size_t begin = 0;
  for (size_t k = 0; k < n; ++k) {
    const int b = body[k];
    bool live = false;   // a live field separator, or with `words` a live blank
    if (esc) esc = false;
    else if (escape >= 0 && b == escape) esc = true;
    else if (quote >= 0 && b == quote) parity = !parity;
    else if (!parity) live = words ? (b == 0x20 || b == 0x09) : b == fs;
    if (words) {
      if (!live && !in_word) { in_word = true; begin = k; }
      else if (live && in_word) { in_word = false; cell(begin, k); }
    } else if (live) {
      cell(begin, k);
      begin = k + 1;
    }
  }
  if (words ? in_word : true) cell(begin, n);
}

// items[0, n_items) with names — lo >= 1: a number item (hi = 0: open); lo == 0: the name names[hi] — against the cells' names:
// out_items[0, n_items) the items as numbers, in the written order, and ranges[0, *n_ranges) the normal form of their union.
// Returns 0; 1 with *missing = the index of a name no cell has; 2 if the union has more than 8 ranges.
inline int kxResolveFieldNames(const kx_field_range* items, uint32_t n_items, const std::vector<std::string>& names,
                               const std::vector<std::string>& cells, kx_field_range* out_items, kx_field_range ranges[KX_FIELD_RANGES],
                               uint32_t* n_ranges, uint32_t* missing) {
  *n_ranges = 0; *missing = 0;
  for (uint32_t j = 0; j < n_items; ++j) {
    if (items[j].lo) { out_items[j] = items[j]; continue; }
    const std::string& name = names[items[j].hi];
    size_t c = 0;
    while (c < cells.size() && cells[c] != name) ++c;
    if (c == cells.size()) { *missing = items[j].hi; return 1; }
    out_items[j] = kx_field_range{(uint32_t)(c + 1), (uint32_t)(c + 1)};
  }
  return kxFieldItemsUnion(out_items, n_items, ranges, n_ranges) ? 2 : 0;
}

// a name for a message: its bytes, the non-printable ones as \xHH
inline std::string kxPrintableName(const std::string& name) {
  static const char* const digits = "0123456789ABCDEF";
  std::string s;
  for (const unsigned char c : name) {
    if (c >= 0x20 && c < 0x7F) s.push_back((char)c);
    else { s += "\\x"; s.push_back(digits[c >> 4]); s.push_back(digits[c & 15]); }
  }
  return s;
}
