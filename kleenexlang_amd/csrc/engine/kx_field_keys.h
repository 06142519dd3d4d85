// kx_field_keys.h — `--keys[=C]` and the NAMES of its `--field=LIST`: the parser of a list of keys, and the byte rules a key
// separator and a name obey.  Host code beside kx_field_names.h, whose name spelling it shares: kxrun.cpp parses the option text
// with it before the engine library is loaded, and the library applies the same byte rules to a kx_field_keys
// (kx_field_keys_host.inc).  The Python restatement is host.parse_field_keys.
//
// LIST = item (',' item)*, cut at the commas that no backslash takes with it.  Every item is a NAME, an all-digits item too: its
// bytes spelled as themselves or as \n \t \r \0 \\ \, \xHH, 1 to 255 of them.  A last `?` that no backslash takes with it is no
// byte of the name: it makes the item OPTIONAL (a literal last `?` is spelled \x3F).  At most KX_FIELD_ITEMS items; items may
// repeat.  The DISTINCT names are numbered in the order of their first item; a name is optional if every item that names it is.
#pragma once

#include <string>
#include <vector>

#include "kx_field_names.h"

struct KxFieldKeys {
  std::vector<std::string> names;   // the distinct names, in the order of their first item
  uint32_t optional_mask = 0;       // bit t: every item that names names[t] ends in `?`
  std::vector<uint32_t> items;      // the items as written, as indices into names
};

// the text's items.  Returns null, or what is wrong with the text (a static string).
inline const char* kxParseFieldKeys(const char* text, KxFieldKeys* out) {
  auto hex = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
  static const char* const bad_escape = "a backslash in a name starts \\n \\t \\r \\0 \\\\ \\, or \\xHH";
  out->names.clear(); out->items.clear(); out->optional_mask = 0;
  uint32_t required = 0;
  const char* p = text;
  for (;;) {
    const char* b = p;
    bool taken = false;                       // the character before p was taken by a backslash
    while (*p && *p != ',') { taken = *p == '\\' && p[1]; if (taken) ++p; ++p; }
    const char* e = p;
    const bool optional = e > b && e[-1] == '?' && !taken;
    if (optional) --e;
    std::string name;
    for (const char* q = b; q < e;) {
      if (*q != '\\') { name.push_back(*q++); continue; }
      if (q + 1 >= e) return bad_escape;
      switch (q[1]) {
        case 'n': name.push_back('\n'); q += 2; break;
        case 't': name.push_back('\t'); q += 2; break;
        case 'r': name.push_back('\r'); q += 2; break;
        case '0': name.push_back('\0'); q += 2; break;
        case '\\': name.push_back('\\'); q += 2; break;
        case ',': name.push_back(','); q += 2; break;
        case 'x':
          if (q + 3 >= e || hex(q[2]) < 0 || hex(q[3]) < 0) return bad_escape;
          name.push_back((char)(hex(q[2]) * 16 + hex(q[3])));
          q += 4;
          break;
        default: return bad_escape;
      }
    }
    if (name.empty()) return "an empty name";
    if (name.size() > KX_FIELD_NAME_MAX) return "a name has at most 255 bytes";
    if (out->items.size() == KX_FIELD_ITEMS) return "more than 16 items";
    uint32_t t = 0;
    while (t < out->names.size() && out->names[t] != name) ++t;
    if (t == out->names.size()) out->names.push_back(name);
    out->items.push_back(t);
    if (!optional) required |= 1u << t;
    if (!*p) break;
    ++p;
  }
  out->optional_mask = ((1u << out->names.size()) - 1u) & ~required;
  return nullptr;
}

// the byte rules of a key separator `kv` beside the framing's bytes — fs (-1 with `words`), the one-byte record separator (-1: it
// has more bytes, or the caller has none), quote and escape (-1: none).  Returns null, or which byte it clashes with.
inline const char* kxFieldKeyByteClash(int kv, int fs, bool words, int rsep, int quote, int escape) {
  if (!words && kv == fs) return "the field separator";
  if (words && (kv == 0x20 || kv == 0x09)) return "a blank";
  if (kv == rsep) return "the record separator";
  if (quote >= 0 && kv == quote) return "the quote character";
  if (escape >= 0 && kv == escape) return "the escape character";
  return nullptr;
}

// a name can be a field's key: it holds no kv byte, no fs byte (with `words`: no blank) and not the one-byte record separator.
// Returns null, or which byte it holds.
inline const char* kxFieldKeyNameClash(const uint8_t* name, size_t n, int kv, int fs, bool words, int rsep) {
  for (size_t k = 0; k < n; ++k) {
    const int b = name[k];
    if (b == kv) return "the key separator";
    if (words ? (b == 0x20 || b == 0x09) : b == fs) return words ? "a blank" : "the field separator";
    if (b == rsep) return "the record separator";
  }
  return nullptr;
}
