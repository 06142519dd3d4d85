// field_keys.cpp — the parser of `--field=LIST --keys` (kx_field_keys.h) and the two lane bodies of the keyed selection
// (kx_field_keys_lanes.h: kv_count_lane, kv_locate_lane; the kernels k_kvcount and k_kvlocate are grid-stride loops around them) run
// one lane at a time on the host and compared with a plain byte loop written here.  Built with -fsanitize=address,undefined by
// tests/test_records_keys.py.  Every body lies in an allocation of exactly the aligned 16-byte granules that hold one of its bytes
// (the lanes load whole granules: the sanitizer sees a load of any other), at each of the 16 start residues, and every output
// array has exactly the size the lanes may touch.
//
//   field_keys      exit 0: every case equal and every listed population seen
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../include/kxhip.h"
#include "../../kleenexlang_amd/csrc/engine/kx_field_keys.h"
#include "../../kleenexlang_amd/csrc/engine/kx_field_keys_lanes.h"

typedef unsigned long long u64;

namespace {

std::set<std::string> seen;

int fail(const char* what, const std::string& body, int mode, bool words, unsigned res, const char* list) {
  fprintf(stderr, "%s: body \"%s\" mode %d words %d residue %u list %s\n", what, body.c_str(), mode, (int)words, res, list);
  return 1;
}

// ---------------------------------------------------------------------------------------------------------------- the parser
int parser() {
  KxFieldKeys k;
  auto ok = [&](const char* text) { return kxParseFieldKeys(text, &k) == nullptr; };
  if (!ok("a") || k.names != std::vector<std::string>{"a"} || k.optional_mask != 0 || k.items != std::vector<uint32_t>{0}) return 1;
  if (!ok("ts,msg?") || k.names != std::vector<std::string>{"ts", "msg"} || k.optional_mask != 2 || k.items != std::vector<uint32_t>{0, 1}) return 2;
  if (!ok("b?,a?") || k.names != std::vector<std::string>{"b", "a"} || k.optional_mask != 3) return 3;
  if (!ok("200") || k.names != std::vector<std::string>{"200"}) return 4;                      // an all-digits item is a name
  if (!ok("a\\x3F") || k.names != std::vector<std::string>{"a?"} || k.optional_mask != 0) return 5;
  if (!ok("a\\x3F?") || k.names != std::vector<std::string>{"a?"} || k.optional_mask != 1) return 6;
  if (!ok("a\\,b,\\\\?") || k.names != std::vector<std::string>{"a,b", "\\"} || k.optional_mask != 2) return 7;
  if (!ok("m,a,m?,a") || k.names != std::vector<std::string>{"m", "a"} || k.optional_mask != 0 || k.items != std::vector<uint32_t>{0, 1, 0, 1}) return 8;
  if (!ok("m?,m?") || k.optional_mask != 1 || k.items.size() != 2) return 9;
  if (!ok("\\n\\t\\r\\0\\x41") || k.names[0] != std::string("\n\t\r\0A", 5)) return 10;
  for (const char* bad : {"", "?", "a,,b", "a,", ",a", "a\\", "a\\q", "a\\x4", "a\\x4g", "a,?"}) if (ok(bad)) { fprintf(stderr, "parsed: %s\n", bad); return 11; }
  std::string sixteen, seventeen;
  for (int i = 0; i < 17; ++i) { if (i == 16) sixteen = seventeen; seventeen += std::string(i ? "," : "") + "k" + std::to_string(i); }
  if (!ok(sixteen.c_str()) || k.names.size() != 16 || ok(seventeen.c_str())) return 12;
  if (!ok(std::string(255, 'n').c_str()) || ok(std::string(256, 'n').c_str()) || !ok((std::string(255, 'n') + "?").c_str())) return 13;
  if (kxFieldKeyByteClash('=', ',', false, '\n', '"', -1) || !kxFieldKeyByteClash(',', ',', false, '\n', -1, -1) || !kxFieldKeyByteClash(' ', -1, true, '\n', -1, -1) ||
      !kxFieldKeyByteClash('\n', ',', false, '\n', -1, -1) || !kxFieldKeyByteClash('"', ',', false, '\n', '"', -1) || !kxFieldKeyByteClash('\\', ',', false, '\n', -1, '\\') ||
      kxFieldKeyByteClash(' ', ',', false, '\n', -1, -1))
    return 14;
  const uint8_t nm[3] = {'a', '=', 'b'};
  if (!kxFieldKeyNameClash(nm, 3, '=', ',', false, '\n') || kxFieldKeyNameClash(nm, 1, '=', ',', false, '\n') || !kxFieldKeyNameClash(nm, 3, ':', '=', false, '\n') ||
      !kxFieldKeyNameClash((const uint8_t*)"a b", 3, '=', -1, true, '\n') || !kxFieldKeyNameClash((const uint8_t*)"a\n", 2, '=', ',', false, '\n'))
    return 15;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the lanes
struct Doc { u64 vb, fe; uint32_t t; };

// the plain reference: the names found and the documents of body (at offset s of the buffer), byte by byte
uint32_t reference(const std::string& body, u64 s, int mode, bool words, int fs, int quote, int escape, int kv, const KxFieldKeys& K, std::vector<Doc>* docs) {
  const size_t n = body.size();
  std::vector<char> lsep(n, 0), lkv(n, 0);
  bool esc = false, parity = false;
  for (size_t k = 0; k < n; ++k) {
    const int b = (unsigned char)body[k];
    if (mode == KV_ESCAPED && esc) esc = false;
    else if (mode == KV_ESCAPED && b == escape) esc = true;
    else if (mode != KV_PLAIN && b == quote) parity = !parity;
    else if (!parity) {
      if (words ? (b == ' ' || b == '\t') : b == fs) lsep[k] = 1;
      else if (b == kv) lkv[k] = 1;
    }
  }
  std::vector<std::pair<size_t, size_t>> fields;
  if (words) {
    for (size_t k = 0; k < n;) {
      if (lsep[k]) { ++k; continue; }
      size_t e = k;
      while (e < n && !lsep[e]) ++e;
      fields.emplace_back(k, e);
      k = e;
    }
  } else {
    size_t b = 0;
    for (size_t k = 0; k <= n; ++k) if (k == n || lsep[k]) { fields.emplace_back(b, k); b = k + 1; }
  }
  uint32_t found = 0;
  docs->clear();
  for (const auto& f : fields) {
    size_t c = f.first;
    while (c < f.second && !lkv[c]) ++c;
    if (c == f.second || c == f.first) continue;                // no live C, or an empty key
    const std::string key = body.substr(f.first, c - f.first);
    for (uint32_t t = 0; t < K.names.size(); ++t)
      if (!((found >> t) & 1u) && K.names[t] == key) { found |= 1u << t; docs->push_back(Doc{s + c + 1, s + f.second, t}); }
  }
  return found;
}

template <int MODE, bool WORDS>
int one(const std::string& body, unsigned res, const KVBytes& B, const KVSpec& V, const KxFieldKeys& K, const char* list) {
  const size_t gran = (res + body.size() + 15) / 16 * 16;
  uint8_t* buf = (uint8_t*)aligned_alloc(16, gran ? gran : 16);
  memset(buf, B.kv, gran ? gran : 16);                          // (bytes outside the body that would count if they were read as its own)
  memcpy(buf + res, body.data(), body.size());
  std::vector<Doc> want;
  const uint32_t wfound = reference(body, res, MODE, WORDS, (int)B.fs, (int)B.quote, (int)B.escape, (int)B.kv, K, &want);
  const bool missing = (wfound & V.req) != V.req;
  int rc = 0;
  u64 found = 99;
  const u64 nd = kv_count_lane<MODE, WORDS>(buf, res, res + body.size(), B, V, &found);
  if (found != wfound) rc = fail("k_kvcount: the names found differ", body, MODE, WORDS, res, list);
  else if (nd != (missing ? 0 : want.size())) rc = fail("k_kvcount: the number of documents differs", body, MODE, WORDS, res, list);
  if (!rc && nd) {
    const u64 da = 3;                                           // the record's first document is not the call's first
    u64* fb = new u64[da + nd]; u64* fe = new u64[da + nd]; u64* dlen = new u64[2 * (da + nd)];
    uint8_t* dkey = new uint8_t[da + nd];
    uint8_t* krow = (uint8_t*)aligned_alloc(16, 16);
    for (u64 d = 0; d < da + nd; ++d) { fb[d] = fe[d] = dlen[2 * d] = dlen[2 * d + 1] = 77; dkey[d] = 77; }
    memset(krow, 0x55, 16);
    kv_locate_lane<MODE, WORDS>(buf, res, res + body.size(), B, V, da, fb, fe, dlen, dkey, krow);
    uint8_t wrow[16];
    memset(wrow, 0xFF, 16);
    for (u64 d = 0; d < nd && !rc; ++d) {
      wrow[want[d].t] = (uint8_t)d;
      if (fb[da + d] != want[d].vb || fe[da + d] != want[d].fe || dlen[2 * (da + d)] != want[d].fe - want[d].vb || dlen[2 * (da + d) + 1] != 0 ||
          dkey[da + d] != want[d].t)
        rc = fail("k_kvlocate: a document differs", body, MODE, WORDS, res, list);
    }
    for (u64 d = 0; d < da && !rc; ++d)
      if (fb[d] != 77 || fe[d] != 77 || dlen[2 * d] != 77 || dkey[d] != 77) rc = fail("k_kvlocate: a document of another record was written", body, MODE, WORDS, res, list);
    if (!rc && memcmp(krow, wrow, 16) != 0) rc = fail("k_kvlocate: the record's row of kdoc differs", body, MODE, WORDS, res, list);
    if (!rc) {                                                  // once more without the row
      kv_locate_lane<MODE, WORDS>(buf, res, res + body.size(), B, V, da, fb, fe, dlen, dkey, nullptr);
      if (fb[da] != want[0].vb) rc = fail("k_kvlocate without a row differs", body, MODE, WORDS, res, list);
    }
    delete[] fb; delete[] fe; delete[] dlen; delete[] dkey; free(krow);
    seen.insert("documents " + std::to_string(nd > 2 ? 2 : nd));
    for (const Doc& d : want) { if (d.vb == d.fe) seen.insert("empty value"); if (d.fe == res + body.size()) seen.insert("value to the body's end"); }
    if (want.size() == 2 && want[0].t > want[1].t) seen.insert("record order is not list order");
  } else if (!rc) {
    seen.insert(missing ? "required name missing" : "no name, none required");
  }
  free(buf);
  return rc;
}

int sweep(const char* alphabet, unsigned maxlen, int mode, bool words, const KVBytes& B, const char* list) {
  KxFieldKeys K;
  if (kxParseFieldKeys(list, &K)) return 1;
  uint8_t* tab = (uint8_t*)aligned_alloc(16, 64 + 16 * 255 + 16);
  memset(tab, 0, 64 + 16 * 255 + 16);
  uint16_t* tl = (uint16_t*)tab;
  uint32_t at = 0;
  for (uint32_t t = 0; t < K.names.size(); ++t) {
    tl[t] = (uint16_t)K.names[t].size(); tl[16 + t] = (uint16_t)at;
    memcpy(tab + 64 + at, K.names[t].data(), K.names[t].size());
    at += (uint32_t)K.names[t].size();
  }
  KVSpec V{tab, nullptr, nullptr, (1u << K.names.size()) - 1u, 0u, B.kv};
  V.req = V.all & ~K.optional_mask;
  const size_t na = strlen(alphabet);
  int rc = 0;
  for (unsigned len = 0; len <= maxlen && !rc; ++len) {
    size_t count = 1;
    for (unsigned k = 0; k < len; ++k) count *= na;
    for (size_t c = 0; c < count && !rc; ++c) {
      std::string body(len, ' ');
      size_t x = c;
      for (unsigned k = 0; k < len; ++k) { body[k] = alphabet[x % na]; x /= na; }
      for (unsigned res = 0; res < 16 && !rc; ++res) {
        rc = mode == KV_PLAIN ? (words ? one<KV_PLAIN, true>(body, res, B, V, K, list) : one<KV_PLAIN, false>(body, res, B, V, K, list))
           : mode == KV_QUOTED ? (words ? one<KV_QUOTED, true>(body, res, B, V, K, list) : one<KV_QUOTED, false>(body, res, B, V, K, list))
                               : (words ? one<KV_ESCAPED, true>(body, res, B, V, K, list) : one<KV_ESCAPED, false>(body, res, B, V, K, list));
      }
    }
  }
  free(tab);
  return rc;
}

// a key as long as a name can be, across many granules, with near misses in front of it
int long_keys() {
  for (unsigned klen : {1u, 15u, 16u, 17u, 31u, 32u, 33u, 255u}) {
    std::string name(klen, 'k');
    for (unsigned k = 0; k < klen; ++k) name[k] = (char)('a' + k % 23);
    std::string last = name, first = name;
    last[klen - 1] = 'Z'; first[0] = 'Z';
    const std::string body = last + "=1," + first + "=2," + name.substr(0, klen - 1) + "=3," + name + "x=4," + name + "=5," + name + "=6";
    for (unsigned res = 0; res < 16; ++res)
      for (int words = 0; words < 2; ++words) {
        std::string b = body;
        if (words) for (char& ch : b) if (ch == ',') ch = ' ';
        KxFieldKeys K;
        K.names = {name}; K.items = {0};
        uint8_t* tab = (uint8_t*)aligned_alloc(16, 64 + 256);
        memset(tab, 0, 64 + 256);
        ((uint16_t*)tab)[0] = (uint16_t)klen;
        memcpy(tab + 64, name.data(), klen);
        const KVSpec V{tab, nullptr, nullptr, 1u, 1u, '='};
        const KVBytes B{',', 256u, 256u, '='};
        const int rc = words ? one<KV_PLAIN, true>(b, res, B, V, K, "long") : one<KV_PLAIN, false>(b, res, B, V, K, "long");
        free(tab);
        if (rc) return rc;
      }
  }
  return 0;
}

}  // namespace

int main() {
  if (const int rc = parser()) { fprintf(stderr, "the parser: check %d failed\n", rc); return 1; }
  unsigned sweeps = 0;
  for (const char* list : {"a", "ab", "a,b?", "b?,a?"})
    for (int words = 0; words < 2; ++words) {
      // every body over {a, b, C, F} of length 0 to 7, under each framing (no quote or escape byte in them: the state never moves)
      const char* plain = words ? "ab= " : "ab=,";
      for (int mode : {KV_PLAIN, KV_QUOTED, KV_ESCAPED}) {
        const KVBytes B{words ? 0u : (uint32_t)',', mode == KV_PLAIN ? 256u : (uint32_t)'"', mode == KV_ESCAPED ? (uint32_t)'\\' : 256u, '='};
        if (sweep(plain, 7, mode, words != 0, B, list)) return 1;
        ++sweeps;
      }
      // and the bodies of length 0 to 6 in which the state moves: a quote, an escape, with WORDS the tab
      const KVBytes Q{words ? 0u : (uint32_t)',', '"', 256u, '='}, E{words ? 0u : (uint32_t)',', '"', '\\', '='}, E1{words ? 0u : (uint32_t)',', 256u, '\\', '='};
      if (sweep(words ? "a= \"" : "a=,\"", 6, KV_QUOTED, words != 0, Q, list)) return 1;
      if (sweep(words ? "a= \"\\" : "a=,\"\\", 5, KV_ESCAPED, words != 0, E, list)) return 1;
      if (sweep(words ? "a=\t\\" : "a=,\\", 6, KV_ESCAPED, words != 0, E1, list)) return 1;
      sweeps += 3;
    }
  if (long_keys()) return 1;
  int missing = 0;
  for (const char* w : {"documents 1", "documents 2", "required name missing", "no name, none required", "empty value", "value to the body's end",
                        "record order is not list order"})
    if (!seen.count(w)) { fprintf(stderr, "never seen: %s\n", w); ++missing; }
  if (missing) return 1;
  printf("field_keys: %u sweeps, every lane equal\n", sweeps);
  return 0;
}
