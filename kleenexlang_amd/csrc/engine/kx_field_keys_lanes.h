// kx_field_keys_lanes.h — per-lane bodies of the keyed selection (`--keys`; the kernels k_kvcount and k_kvlocate in
// kx_field_keys.inc are thin grid-stride loops over kv_count_lane and kv_locate_lane) that also compile as plain C++, as
// kx_field_lanes.h does: tests/native/field_keys.cpp runs the same text one lane at a time under a sanitizer.  Needs
// kx_batch_doc (include/kxhip.h) from the including file; reads no other engine type.
//
// A lane is a record.  It walks the aligned 16-byte granules that hold a byte of its body [s, be) of `in`, one 16-byte load each
// (an empty body loads nothing), and sees a granule through kv_masks: three 16-bit masks, bit p for the granule's byte p — the
// live field separators (WORDS: the live blanks), the live key separators C, and the bytes of the body.  LIVE is kx_fields.inc's
// rule for an F byte, for all of them: every one (KV_PLAIN); one at even parity of the quote bytes before it in the record
// (KV_QUOTED); an unescaped one at even parity of the record's unescaped quotes (KV_ESCAPED).  The events of the walk, in address
// order: a field begins (behind a live F or at the body's start; WORDS: a word's first byte), a field's FIRST live C — its key is
// the bytes from the field's begin to it, its value what follows — and a field ends (a live F, the first byte behind a word, the
// body's end).  A key is compared, byte by byte, only with the listed names of its length that the record has not had yet: the
// first field with a key wins, later ones are bytes like any other.  A granule without a live C, met while no document is open,
// moves the field's begin and nothing else.  The walk ends once every name is found and the last document is closed.
#pragma once

#include <cstring>

#include "kx_field_lanes.h"

enum { KV_PLAIN = 0, KV_QUOTED = 1, KV_ESCAPED = 2 };   // (kx_fields.inc's FLD_* values)

// the bytes the masks are made of: fs (not with WORDS), quote and escape (256: none), and C
struct KVBytes { uint32_t fs, quote, escape, kv; };

// 0x80 in every byte of x that is 0 (k_rcount's exact test), and the four high bits of such a word as bits 0 to 3
KX_LANE uint32_t kv_zero(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); }
KX_LANE uint32_t kv_pack(uint32_t m) { return (((m >> 7) & 0x01010101u) * 0x01020408u) >> 24; }

// the granule at g: sep = its live field separators (WORDS: live blanks), cm = its live C bytes, inb = its bytes of the body
// [pa, pe).  KV_PLAIN: two zero-byte tests per word (WORDS: three), no state; else byte by byte with the two-bit state.
template <int MODE, bool WORDS>
KX_LANE void kv_masks(uintptr_t g, uintptr_t pa, uintptr_t pe, const KVBytes& B, uint32_t& parity, uint32_t& esc, uint32_t& sep, uint32_t& cm,
                      uint32_t& inb) {
  uint32_t w[4];
#ifdef __HIPCC__
  const uint4 v = *reinterpret_cast<const uint4*>(g);
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
#else
  memcpy(w, reinterpret_cast<const void*>(g), 16);
#endif
  const uint32_t lo = pa > g ? (uint32_t)(pa - g) : 0u, hi = pe - g < 16 ? (uint32_t)(pe - g) : 16u;
  inb = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
  sep = cm = 0;
  if (MODE == KV_PLAIN) {
    const uint32_t pc = 0x01010101u * B.kv, pf = 0x01010101u * B.fs;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t f = WORDS ? kv_zero(w[k] ^ 0x20202020u) | kv_zero(w[k] ^ 0x09090909u) : kv_zero(w[k] ^ pf);
      sep |= kv_pack(f) << (4 * k);
      cm |= kv_pack(kv_zero(w[k] ^ pc)) << (4 * k);
    }
    sep &= inb; cm &= inb;
  } else {
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      if (!((inb >> p) & 1u)) continue;
      const uint32_t ch = (w[p >> 2] >> (8 * (p & 3))) & 0xFFu;
      if (MODE == KV_ESCAPED && esc) esc = 0;                   // an escaped byte is only data
      else if (MODE == KV_ESCAPED && ch == B.escape) esc = 1;
      else if (ch == B.quote) parity ^= 1u;
      else if (parity == 0) {
        if (WORDS ? (ch == 0x20u || ch == 0x09u) : ch == B.fs) sep |= 1u << p;
        else if (ch == B.kv) cm |= 1u << p;
      }
    }
  }
}

// the listed name, not in `found`, that in[kb, kb + klen) spells; 16: none
KX_LANE uint32_t kv_match(const uint8_t* __restrict__ in, unsigned long long kb, unsigned long long klen, const KVSpec& V, uint32_t found) {
  if (klen == 0 || klen > 255) return 16;
  const uint16_t* const tl = reinterpret_cast<const uint16_t*>(V.tab);
  for (uint32_t cand = V.all & ~found; cand; cand &= cand - 1) {
    const uint32_t t = (uint32_t)__builtin_ctz(cand);
    if (tl[t] != klen) continue;
    const uint8_t* const nm = V.tab + 64 + tl[16 + t];
    unsigned long long k = 0;
    while (k < klen && in[kb + k] == nm[k]) ++k;
    if (k == klen) return t;
  }
  return 16;
}

// The walk of the body in[s, be).  Returns the mask of the names found.  With LOCATE the documents are written from number d on, in
// address order: fb[d] = the value's begin, fe[d] = the field's end, dlen[2 d] = their difference and dlen[2 d + 1] = 0 (a 16-byte
// length record), dkey[d] = the name's index, and with krow (the record's 16 bytes of kdoc, all 0xFF before) krow[index] = the
// document's number in the record.
template <int MODE, bool WORDS, bool LOCATE>
KX_LANE uint32_t kv_walk(const uint8_t* __restrict__ in, unsigned long long s, unsigned long long be, const KVBytes& B, const KVSpec& V,
                         unsigned long long d, unsigned long long* __restrict__ fb, unsigned long long* __restrict__ fe,
                         unsigned long long* __restrict__ dlen, uint8_t* __restrict__ dkey, uint8_t* __restrict__ krow) {
  const uintptr_t base = (uintptr_t)in, pa = base + s, pe = base + be;
  const unsigned long long dfirst = d;
  uint32_t found = 0, parity = 0, esc = 0, carry = 0;           // carry (WORDS): the byte before the granule is a word's
  bool has_c = false, open = false;                             // the field has had its first live C; it is document d, not ended
  unsigned long long fbeg = s, cb = s;                          // the field's begin; the open document's
  for (uintptr_t g = pa < pe ? pa & ~(uintptr_t)15 : pe; g < pe && (open || found != V.all); g += 16) {
    uint32_t sep, cm, inb;
    kv_masks<MODE, WORDS>(g, pa, pe, B, parity, esc, sep, cm, inb);
    uint32_t st = 0, en = sep;                                  // a field's first byte (WORDS); the byte that ends a field
    if (WORDS) {
      const uint32_t wd = inb & ~sep, prev = (wd << 1) | carry;
      st = wd & ~prev; en = ~wd & prev & 0xFFFFu;               // (en may lie behind the body: at its end)
      carry = wd >> 15;
    }
    if (cm == 0 && !open) {                                     // no key ends here: only the field's begin moves
      const uint32_t last = WORDS ? st : en;
      if (last) { fbeg = (unsigned long long)(g - base) + (31u - (uint32_t)__builtin_clz(last)) + (WORDS ? 0u : 1u); has_c = false; }
      continue;
    }
    uint32_t ev = st | en | cm;
    while (ev) {                                                // the granule's events, in address order
      const uint32_t p = (uint32_t)__builtin_ctz(ev), bit = 1u << p;
      ev &= ev - 1;
      const unsigned long long at = (unsigned long long)(g - base) + p;
      if (WORDS && (st & bit)) { fbeg = at; has_c = false; }
      if (en & bit) {
        if (LOCATE && open) { fe[d] = at; dlen[2 * d] = at - cb; dlen[2 * d + 1] = 0; ++d; }
        open = false;
        if (!WORDS) { fbeg = at + 1; has_c = false; }
      } else if ((cm & bit) && !has_c) {                        // the field's key is in[fbeg, at)
        has_c = true;
        const uint32_t t = kv_match(in, fbeg, at - fbeg, V, found);
        if (t < 16) {
          found |= 1u << t;
          if (LOCATE) {
            fb[d] = at + 1; dkey[d] = (uint8_t)t; cb = at + 1; open = true;
            if (krow) krow[t] = (uint8_t)(d - dfirst);
          }
        }
      }
    }
  }
  if (LOCATE && open) { fe[d] = be; dlen[2 * d] = be - cb; dlen[2 * d + 1] = 0; }   // the body ends inside the value
  return found;
}

// k_kvcount's lane: the names record body in[s, be) has, in *found; returns its number of documents — one per name found, or
// none if it lacks a required name
template <int MODE, bool WORDS>
KX_LANE unsigned long long kv_count_lane(const uint8_t* __restrict__ in, unsigned long long s, unsigned long long be, const KVBytes& B,
                                         const KVSpec& V, unsigned long long* found) {
  const uint32_t f = kv_walk<MODE, WORDS, false>(in, s, be, B, V, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
  *found = f;
  return (f & V.req) == V.req ? (unsigned long long)__builtin_popcount(f) : 0ull;
}

// k_kvlocate's lane: the documents da .. db - 1 (db > da) of the record body in[s, be), as kv_walk writes them; krow: null, or
// the record's 16 bytes of kdoc, which are written whole
template <int MODE, bool WORDS>
KX_LANE void kv_locate_lane(const uint8_t* __restrict__ in, unsigned long long s, unsigned long long be, const KVBytes& B, const KVSpec& V,
                            unsigned long long da, unsigned long long* __restrict__ fb, unsigned long long* __restrict__ fe,
                            unsigned long long* __restrict__ dlen, uint8_t* __restrict__ dkey, uint8_t* __restrict__ krow) {
  if (krow) {
#ifdef __HIPCC__
    *reinterpret_cast<uint4*>(krow) = make_uint4(~0u, ~0u, ~0u, ~0u);
#else
    memset(krow, 0xFF, 16);
#endif
  }
  (void)kv_walk<MODE, WORDS, true>(in, s, be, B, V, da, fb, fe, dlen, dkey, krow);
}
