// kx_field_words.inc — device side of field mode on WORDS (include/kxhip.h: kx_run_batch_field_words,
// kx_run_records_fd_field_words; `BIN --records … --field=LIST --blanks`): the fields of a body are the maximal runs of its bytes
// that are not live blanks, as awk's default splitting has them.  Included by kx_engine.hip behind kx_field_list.inc, whose FLSpec,
// range table, fl_range, k_flsplen and k_flsplice serve here unchanged; the host driver is kx_field_list_host.inc's runFieldList
// with a switch for the two kernels below.  The normative model is host.blank_field_list_records_model.
//
// A BLANK is the byte 0x20 or 0x09.  It is LIVE under the rule that makes an F byte live in kx_fields.inc: every one (PLAIN), one
// at even parity of the quote bytes before it in the record (QUOTED), an unescaped one at even parity of the record's unescaped
// quotes (ESCAPED); the state at a record's start is 0.  Words are numbered from 1; a word is never empty; a body that is empty or
// all live blanks has none.
//
//   k_fwcount   lane = record: the granules of the body as k_flcount walks them, the words that BEGIN counted (a closed list stops
//               once `need` words have begun).  Writes the record's number of documents as a BDoc length and the words found.
//   k_fwlocate  lane = record: the same walk with a cursor in the range list.  Writes fb[d], fe[d] (offsets in `in`) and the length
//               BDoc of every document of the record.  A granule in which no selected word begins or ends is passed on one
//               popcount; the others are walked event by event (a word's first byte; the first byte behind a word).
// Both see a granule through fw_masks: two 16-bit masks, bit p for the granule's byte p — the live blanks, and the bytes of the
// body.  The words' bytes are the body's bytes that are not live blanks; one bit is carried from granule to granule: was the last
// byte of the previous granule inside a word.  Bytes are read only inside the aligned granules that hold a byte of the body: an
// empty body loads nothing, whatever its address.

// the high bits of the four bytes of a match word as bits 0 to 3
__device__ __forceinline__ uint32_t fw_pack(uint32_t m) { return (((m >> 7) & 0x01010101u) * 0x01020408u) >> 24; }

// the granule at g: bl = its live blanks, inb = its bytes of the body [pa, pe); bit p of either is byte g + p.  PLAIN: k_rcount's
// exact zero-byte test on the granule ^ 0x20… and on the granule ^ 0x09…, no state; QUOTED, ESCAPED: byte by byte with the two-bit
// state (fl_masks's chain, "is a blank" in place of the field separator).
template <int MODE>
__device__ __forceinline__ void fw_masks(uintptr_t g, uintptr_t pa, uintptr_t pe, const FSpec& F, uint32_t& parity, uint32_t& esc,
                                         uint32_t& bl, uint32_t& inb) {
  const uint4 v = *reinterpret_cast<const uint4*>(g);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  bl = 0;
  if constexpr (MODE == FLD_PLAIN) {
    uint32_t m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t x = w[k] ^ 0x20202020u, y = w[k] ^ 0x09090909u;
      m[k] = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu) | ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
    }
    inb = 0xFFFFu;
    if (g < pa || g + 16 > pe) {   // (the body's first and last granule only)
      inb = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t span = rec_byte_span((long long)pa - (long long)(g + 4 * k), (long long)pe - (long long)(g + 4 * k));
        m[k] &= span;
        inb |= fw_pack(span) << (4 * k);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) bl |= fw_pack(m[k]) << (4 * k);
  } else {
    inb = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uintptr_t a = g + 4 * k + j;
        if (a < pa || a >= pe) continue;
        inb |= 1u << (4 * k + j);
        const uint32_t ch = (w[k] >> (8 * j)) & 0xFFu;
        if (MODE == FLD_ESCAPED && esc) esc = 0;            // an escaped byte is only data
        else if (MODE == FLD_ESCAPED && ch == F.escape) esc = 1;
        else if (ch == F.quote) parity ^= 1u;
        else if ((ch == 0x20u || ch == 0x09u) && parity == 0) bl |= 1u << (4 * k + j);
      }
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(FLD_BT) void k_fwcount(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                    unsigned long long n, FLSpec L, BDoc* __restrict__ cnt,
                                                    unsigned long long* __restrict__ nf) {
  const bool closed = L.open_lo == 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long s = off[i], be = fld_body_end(off[i + 1], i, L.F);
    const uintptr_t base = (uintptr_t)in, pa = base + s, pe = base + be;
    unsigned long long c = 0;                                   // words that have begun
    uint32_t parity = 0, esc = 0, carry = 0;                    // carry: the byte before the granule is a word's
    for (uintptr_t g = pa < pe ? pa & ~(uintptr_t)15 : pe; g < pe && !(closed && c >= L.need); g += 16) {
      uint32_t bl, inb;
      fw_masks<MODE>(g, pa, pe, L.F, parity, esc, bl, inb);
      const uint32_t wd = inb & ~bl;
      c += (unsigned long long)__popc(wd & ~((wd << 1) | carry));
      carry = wd >> 15;
    }
    BDoc d{0, 0, BM_RUN, 0};                                    // (a closed list that stopped early: at least `need` words)
    if (c >= L.need) d.len = L.closed + (closed ? 0ull : c - L.open_lo + 1);
    cnt[i] = d;
    nf[i] = c;
  }
}

template <int MODE>
__global__ __launch_bounds__(FLD_BT) void k_fwlocate(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                     unsigned long long n, FLSpec L, const unsigned long long* __restrict__ d0,
                                                     unsigned long long* __restrict__ fb, unsigned long long* __restrict__ fe,
                                                     BDoc* __restrict__ len) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    unsigned long long d = d0[i];
    const unsigned long long dend = d0[i + 1];
    if (d == dend) continue;                                    // fewer than `need` words
    const unsigned long long s = off[i], be = fld_body_end(off[i + 1], i, L.F);
    const uintptr_t base = (uintptr_t)in, pa = base + s, pe = base + be;
    unsigned long long c = 0;                                   // words that have begun: the walk is in word c, or behind it
    uint32_t j = 0, parity = 0, esc = 0, carry = 0;
    unsigned long long lo, hi;                                  // the first range that does not end before word c + 1
    fl_range(L, 0, lo, hi);
    bool open = false;                                          // word c is a document (number d), it began at cb and has not ended
    unsigned long long cb = s;
    for (uintptr_t g = pa < pe ? pa & ~(uintptr_t)15 : pe; g < pe && d < dend; g += 16) {
      uint32_t bl, inb;
      fw_masks<MODE>(g, pa, pe, L.F, parity, esc, bl, inb);
      const uint32_t wd = inb & ~bl, prev = (wd << 1) | carry;
      const uint32_t st = wd & ~prev, en = ~wd & prev & 0xFFFFu;   // a word's first byte; the first byte behind a word
      carry = wd >> 15;
      const unsigned long long ns = (unsigned long long)__popc(st);
      if (!open && lo > c + ns) { c += ns; continue; }          // no selected word begins or ends here
      uint32_t ev = st | en;                                    // (no byte is both)
      while (ev && d < dend) {                                  // the granule's events, in address order
        const uint32_t p = (uint32_t)__builtin_ctz(ev);
        ev &= ev - 1;
        const unsigned long long at = (unsigned long long)(g - base) + p;
        if ((st >> p) & 1u) {                                   // word c + 1 begins
          ++c;
          if (c > hi) fl_range(L, ++j, lo, hi);
          open = c >= lo;
          if (open) { cb = at; fb[d] = at; }
        } else if (open) {                                      // word c, a document, has ended
          BDoc b{at - cb, 0, BM_RUN, 0};
          fe[d] = at; len[d] = b;
          ++d;
          open = false;
        }
      }
    }
    if (open && d < dend) {                                     // the body ends inside the word
      BDoc b{be - cb, 0, BM_RUN, 0};
      fe[d] = be; len[d] = b;
    }
  }
}
