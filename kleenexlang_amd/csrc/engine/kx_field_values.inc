// kx_field_values.inc — device side of field mode on unquoted VALUES (include/kxhip.h: kx_run_batch_field_values,
// kx_run_records_fd_field_values; `--unquote`): the program runs on the value of every selected field, and the field is replaced by
// the spelling of the program's output.  Included by kx_engine.hip behind kx_field_list.inc, whose records, documents, fb / fe and
// scans these kernels share; the driver is kx_run_batch_field_list's (kx_field_list_host.inc), the entry point is in
// kx_field_values_host.inc.  The two rules are host.unquote_field_model and host.requote_field_model.
//
// A document is one selected field, in[fb[d], fe[d]); every kernel here gives a document to one lane.
//
//   k_fvdeclen  the value rule with numbers only: the value's length as a BDoc, and the document's flag byte (FV_WAS_QUOTED: a
//               quote byte is set and the field begins with it)
//   the scan of the values' lengths (uoff)
//   k_fvdecode  the same walk, the value's bytes to ucomp + uoff[d]
//   [kx_run_batch over (ucomp, uoff): the program's outputs pout / poff and the documents' records]
//   k_fvenclen  an accepted document's output in one pass: the bytes that get a prefix or are doubled, and whether the spelling is
//               wrapped in quotes (FV_WRAP in the flag byte).  The spelling's length as a BDoc; a rejected document's is 0.
//   the scan of the spellings' lengths (qoff)
//   k_fvencode  the spelling to qout + qoff[d]
//   [k_flsplen and k_flsplice with (coff, qoff, qout) where they took (coff, poff, pout)]
// Bytes are read as aligned 16-byte granules, and only granules that hold a byte of the document (fv_bytes); they are written
// through FvOut, one 16-byte store per aligned granule that lies wholly inside the document's own output range, byte stores in
// the partial ones at its two ends — neighbouring documents belong to other lanes.

enum { FV_WAS_QUOTED = 1, FV_WRAP = 2 };           // a document's flag byte

// what the kernels know of the list's bytes and of a kx_field_codec: quote, escape = 256 where there is none (no byte equals it)
struct FVSpec { uint32_t fs, quote, escape, nsp; unsigned long long sp8; };   // sp8: the nsp special bytes, the first one lowest

// f(b) for every byte of base[a, e), in order
template <class Fn>
__device__ __forceinline__ void fv_bytes(const uint8_t* base, unsigned long long a, unsigned long long e, Fn f) {
  if (a >= e) return;                                           // (no byte: no granule)
  const uintptr_t pa = (uintptr_t)base + a, pe = (uintptr_t)base + e;
  for (uintptr_t g = pa & ~(uintptr_t)15; g < pe; g += 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(g);
    const unsigned long long lo = (unsigned long long)v.x | (unsigned long long)v.y << 32, hi = (unsigned long long)v.z | (unsigned long long)v.w << 32;
    const uint32_t t1 = pe - g < 16 ? (uint32_t)(pe - g) : 16u;
    for (uint32_t t = g < pa ? (uint32_t)(pa - g) : 0u; t < t1; ++t) f((uint32_t)((t < 8 ? lo : hi) >> (8 * (t & 7))) & 0xFFu);
  }
}

// buf (16-byte aligned) from offset start on, byte by byte
struct FvOut {
  uint8_t* buf;
  unsigned long long start, p, lo, hi;
  __device__ __forceinline__ FvOut(uint8_t* b, unsigned long long at) : buf(b), start(at), p(at), lo(0), hi(0) {}
  // the granule that ends at p, or what [start, p) holds of it
  __device__ __forceinline__ void flush() {
    const unsigned long long g = (p - 1) & ~15ull;
    if (g >= start && p - g == 16) *reinterpret_cast<uint4*>(buf + g) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    else
      for (unsigned long long q = g > start ? g : start; q < p; ++q) {
        const uint32_t k = (uint32_t)(q & 15);
        buf[q] = (uint8_t)(k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8)));
      }
    lo = hi = 0;
  }
  __device__ __forceinline__ void put(uint32_t v) {
    fld_put(lo, hi, (uint32_t)(p & 15), (uint8_t)v);
    if ((++p & 15) == 0) flush();
  }
  __device__ __forceinline__ void finish() { if (p > start && (p & 15)) flush(); }
};

// emit(b) for every byte of the value of the field in[fb, fe) (host.unquote_field_model): s = inside quotes, pc = the byte before
// was a closing quote, esc = the byte before was an unescaped escape byte.  QUOTED: there is no escape byte.
template <int MODE, class Fn>
__device__ __forceinline__ void fv_value(const uint8_t* in, unsigned long long fb, unsigned long long fe, const FVSpec& C, Fn emit) {
  uint32_t s = 0, pc = 0, esc = 0;
  fv_bytes(in, fb, fe, [&](uint32_t b) {
    if (MODE == FLD_ESCAPED && esc) { esc = 0; emit(b); }       // the byte behind an escape is data (a last escape alone: dropped)
    else if (MODE == FLD_ESCAPED && b == C.escape) { esc = 1; pc = 0; }
    else if (b == C.quote) {
      if (s) { s = 0; pc = 1; }                                 // a closing quote: nothing
      else { s = 1; if (pc) emit(C.quote); pc = 0; }            // an opening one right behind a closing one: the "" of a quoted field
    } else { emit(b); pc = 0; }
  });
}

template <int MODE>
__global__ __launch_bounds__(FLD_BT) void k_fvdeclen(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ fb,
                                                     const unsigned long long* __restrict__ fe, unsigned long long n, FVSpec C,
                                                     BDoc* __restrict__ len, uint8_t* __restrict__ flag) {
  for (unsigned long long d = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long a = fb[d], e = fe[d];
    unsigned long long v = 0;
    fv_value<MODE>(in, a, e, C, [&](uint32_t) { ++v; });
    const BDoc b{v, 0, BM_RUN, 0};
    len[d] = b;
    flag[d] = C.quote < 256u && e > a && in[a] == C.quote ? FV_WAS_QUOTED : 0;
  }
}

template <int MODE>
__global__ __launch_bounds__(FLD_BT) void k_fvdecode(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ fb,
                                                     const unsigned long long* __restrict__ fe, unsigned long long n, FVSpec C,
                                                     const unsigned long long* __restrict__ uoff, uint8_t* __restrict__ ucomp) {
  for (unsigned long long d = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (unsigned long long)gridDim.x * blockDim.x) {
    FvOut o(ucomp, uoff[d]);
    fv_value<MODE>(in, fb[d], fe[d], C, [&](uint32_t b) { o.put(b); });
    o.finish();
  }
}

__device__ __forceinline__ bool fv_special(const FVSpec& C, uint32_t b) {
  bool hit = false;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) hit |= k < C.nsp && ((uint32_t)(C.sp8 >> (8 * k)) & 0xFFu) == b;
  return hit;
}

// the spelling (host.requote_field_model) has one more byte in front of b: an escape byte, or with no escape byte the quote doubled
__device__ __forceinline__ bool fv_extra(const FVSpec& C, uint32_t b) {
  if (C.escape >= 256u) return b == C.quote;
  return b == C.escape || (C.quote < 256u ? b == C.quote : (b == C.fs || fv_special(C, b)));
}

// with a quote byte: b makes the spelling a quoted one
__device__ __forceinline__ bool fv_wraps(const FVSpec& C, uint32_t b) {
  return b == C.fs || fv_special(C, b) || (C.escape >= 256u && b == C.quote);
}

__global__ __launch_bounds__(FLD_BT) void k_fvenclen(const uint8_t* __restrict__ pout, const unsigned long long* __restrict__ poff,
                                                     const kx_batch_doc* __restrict__ drec, unsigned long long n, FVSpec C,
                                                     uint8_t* __restrict__ flag, BDoc* __restrict__ len) {
  for (unsigned long long d = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (unsigned long long)gridDim.x * blockDim.x) {
    BDoc b{0, 0, BM_RUN, 0};
    uint32_t f = flag[d] & FV_WAS_QUOTED;
    if (drec[d].status == 0) {                                  // (a rejected document is spelled as nothing, quoted or not)
      const unsigned long long a = poff[d], e = poff[d + 1];
      unsigned long long extra = 0;
      bool wraps = false;
      fv_bytes(pout, a, e, [&](uint32_t ch) { extra += fv_extra(C, ch) ? 1u : 0u; wraps |= fv_wraps(C, ch); });
      if (C.quote < 256u && (f || wraps)) f |= FV_WRAP;
      b.len = (e - a) + extra + (f & FV_WRAP ? 2u : 0u);
    }
    len[d] = b;
    flag[d] = (uint8_t)f;
  }
}

__global__ __launch_bounds__(FLD_BT) void k_fvencode(const uint8_t* __restrict__ pout, const unsigned long long* __restrict__ poff,
                                                     const kx_batch_doc* __restrict__ drec, unsigned long long n, FVSpec C,
                                                     const uint8_t* __restrict__ flag, const unsigned long long* __restrict__ qoff,
                                                     uint8_t* __restrict__ qout) {
  const uint32_t front = C.escape < 256u ? C.escape : C.quote;
  for (unsigned long long d = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (unsigned long long)gridDim.x * blockDim.x) {
    if (drec[d].status != 0) continue;
    const bool wrap = (flag[d] & FV_WRAP) != 0;
    FvOut o(qout, qoff[d]);
    if (wrap) o.put(C.quote);
    fv_bytes(pout, poff[d], poff[d + 1], [&](uint32_t ch) {
      if (fv_extra(C, ch)) o.put(front);
      o.put(ch);
    });
    if (wrap) o.put(C.quote);
    o.finish();
  }
}

// ---------------------------------------------------------------------------- host-side workspace of kx_run_batch_field_values
// grow-only device buffers of one program's runs on values (kx_program::field_values; freed by kx_free), beside the FieldListWs the
// driver fills: per document 8 + 8 bytes of the two offset arrays and a flag byte; per byte of the values one of ucomp; per byte of
// the spellings one of qout.
struct FieldValuesWs {
  BatchWs::Buf uoff, qoff, vflag, ucomp, qout;
  hipEvent_t ev[4] = {};
  bool have_events = false;
  ~FieldValuesWs() {
    for (BatchWs::Buf* b : {&uoff, &qoff, &vflag, &ucomp, &qout}) if (b->p) (void)hipFree(b->p);
    if (have_events) for (auto& e : ev) (void)hipEventDestroy(e);
  }
};
