// kx_fields.inc — device side of field mode (include/kxhip.h: kx_run_batch_fields, kx_run_records_fd_fields): the program runs
// on field K of every record, the rest of the record is copied around its output.  Included by kx_engine.hip behind
// kx_records_rs.inc; the host driver is kx_fields_host.inc.
//
// A record is the range in[off[i], off[i+1]); its BODY is the range without its last sep_len bytes (the record separator; one
// record, `whole`, may have none).  The body's fields lie between its live field separators F: every F byte (PLAIN), an F byte at
// even parity of the quote bytes before it in the record (QUOTED), an unescaped F byte at even parity of the record's unescaped
// quotes (ESCAPED).  The state at a record's start is 0.
//
//   k_fcheck    lane = record: offsets non-decreasing, no range shorter than the separator (else the call fails with KX_E_ARG
//               before any kernel reads a record)
//   k_flocate   lane = record: the aligned 16-byte granules that hold a byte of the body, in order, until live F number K.
//               Writes the field's begin and end (offsets in `in`) or the mark FLD_NONE with the number of fields found, and the
//               field's length as the BDoc that the batch's scan kernels read.  PLAIN: the exact zero-byte test of k_rcount
//               on (granule ^ F·0x01010101) and a popcount per word, no state; QUOTED, ESCAPED: byte by byte with the two-bit state.
//   k_bscan_reduce, k_scan_groups, k_bscan_down (kx_batch.inc, kx_engine.hip): exclusive scan of the field lengths
//   k_fgather   lane = aligned 16-byte granule of the COMPACT buffer: the record that holds the granule's first byte by a search
//               in the scanned offsets, then the granule's bytes from one field after the other; one 16-byte store per lane
//   [kx_run_batch over the compact buffer: the program's outputs and the documents' records]
//   k_fsplen    lane = record: the record's output length — 0 unless it was accepted, else prefix + program output + rest of
//               the body + kept separator + suffix — as a BDoc; a record without field K gets {fields found, 2, 0}
//   the scan again, into the caller's output offsets
//   k_fsplice   lane = aligned 16-byte granule of the OUTPUT (the first and the last may be partial): the record by a search in
//               the output offsets, every byte from the piece of the record it belongs to; one 16-byte store per full granule,
//               byte stores in the two partial ones.  Every output byte is written exactly once.
// Bytes are read only inside a record's own range (k_flocate: inside the granules of its body), written only below the total.

#include "kx_field_lanes.h"   // fld_find, fld_put: the splice kernels' helpers, which also compile as plain C++

constexpr uint32_t FLD_BT = 512;                   // threads per workgroup of the per-record kernels
constexpr uint32_t FLD_GT = 256;                   // threads per workgroup of the per-granule kernels
constexpr unsigned long long FLD_NONE = ~0ull;     // fb[i]: the record has no field K (fe[i] = the fields it has)
enum { FC_BADOFF = 0, FC_SHORT = 1, FC_REJECTED = 2, FC_N = 4 };
enum { FLD_PLAIN = 0, FLD_QUOTED = 1, FLD_ESCAPED = 2 };

// what the kernels know of a kx_batch_fields: quote, escape = 256 where there is none (no byte equals it)
struct FSpec { unsigned long long field, sep_len, whole; uint32_t fs, quote, escape, keep; };

__device__ __forceinline__ unsigned long long fld_body_end(unsigned long long e, unsigned long long i, const FSpec& F) {
  return e - (i == F.whole ? 0ull : F.sep_len);
}

__global__ void k_fcheck(const unsigned long long* __restrict__ off, unsigned long long n, FSpec F, unsigned long long* __restrict__ ctr) {
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (off[i + 1] < off[i]) atomicOr(&ctr[FC_BADOFF], 1ull);
  else if (i != F.whole && off[i + 1] - off[i] < F.sep_len) atomicOr(&ctr[FC_SHORT], 1ull);
}

// byte index (0 to 15) of set high bit number j (from 1) of the granule's match words
__device__ __forceinline__ uint32_t fld_select(const uint32_t (&m)[4], uint32_t j) {
  uint32_t at = 0;
  bool found = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t pk = (uint32_t)__popc(m[k]);
    if (!found && j <= pk) {
      uint32_t x = m[k];
      for (uint32_t t = 1; t < j; ++t) x &= x - 1;
      at = 4u * k + ((uint32_t)__builtin_ctz(x) >> 3);
      found = true;
    }
    j -= found ? 0u : pk;
  }
  return at;
}

template <int MODE>
__global__ __launch_bounds__(FLD_BT) void k_flocate(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                    unsigned long long n, FSpec F, unsigned long long* __restrict__ fb,
                                                    unsigned long long* __restrict__ fe, BDoc* __restrict__ len) {
  const uint32_t pat = 0x01010101u * F.fs;
  const unsigned long long K = F.field;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long s = off[i], be = fld_body_end(off[i + 1], i, F);
    const uintptr_t base = (uintptr_t)in, pa = base + s, pe = base + be;
    unsigned long long c = 0;                                   // live separators met
    unsigned long long b = K == 1 ? s : FLD_NONE, e = FLD_NONE;
    uint32_t parity = 0, esc = 0;                               // (QUOTED, ESCAPED only)
    for (uintptr_t g = pa & ~(uintptr_t)15; g < pe && e == FLD_NONE; g += 16) {
      const uint4 v = *reinterpret_cast<const uint4*>(g);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      uint32_t m[4];
      if constexpr (MODE == FLD_PLAIN) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t x = w[k] ^ pat;
          m[k] = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
        }
        if (g < pa || g + 16 > pe) {   // (the body's first and last granule only)
#pragma unroll
          for (int k = 0; k < 4; ++k) m[k] &= rec_byte_span((long long)pa - (long long)(g + 4 * k), (long long)pe - (long long)(g + 4 * k));
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          m[k] = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uintptr_t a = g + 4 * k + j;
            if (a < pa || a >= pe) continue;
            const uint32_t ch = (w[k] >> (8 * j)) & 0xFFu;
            if (MODE == FLD_ESCAPED && esc) esc = 0;            // an escaped byte is only data
            else if (MODE == FLD_ESCAPED && ch == F.escape) esc = 1;
            else if (ch == F.quote) parity ^= 1u;
            else if (ch == F.fs && parity == 0) m[k] |= 0x80u << (8 * j);
          }
        }
      }
      const unsigned long long pc = (unsigned long long)(__popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]));
      if (pc) {
        if (b == FLD_NONE && c + pc >= K - 1) b = (unsigned long long)(g - base) + fld_select(m, (uint32_t)(K - 1 - c)) + 1;
        if (c + pc >= K) e = (unsigned long long)(g - base) + fld_select(m, (uint32_t)(K - c));
        c += pc;
      }
    }
    BDoc d{0, 0, BM_RUN, 0};
    if (b == FLD_NONE) { fb[i] = FLD_NONE; fe[i] = c + 1; }
    else {
      if (e == FLD_NONE) e = be;
      fb[i] = b; fe[i] = e; d.len = e - b;
    }
    len[i] = d;
  }
}

// comp (16-byte aligned, room for the last granule) = the fields one after the other; coff: their scanned lengths
__global__ __launch_bounds__(FLD_GT) void k_fgather(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ fb,
                                                    const unsigned long long* __restrict__ coff, unsigned long long n,
                                                    unsigned long long total, uint8_t* __restrict__ comp) {
  const unsigned long long ng = (total + 15) >> 4;
  for (unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += (unsigned long long)gridDim.x * blockDim.x) {
    unsigned long long pos = g << 4;
    const unsigned long long end = pos + 16 < total ? pos + 16 : total;
    unsigned long long r = fld_find(coff, n, pos), rb = coff[r], re = coff[r + 1], src = fb[r];
    unsigned long long lo = 0, hi = 0;
    for (uint32_t k = 0; pos < end; ++k, ++pos) {
      while (pos >= re) { ++r; rb = re; re = coff[r + 1]; src = fb[r]; }   // (pos < total = coff[n]: r stays below n)
      fld_put(lo, hi, k, in[src + (pos - rb)]);
    }
    *reinterpret_cast<uint4*>(comp + (g << 4)) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
  }
}

__global__ __launch_bounds__(FLD_BT) void k_fsplen(const unsigned long long* __restrict__ off, unsigned long long n, FSpec F,
                                                   const unsigned long long* __restrict__ fb, const unsigned long long* __restrict__ fe,
                                                   const unsigned long long* __restrict__ poff, kx_batch_doc* __restrict__ rec,
                                                   unsigned long long sfx, BDoc* __restrict__ len, unsigned long long* __restrict__ ctr) {
  // (the loop's bound is the workgroup's, so that whole waves take each step and one lane adds a wave's rejected records)
  for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < n; base += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long i = base + threadIdx.x;
    bool rejected = false;
    if (i < n) {
      BDoc d{0, 0, BM_RUN, 0};
      const unsigned long long b = fb[i];
      if (b == FLD_NONE) rec[i] = kx_batch_doc{fe[i], 2u, 0u};   // (run as an empty document; whatever that gave is overwritten)
      rejected = b == FLD_NONE || rec[i].status != 0;
      if (!rejected) {
        const unsigned long long s = off[i], e = off[i + 1], be = fld_body_end(e, i, F);
        d.len = (b - s) + (poff[i + 1] - poff[i]) + (be - fe[i]) + (F.keep ? e - be : 0ull) + sfx;
      }
      len[i] = d;
    }
    const unsigned long long bal = __ballot(rejected);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&ctr[FC_REJECTED], (unsigned long long)__popcll(bal));
  }
}

// out[0, total) (any alignment): record r's bytes are out[ooff[r], ooff[r+1]) = body[0, field begin) + the program's output +
// body[field end, body end) + the kept separator + the suffix
__global__ __launch_bounds__(FLD_GT) void k_fsplice(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                    unsigned long long n, FSpec F, const unsigned long long* __restrict__ fb,
                                                    const unsigned long long* __restrict__ fe, const uint8_t* __restrict__ pout,
                                                    const unsigned long long* __restrict__ poff, const unsigned long long* __restrict__ ooff,
                                                    unsigned long long total, unsigned long long sfx8, uint8_t* __restrict__ out) {
  const unsigned long long lead = (unsigned long long)((uintptr_t)out & 15), ng = (lead + total + 15) >> 4;
  for (unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long p0 = (g << 4) < lead ? 0ull : (g << 4) - lead;
    const unsigned long long p1 = (g << 4) + 16 - lead < total ? (g << 4) + 16 - lead : total;
    unsigned long long r = fld_find(ooff, n, p0), rb = 0, re = ooff[r];   // (the loop's first step loads record r)
    unsigned long long s = 0, fend = 0, be = 0, ps = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
    --r;
    unsigned long long lo = 0, hi = 0;
    for (unsigned long long pos = p0; pos < p1; ++pos) {
      while (pos >= re) {   // (pos < total = ooff[n]: r stays below n; a record with no output is stepped over)
        ++r; rb = re; re = ooff[r + 1];
        if (re > rb) {
          s = off[r]; be = fld_body_end(off[r + 1], r, F); fend = fe[r]; ps = poff[r];
          a1 = fb[r] - s; a2 = a1 + (poff[r + 1] - ps); a3 = a2 + (be - fend); a4 = a3 + (F.keep ? off[r + 1] - be : 0ull);
        }
      }
      const unsigned long long k = pos - rb;
      const uint8_t v = k < a1 ? in[s + k] : k < a2 ? pout[ps + (k - a1)] : k < a3 ? in[fend + (k - a2)] : k < a4 ? in[be + (k - a3)]
                                                                                                         : (uint8_t)(sfx8 >> (8 * (k - a4)));
      fld_put(lo, hi, (uint32_t)((lead + pos) & 15), v);
    }
    if (p1 - p0 == 16) *reinterpret_cast<uint4*>(out + p0) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    else
      for (unsigned long long pos = p0; pos < p1; ++pos) {
        const uint32_t k = (uint32_t)((lead + pos) & 15);
        out[pos] = (uint8_t)(k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8)));
      }
  }
}

// ---------------------------------------------------------------------------- host-side workspace of kx_run_batch_fields
// grow-only device buffers of one program's field runs (kx_program::fields; freed by kx_free).  Per record: 8 + 8 bytes of
// field bounds, 16 of a length record, 8 + 8 of the two offset arrays; per field byte one of the compact buffer; per byte of
// program output one of the second buffer.
struct FieldWs {
  BatchWs::Buf ctr, fb, fe, len, coff, comp, pout, poff, wsum, woff, flags;
  hipEvent_t ev[9] = {};
  bool have_events = false;
  float locate_ms = 0, gather_ms = 0, scan_ms = 0, splice_ms = 0;   // HIP events, with kx_config::collect_timing; summed over the calls
  uint64_t calls = 0;
  ~FieldWs() {
    for (BatchWs::Buf* b : {&ctr, &fb, &fe, &len, &coff, &comp, &pout, &poff, &wsum, &woff, &flags}) if (b->p) (void)hipFree(b->p);
    if (have_events) for (auto& e : ev) (void)hipEventDestroy(e);
  }
};
