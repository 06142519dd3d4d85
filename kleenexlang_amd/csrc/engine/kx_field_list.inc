// kx_field_list.inc — device side of field mode with a LIST of fields (include/kxhip.h: kx_run_batch_field_list,
// kx_run_records_fd_field_list): the program runs on every selected field of a record, the bytes between them are copied.  Included
// by kx_engine.hip behind kx_fields.inc, whose records, bodies, live separators, k_fcheck, k_fgather, fld_find and fld_put these
// kernels share; the host driver is kx_field_list_host.inc.
//
// The selected set S is at most 8 ranges in normal form (sorted, disjoint, not adjacent; only the last may be open).  A record with
// fewer than `need` fields (the largest number S names) selects nothing; any other record has one DOCUMENT per selected field, in
// field order.  Record i's documents are d0[i] .. d0[i+1] - 1 of one array for the whole call.
//
//   k_flcount   lane = record: the granules of the body as k_flocate walks them, the live F bytes counted (a closed list stops
//               once `need` fields are seen).  Writes the record's number of documents as a BDoc length and the fields found.
//   the 64-bit scan (k_bscan_reduce, k_scan_groups, k_bscan_down): d0, and the documents' total
//   k_fllocate  lane = record: the same walk with a cursor in the range list.  Writes fb[d], fe[d] (offsets in `in`) and the length
//               BDoc of every document of the record.  A granule in which no selected field begins or ends is passed on its
//               popcounts alone (the test needs the cursor's range only); the others are walked separator by separator.
//   the scan of the documents' lengths, k_fgather (unchanged: it takes any (fb, coff, n)), kx_run_batch over the compact buffer
//   k_flsplen   lane = record: the first of the record's documents with a non-zero status gives the record's; else its output
//               length = body - the fields' bytes + the outputs' bytes (two differences of scanned offsets) + separator + suffix
//   the scan again, into the caller's output offsets
//   k_flsplice  lane = aligned 16-byte granule of the OUTPUT: the record by a search in the output offsets, the piece of the
//               lane's first byte by a search over the record's documents — output j starts at the closed form fl_ostart, which
//               does not decrease in j — and from there a cursor through gap, output, gap, …, separator, suffix.
// Bytes are read only inside a record's own range (k_flcount, k_fllocate: inside the granules of its body), written only below the
// total; every output byte is written exactly once.

// (FL_OPEN, hi of an open range and lo and hi of the entries behind the list's last range, is kx_field_lanes.h's, with fl_member,
// fl_missing and fl_status, which walk the table)

// what the kernels know of a kx_batch_field_list (F.field is not used).  The ranges are a table in device memory, lo[0..7] then
// hi[0..7]: a kernel argument indexed by the cursor would go through scratch, and 32 more SGPRs would not fit.
struct FLSpec {
  FSpec F;
  const unsigned long long* rng;
  unsigned long long need;       // the largest field number the list names
  unsigned long long closed;     // the fields of the closed ranges
  unsigned long long open_lo;    // lo of the open range, 0: there is none
};

// range j of the list (j >= 8: nothing)
__device__ __forceinline__ void fl_range(const FLSpec& L, uint32_t j, unsigned long long& lo, unsigned long long& hi) {
  lo = hi = FL_OPEN;
  if (j < 8) { lo = L.rng[j]; hi = L.rng[8 + j]; }
}

// the live F bytes of the granule at g as the high bits of m; only bytes of the body [pa, pe) count.  PLAIN: k_rcount's exact
// zero-byte test, no state; QUOTED, ESCAPED: byte by byte with the two-bit state (k_flocate's rules).
template <int MODE>
__device__ __forceinline__ void fl_masks(uintptr_t g, uintptr_t pa, uintptr_t pe, const FSpec& F, uint32_t pat, uint32_t& parity,
                                         uint32_t& esc, uint32_t (&m)[4]) {
  const uint4 v = *reinterpret_cast<const uint4*>(g);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
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
}

template <int MODE>
__global__ __launch_bounds__(FLD_BT) void k_flcount(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                    unsigned long long n, FLSpec L, BDoc* __restrict__ cnt,
                                                    unsigned long long* __restrict__ nf) {
  const uint32_t pat = 0x01010101u * L.F.fs;
  const bool closed = L.open_lo == 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long s = off[i], be = fld_body_end(off[i + 1], i, L.F);
    const uintptr_t base = (uintptr_t)in, pa = base + s, pe = base + be;
    unsigned long long c = 0;                                   // live separators met
    uint32_t parity = 0, esc = 0;
    for (uintptr_t g = pa & ~(uintptr_t)15; g < pe && !(closed && c + 1 >= L.need); g += 16) {
      uint32_t m[4];
      fl_masks<MODE>(g, pa, pe, L.F, pat, parity, esc, m);
      c += (unsigned long long)(__popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]));
    }
    const unsigned long long fields = c + 1;                    // (a closed list that stopped early: at least `need`)
    BDoc d{0, 0, BM_RUN, 0};
    if (fields >= L.need) d.len = L.closed + (closed ? 0ull : fields - L.open_lo + 1);
    cnt[i] = d;
    nf[i] = fields;
  }
}

template <int MODE>
__global__ __launch_bounds__(FLD_BT) void k_fllocate(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                     unsigned long long n, FLSpec L, const unsigned long long* __restrict__ d0,
                                                     unsigned long long* __restrict__ fb, unsigned long long* __restrict__ fe,
                                                     BDoc* __restrict__ len) {
  const uint32_t pat = 0x01010101u * L.F.fs;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    unsigned long long d = d0[i];
    const unsigned long long dend = d0[i + 1];
    if (d == dend) continue;                                    // fewer than `need` fields
    const unsigned long long s = off[i], be = fld_body_end(off[i + 1], i, L.F);
    const uintptr_t base = (uintptr_t)in, pa = base + s, pe = base + be;
    unsigned long long c = 0;                                   // live separators met: the walk is in field c + 1
    uint32_t j = 0, parity = 0, esc = 0;
    unsigned long long lo, hi;                                  // the first range that does not end before field c + 1
    fl_range(L, 0, lo, hi);
    bool sel = lo <= 1;                                         // field c + 1 is a document; it began at cb
    unsigned long long cb = s;
    if (sel) fb[d] = s;
    for (uintptr_t g = pa & ~(uintptr_t)15; g < pe && d < dend; g += 16) {
      uint32_t m[4];
      fl_masks<MODE>(g, pa, pe, L.F, pat, parity, esc, m);
      const unsigned long long pc = (unsigned long long)(__popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]));
      if (pc == 0) continue;
      if (!sel && lo > c + pc + 1) { c += pc; continue; }       // no selected field begins or ends here
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uint32_t x = m[k];
        while (x) {                                             // the granule's live separators, in address order
          const unsigned long long at = (unsigned long long)(g - base) + 4u * k + ((uint32_t)__builtin_ctz(x) >> 3);
          x &= x - 1;
          if (sel) {                                            // it ends field c + 1
            BDoc b{at - cb, 0, BM_RUN, 0};
            fe[d] = at; len[d] = b;
            ++d;
          }
          ++c;                                                  // behind it begins field c + 1
          if (c + 1 > hi) fl_range(L, ++j, lo, hi);
          sel = c + 1 >= lo && d < dend;
          if (sel) { cb = at + 1; fb[d] = cb; }
        }
      }
    }
    if (sel && d < dend) {                                      // the body's last field
      BDoc b{be - cb, 0, BM_RUN, 0};
      fe[d] = be; len[d] = b;
    }
  }
}

__global__ __launch_bounds__(FLD_BT) void k_flsplen(const unsigned long long* __restrict__ off, unsigned long long n, FLSpec L,
                                                    const unsigned long long* __restrict__ d0, const unsigned long long* __restrict__ nf,
                                                    const unsigned long long* __restrict__ coff, const unsigned long long* __restrict__ poff,
                                                    const kx_batch_doc* __restrict__ drec, kx_batch_doc* __restrict__ rec,
                                                    uint32_t* __restrict__ fail_field, unsigned long long sfx, BDoc* __restrict__ len,
                                                    unsigned long long* __restrict__ ctr) {
  // (the loop's bound is the workgroup's, so that whole waves take each step and one lane adds a wave's rejected records)
  for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < n; base += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long i = base + threadIdx.x;
    bool rejected = false;
    if (i < n) {
      BDoc d{0, 0, BM_RUN, 0};
      const unsigned long long da = d0[i], db = d0[i + 1];
      unsigned long long K;
      const kx_batch_doc r = fl_status(L.rng, i, da, db, nf, drec, K);
      rejected = r.status != 0;
      if (!rejected) {
        const unsigned long long s = off[i], e = off[i + 1], be = fld_body_end(e, i, L.F);
        d.len = (be - s) - (coff[db] - coff[da]) + (poff[db] - poff[da]) + (L.F.keep ? e - be : 0ull) + sfx;
      }
      rec[i] = r;
      if (fail_field) fail_field[i] = (uint32_t)K;
      len[i] = d;
    }
    const unsigned long long bal = __ballot(rejected);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&ctr[FC_REJECTED], (unsigned long long)__popcll(bal));
  }
}

// out[0, total) (any alignment): record r's bytes out[ooff[r], ooff[r+1]) = gap 0 + output 0 + gap 1 + … + output m-1 + gap m + the
// kept separator + the suffix, for its documents da .. da + m - 1: gap j the body's bytes between field j - 1 and field j (from
// the body's start, to its end), output j the program's for field j.  Inside the record's output, output j starts at
//   fl_ostart(j) = (fb[da+j] - s) - (coff[da+j] - coff[da]) + (poff[da+j] - poff[da])
// (the body up to the field, less the fields in front of it, plus their outputs), which does not decrease in j.
__global__ __launch_bounds__(FLD_GT) void k_flsplice(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                     unsigned long long n, FSpec F, const unsigned long long* __restrict__ d0,
                                                     const unsigned long long* __restrict__ fb, const unsigned long long* __restrict__ fe,
                                                     const unsigned long long* __restrict__ coff, const uint8_t* __restrict__ pout,
                                                     const unsigned long long* __restrict__ poff, const unsigned long long* __restrict__ ooff,
                                                     unsigned long long total, unsigned long long sfx8, uint8_t* __restrict__ out) {
  enum { GAP = 0, OUT = 1, SEP = 2, SFX = 3 };
  const unsigned long long lead = (unsigned long long)((uintptr_t)out & 15), ng = (lead + total + 15) >> 4;
  for (unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long p0 = (g << 4) < lead ? 0ull : (g << 4) - lead;
    const unsigned long long p1 = (g << 4) + 16 - lead < total ? (g << 4) + 16 - lead : total;
    unsigned long long r = fld_find(ooff, n, p0), rb = ooff[r], re = ooff[r + 1];   // (p0 < total: the record has output)
    // the record: its range, its documents; the piece the cursor is in: [ps, pe) of the record's output, its bytes at src
    unsigned long long s, e, be, da, m, j, ps, pe;
    uint32_t phase;
    const uint8_t* src;
    auto ostart = [&](unsigned long long t) { return (fb[da + t] - s) - (coff[da + t] - coff[da]) + (poff[da + t] - poff[da]); };
    auto enter = [&] {                                          // record r from its first byte: gap 0
      s = off[r]; e = off[r + 1]; be = fld_body_end(e, r, F); da = d0[r]; m = d0[r + 1] - da;
      j = 0; phase = GAP; ps = 0; pe = (m ? fb[da] : be) - s; src = in + s;   // (keyed runs: no document, gap 0 is the whole body)
    };
    auto advance = [&] {
      if (phase == GAP && j < m) {                              // gap j -> output j
        const unsigned long long a = poff[da + j];
        phase = OUT; ps = pe; pe = ps + (poff[da + j + 1] - a); src = pout + a;
      } else if (phase == GAP) {                                // the last gap -> the separator
        phase = SEP; ps = pe; pe = ps + (F.keep ? e - be : 0ull); src = in + be;
      } else if (phase == OUT) {                                // output j -> gap j + 1
        const unsigned long long fend = fe[da + j];
        ++j; phase = GAP; ps = pe; src = in + fend;
        pe = ps + ((j < m ? fb[da + j] : be) - fend);
      } else { phase = SFX; ps = pe; pe = ~0ull; }              // the separator -> the suffix
    };
    enter();
    {
      const unsigned long long k0 = p0 - rb;
      unsigned long long lo = 0, hi = m;                        // the outputs that start at or before k0
      while (lo < hi) {
        const unsigned long long mid = (lo + hi) >> 1;
        if (ostart(mid) <= k0) lo = mid + 1; else hi = mid;
      }
      if (lo) {                                                 // in output lo - 1 or behind it (the cursor steps on from there)
        j = lo - 1;
        const unsigned long long a = poff[da + j];
        phase = OUT; ps = ostart(j); pe = ps + (poff[da + j + 1] - a); src = pout + a;
      }
    }
    unsigned long long lo = 0, hi = 0;
    for (unsigned long long pos = p0; pos < p1; ++pos) {
      if (pos >= re) {   // (pos < total = ooff[n]: r stays below n; a record with no output is stepped over)
        do { ++r; rb = re; re = ooff[r + 1]; } while (pos >= re);
        enter();
      }
      const unsigned long long k = pos - rb;
      while (k >= pe) advance();
      const uint8_t v = phase == SFX ? (uint8_t)(sfx8 >> (8 * (k - ps))) : src[k - ps];
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

// ---------------------------------------------------------------------------- host-side workspace of kx_run_batch_field_list
// grow-only device buffers of one program's field-list runs (kx_program::field_list; freed by kx_free).  Per record: 16 bytes of a
// length record (the document count, then the output length), 8 of the first document's index, 8 of the fields found.  Per
// document (selected field): 8 + 8 bytes of field bounds, 16 of a length record, 8 + 8 of the two offset arrays, 16 of the inner
// batch's document record.  Per selected byte one of the compact buffer; per byte of program output one of the second buffer.  128
// bytes for the ranges' table; with a projection (kx_field_project.inc) 256 for the items'.
struct FieldListWs {
  BatchWs::Buf ctr, rng, itm, cnt, d0, nf, fb, fe, len, coff, comp, pout, poff, drec, wsum, woff, flags;
  BatchWs::Buf ktab, dkey, kdoc;   // keyed runs (kx_field_keys.inc): the names' table, a byte per document, with a projection 16 per record
  hipEvent_t ev[12] = {};
  bool have_events = false;
  ~FieldListWs() {
    for (BatchWs::Buf* b : {&ctr, &rng, &itm, &cnt, &d0, &nf, &fb, &fe, &len, &coff, &comp, &pout, &poff, &drec, &wsum, &woff, &flags, &ktab, &dkey, &kdoc}) if (b->p) (void)hipFree(b->p);
    if (have_events) for (auto& e : ev) (void)hipEventDestroy(e);
  }
};
