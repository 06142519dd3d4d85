// kx_field_lanes.h — per-lane bodies of field mode's kernels that also compile as plain C++: the helpers the splice kernels share
// (fld_find, fld_put), the walks of the range table and the result of a record from its documents' (k_flsplen and k_fpsplen), and
// the two lane bodies of the projection (`--only`: k_fpsplen, k_fpsplice in kx_field_project.inc, which are thin grid-stride loops
// over them), and the status rule of keyed runs (KVSpec, kv_status: `--keys`, kx_field_keys.inc, whose projection runs the same two
// lane bodies with a KVSpec).  Included by kx_fields.inc inside kx_engine.hip, where KX_LANE is `__device__ __forceinline__`, and by
// tests/native/project_lanes.cpp, a stand-alone host program that runs the same text one lane at a time under a sanitizer.
// Needs kx_batch_doc (include/kxhip.h) from the including file; reads no other engine type.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define KX_LANE __device__ __forceinline__
#else
#define KX_LANE inline
#endif

constexpr unsigned long long FL_OPEN = ~0ull;      // hi of an open range; lo and hi of the entries behind the list's last range

// the last index r with o[r] <= pos, for pos < o[n] (o: n + 1 non-decreasing entries, o[0] = 0)
KX_LANE unsigned long long fld_find(const unsigned long long* __restrict__ o, unsigned long long n, unsigned long long pos) {
  unsigned long long lo = 0, hi = n + 1;
  while (lo < hi) {
    const unsigned long long mid = (lo + hi) >> 1;
    if (o[mid] <= pos) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

KX_LANE void fld_put(unsigned long long& lo, unsigned long long& hi, uint32_t k, uint8_t v) {
  if (k < 8) lo |= (unsigned long long)v << (8 * k); else hi |= (unsigned long long)v << (8 * (k - 8));
}

// ---- the selected set S as the kernels have it: rng = lo[0..7] then hi[0..7] in device memory (FL_OPEN behind the last range)

// field number of S's member number t (from 0)
KX_LANE unsigned long long fl_member(const unsigned long long* __restrict__ rng, unsigned long long t) {
  for (uint32_t k = 0; k < 8; ++k) {
    const unsigned long long lo = rng[k], hi = rng[8 + k];
    const unsigned long long size = hi == FL_OPEN ? FL_OPEN : hi - lo + 1;   // (behind the list: FL_OPEN, never reached)
    if (t < size) return lo + t;
    t -= size;
  }
  return 0;
}

// the smallest member of S above `fields` (there is one: fields < need)
KX_LANE unsigned long long fl_missing(const unsigned long long* __restrict__ rng, unsigned long long fields) {
  for (uint32_t k = 0; k < 8; ++k) {
    const unsigned long long lo = rng[k], hi = rng[8 + k];
    if (lo != FL_OPEN && hi > fields) return lo > fields ? lo : fields + 1;
  }
  return 0;
}

// record i's result from its documents da .. db - 1, and K of its report line (0: accepted): without a document the record had
// too few fields — {fields found, 2, 0}, K the smallest member it lacks; else the first document with a non-zero status gives the
// record's, K its field number
KX_LANE kx_batch_doc fl_status(const unsigned long long* __restrict__ rng, unsigned long long i, unsigned long long da, unsigned long long db,
                               const unsigned long long* __restrict__ nf, const kx_batch_doc* __restrict__ drec, unsigned long long& K) {
  kx_batch_doc r{0, 0u, 0u};
  K = 0;
  if (da == db) { r = kx_batch_doc{nf[i], 2u, 0u}; K = fl_missing(rng, nf[i]); }
  else {
    unsigned long long t = da;
    while (t < db && drec[t].status == 0) ++t;                  // the lowest rejected field
    if (t < db) { r = drec[t]; K = fl_member(rng, t - da); }
  }
  return r;
}

// ---- keyed runs (`--keys`, kx_field_keys.inc): a record's documents are the values of the first fields whose keys are the listed
// names, in address order; document t is the value of name dkey[t].

// what the kernels know of a kx_field_keys.  The names are a table in device memory as the ranges are (an indexed kernel argument
// would go through scratch): 16 lengths and 16 offsets of 16 bits each, then the names' bytes at tab + 64 + offset.
struct KVSpec {
  const uint8_t* tab;    // the names
  const uint8_t* dkey;   // per document: the index of its name (k_kvlocate writes it)
  const uint8_t* kdoc;   // with a projection, per record 16 bytes: the record-relative document of name t, or 0xFF
  uint32_t all, req;     // bit t: name t is listed; it is required
  uint32_t kv;           // the key separator C
};

// fl_status of a keyed run: nf[i] is the mask of the names record i has.  Without a document the record is accepted if it lacks no
// required name — else {names found, 2, 0}, K = 1 + the lowest required name it lacks (the names are numbered as written); else the
// first document with a non-zero status gives the record's, K = 1 + its name
KX_LANE kx_batch_doc kv_status(const KVSpec& V, unsigned long long i, unsigned long long da, unsigned long long db,
                               const unsigned long long* __restrict__ nf, const kx_batch_doc* __restrict__ drec, unsigned long long& K) {
  kx_batch_doc r{0, 0u, 0u};
  K = 0;
  if (da == db) {
    const uint32_t miss = V.req & ~(uint32_t)nf[i];
    if (miss) { r = kx_batch_doc{nf[i], 2u, 0u}; K = 1ull + (unsigned long long)__builtin_ctz(miss); }
  } else {
    unsigned long long t = da;
    while (t < db && drec[t].status == 0) ++t;                  // the rejected value at the lowest address
    if (t < db) { r = drec[t]; K = 1ull + V.dkey[t]; }
  }
  return r;
}

// ---- the projection (`--only`): an accepted record writes, item by item as the list was written, the outputs of the item's fields,
// every two consecutive outputs joined by OFS, then the kept separator, then the suffix.  An item's fields are consecutive members
// of S, so consecutive documents: item t of a record with the documents da .. da + m - 1 begins at document a = da + rank (the
// members of S below the item's lo) and has c of them: hi - lo + 1, or what the record has of them.  Only an item inside S's
// open range can have fewer, or none (3-,9-10 on a record of 5 fields: need is 3): the range's documents are the record's last,
// so c = min(hi - lo + 1, m - rank) and the fields found are not needed.  An item without a field writes nothing, no OFS either;
// a record with `need` fields has at least one output (the item that gave the open range its lo, or any closed one).  In a keyed
// run (`kv` set) item t is a name, P.itm[t] its index: its one document is kdoc[16 i + index], and an optional name the record
// lacks has none — an accepted record may then have no output at all, and writes its separator and the suffix alone.

// what k_fpsplen and k_fpsplice know of a kx_field_project and of the list's framing.  The items are a table in device memory as
// the ranges are (an indexed kernel argument would go through scratch): rank[0..15] then size[0..15], size = hi - lo + 1, or
// FL_OPEN for an open item.  The ranks depend on the call alone, so the host walks the ranges for them, once: a walk per item
// and lane put a chain of dependent loads in front of every offset k_fpsplice reads.
struct FPSpec {
  const unsigned long long* rng;   // S
  const unsigned long long* itm;   // the items as written: rank in S, size
  unsigned long long sep_len, whole;   // a record's body ends sep_len before its range's end; record `whole` has no separator
  unsigned long long ofs8, sfx8;   // OFS and the suffix, the first byte lowest
  uint32_t n_items, ofs_len, sfx_len, keep;
};

KX_LANE unsigned long long fp_body_end(const FPSpec& P, unsigned long long e, unsigned long long i) {
  return e - (i == P.whole ? 0ull : P.sep_len);
}

// item t of a record with m documents from da: its first document, and how many (0: a is not a document of the record's).  krow:
// null, or in a keyed run the record's 16 bytes of kdoc (c is then 0 or 1)
KX_LANE void fp_item(const FPSpec& P, uint32_t t, unsigned long long da, unsigned long long m, unsigned long long& a, unsigned long long& c,
                     const uint8_t* __restrict__ krow = nullptr) {
  const unsigned long long rk = P.itm[t], size = P.itm[16 + t];
  if (krow) {
    const uint32_t x = m ? krow[rk] : 0xFFu;                    // (a record without a document has no row)
    a = da + x;
    c = x != 0xFFu ? 1ull : 0ull;
    return;
  }
  a = da + rk;
  c = rk >= m ? 0ull : size < m - rk ? size : m - rk;
}

// k_fpsplen's lane: record i's result in *rec, K of its report line in *K, and the bytes it writes (0 for a rejected one)
KX_LANE unsigned long long fp_splen_lane(const FPSpec& P, const unsigned long long* __restrict__ off, unsigned long long i,
                                         const unsigned long long* __restrict__ d0, const unsigned long long* __restrict__ nf,
                                         const unsigned long long* __restrict__ poff, const kx_batch_doc* __restrict__ drec,
                                         kx_batch_doc* rec, unsigned long long* K, const KVSpec* kv = nullptr) {
  const unsigned long long da = d0[i], db = d0[i + 1];
  *rec = kv ? kv_status(*kv, i, da, db, nf, drec, *K) : fl_status(P.rng, i, da, db, nf, drec, *K);
  if (rec->status != 0) return 0;
  const unsigned long long e = off[i + 1], be = fp_body_end(P, e, i);
  unsigned long long len = (P.keep ? e - be : 0ull) + P.sfx_len, w = 0;   // w: the outputs written (at least one; keyed: or none)
  const uint8_t* const krow = kv ? kv->kdoc + 16 * i : nullptr;
  for (uint32_t t = 0; t < P.n_items; ++t) {
    unsigned long long a, c;
    fp_item(P, t, da, db - da, a, c, krow);
    if (c) len += poff[a + c] - poff[a];
    w += c;
  }
  return len + (w ? (w - 1) * P.ofs_len : 0ull);
}

// k_fpsplice's lane: granule g of out[0, total) as it lies in memory (any alignment; `lead` bytes of the first granule are not the
// output's).  Record r's bytes are out[ooff[r], ooff[r+1]).  The record of the lane's first byte by a search in ooff, the item by a
// walk of the at most 16 items, the output inside the item by a search: output j of item t starts, inside the record, at
//   item start + (poff[a + j] - poff[a]) + j * ofs_len,
// which does not decrease in j.  From there a cursor through output, OFS, output, …, separator, suffix; a record that begins
// inside the granule is entered at its first piece.  Of `in` only a kept separator's bytes are read.  One 16-byte store for a full
// granule, byte stores in the partial first and last one; nothing at or behind `total`.
KX_LANE void fp_splice_lane(const FPSpec& P, const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off, unsigned long long n,
                            const unsigned long long* __restrict__ d0, const uint8_t* __restrict__ pout,
                            const unsigned long long* __restrict__ poff, const unsigned long long* __restrict__ ooff,
                            unsigned long long total, uint8_t* __restrict__ out, unsigned long long g, const KVSpec* kv = nullptr) {
  enum { OUT = 0, OFS = 1, SEP = 2, SFX = 3 };
  const unsigned long long lead = (unsigned long long)((uintptr_t)out & 15);
  const unsigned long long p0 = (g << 4) < lead ? 0ull : (g << 4) - lead;
  const unsigned long long p1 = (g << 4) + 16 - lead < total ? (g << 4) + 16 - lead : total;
  unsigned long long r = fld_find(ooff, n, p0), rb = ooff[r], re = ooff[r + 1];   // (p0 < total: the record has output)
  // the record: its documents, its separator; the item the cursor is in: documents a .. a + c - 1; the cursor's output, or in
  // OFS the one behind it: number j of item t; the piece it is in: [ps, pe) of the record's output, its bytes at src
  unsigned long long e, be, da, m, a, c, j, ps, pe;
  uint32_t t, phase;
  const uint8_t* src;
  const uint8_t* krow = nullptr;                                // keyed: the record's row of kdoc
  bool has;                                                     // the record has an output (always, but in a keyed run)
  auto output = [&] {                                           // the piece at ps is output j of item t
    const unsigned long long b = poff[a + j];
    phase = OUT; pe = ps + (poff[a + j + 1] - b); src = pout + b;
  };
  auto separator = [&] { phase = SEP; pe = ps + (P.keep ? e - be : 0ull); src = in + be; };
  auto item = [&] {                                             // from item t on, the first one with a field; false: none
    for (; t < P.n_items; ++t) {
      fp_item(P, t, da, m, a, c, krow);
      if (c) return true;
    }
    return false;
  };
  auto enter = [&] {                                            // record r: its first output, if it has one
    e = off[r + 1]; be = fp_body_end(P, e, r); da = d0[r]; m = d0[r + 1] - da;
    if (kv) krow = kv->kdoc + 16 * r;
    t = 0; j = 0; ps = 0;
    has = item();
  };
  auto first = [&] { if (has) output(); else separator(); };    // the piece at the record's first byte
  auto advance = [&] {
    ps = pe;
    if (phase == OUT) {                                         // OFS if an output follows, in this item or a later one
      bool more = ++j < c;
      if (!more) { ++t; j = 0; more = item(); }
      if (more) { phase = OFS; pe = ps + P.ofs_len; } else separator();
    } else if (phase == OFS) output();
    else { phase = SFX; pe = ~0ull; }
  };
  enter();
  if (p0 == rb || !has) first();
  else {
    const unsigned long long k0 = p0 - rb;
    for (;;) {                                                  // the item that holds byte k0, or the OFS in front of it
      const unsigned long long ilen = poff[a + c] - poff[a] + (c - 1) * P.ofs_len;
      if (k0 < ps + ilen) {
        const unsigned long long b0 = poff[a];
        unsigned long long lo = 1, hi = c;                      // the item's outputs that start at or before k0 (number 0 does)
        while (lo < hi) {
          const unsigned long long mid = (lo + hi) >> 1;
          if (ps + (poff[a + mid] - b0) + mid * P.ofs_len <= k0) lo = mid + 1; else hi = mid;
        }
        j = lo - 1;                                             // in output j or the OFS behind it (the cursor steps on from there)
        ps += (poff[a + j] - b0) + j * P.ofs_len;
        output();
        break;
      }
      ps += ilen;
      ++t;
      if (!item()) { separator(); break; }                      // behind the last output
      if (k0 < ps + P.ofs_len) { phase = OFS; pe = ps + P.ofs_len; break; }
      ps += P.ofs_len;
    }
  }
  unsigned long long lo = 0, hi = 0;
  for (unsigned long long pos = p0; pos < p1; ++pos) {
    if (pos >= re) {   // (pos < total = ooff[n]: r stays below n; a record with no output is stepped over)
      do { ++r; rb = re; re = ooff[r + 1]; } while (pos >= re);
      enter();
      first();
    }
    const unsigned long long k = pos - rb;
    while (k >= pe) advance();
    const uint8_t v = phase == SFX ? (uint8_t)(P.sfx8 >> (8 * (k - ps))) : phase == OFS ? (uint8_t)(P.ofs8 >> (8 * (k - ps))) : src[k - ps];
    fld_put(lo, hi, (uint32_t)((lead + pos) & 15), v);
  }
  if (p1 - p0 == 16) {
#ifdef __HIPCC__
    *reinterpret_cast<uint4*>(out + p0) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
#else
    for (uint32_t k = 0; k < 16; ++k) out[p0 + k] = (uint8_t)(k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8)));   // (the host has no uint4)
#endif
  } else
    for (unsigned long long pos = p0; pos < p1; ++pos) {
      const uint32_t k = (uint32_t)((lead + pos) & 15);
      out[pos] = (uint8_t)(k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8)));
    }
}
