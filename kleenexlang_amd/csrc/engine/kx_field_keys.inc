// kx_field_keys.inc — device side of field mode BY KEY (include/kxhip.h: kx_run_batch_field_keys, kx_run_records_fd_field_keys;
// `BIN --records … --field=LIST --keys[=C]`): the fields of a record are cut as ever — by the live F bytes, or with WORDS into
// the words between live blanks — and a field whose bytes before its first live C spell a listed name is selected: the program
// runs on its VALUE, the bytes behind that C.  Included by kx_engine.hip behind kx_field_project.inc; the host driver is
// kx_field_list_host.inc's runFieldList with a switch for the kernels below, the normative model host.keyed_records_model.
//
//   k_kvcount   lane = record: the walk of kx_field_keys_lanes.h.  Writes the record's number of documents as a BDoc length — one
//               per name found, 0 if a required name is missing — and the 16-bit mask of the names found into nf[i].
//   k_kvlocate  lane = record: the same walk.  Writes fb[d] (the value's begin), fe[d] (the field's end), the length BDoc and the
//               name's index dkey[d] of every document of the record, in address order, and with a projection the record's 16
//               bytes of kdoc: the record-relative document of every name, or 0xFF.
// Everything between them and the last step is the list's: the scans, k_fgather or the value codec, kx_run_batch.  The last step
// knows a keyed run by kv_status (kx_field_lanes.h): a record without a document is ACCEPTED unless it lacks a required name.
//   k_kvsplen   k_flsplen with kv_status; a record without a document is as long as its body, separator and suffix.  k_flsplice
//               then copies such a record's body as its gap 0.
//   k_kpsplen, k_kpsplice   k_fpsplen and k_fpsplice — the same lane bodies — with the KVSpec: an item is a name, its document
//               comes from kdoc, and a record without any output writes its separator and the suffix alone.
// The names are a table in device memory (KVSpec::tab), never an indexed kernel argument: FLSpec's comment says why.  Bytes are
// read only inside the aligned granules that hold a byte of a record's body; no kernel here uses scratch memory.

#include "kx_field_keys_lanes.h"

static_assert(sizeof(BDoc) == 16 && BM_RUN == 0, "kv_walk writes a length record as two 64-bit words: the length, then zero");
static_assert(KV_PLAIN == FLD_PLAIN && KV_QUOTED == FLD_QUOTED && KV_ESCAPED == FLD_ESCAPED, "the lanes' modes are the kernels'");

template <int MODE, bool WORDS>
__global__ __launch_bounds__(FLD_BT) void k_kvcount(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                    unsigned long long n, FSpec F, KVSpec V, BDoc* __restrict__ cnt,
                                                    unsigned long long* __restrict__ nf) {
  const KVBytes B{F.fs, F.quote, F.escape, V.kv};
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    unsigned long long found;
    BDoc d{0, 0, BM_RUN, 0};
    d.len = kv_count_lane<MODE, WORDS>(in, off[i], fld_body_end(off[i + 1], i, F), B, V, &found);
    cnt[i] = d;
    nf[i] = found;
  }
}

template <int MODE, bool WORDS>
__global__ __launch_bounds__(FLD_BT) void k_kvlocate(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                     unsigned long long n, FSpec F, KVSpec V, const unsigned long long* __restrict__ d0,
                                                     unsigned long long* __restrict__ fb, unsigned long long* __restrict__ fe,
                                                     BDoc* __restrict__ len, uint8_t* __restrict__ dkey, uint8_t* __restrict__ kdoc) {
  const KVBytes B{F.fs, F.quote, F.escape, V.kv};
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long da = d0[i];
    if (da == d0[i + 1]) continue;                              // no listed name, or a required one is missing
    kv_locate_lane<MODE, WORDS>(in, off[i], fld_body_end(off[i + 1], i, F), B, V, da, fb, fe, reinterpret_cast<unsigned long long*>(len), dkey,
                                kdoc ? kdoc + 16 * i : nullptr);
  }
}

__global__ __launch_bounds__(FLD_BT) void k_kvsplen(const unsigned long long* __restrict__ off, unsigned long long n, FSpec F, KVSpec V,
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
      const kx_batch_doc r = kv_status(V, i, da, db, nf, drec, K);
      rejected = r.status != 0;
      if (!rejected) {
        const unsigned long long s = off[i], e = off[i + 1], be = fld_body_end(e, i, F);
        d.len = (be - s) + (F.keep ? e - be : 0ull) + sfx;
        if (da != db) d.len = d.len - (coff[db] - coff[da]) + (poff[db] - poff[da]);   // (a call without a document has no offsets)
      }
      rec[i] = r;
      if (fail_field) fail_field[i] = (uint32_t)K;
      len[i] = d;
    }
    const unsigned long long bal = __ballot(rejected);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&ctr[FC_REJECTED], (unsigned long long)__popcll(bal));
  }
}

__global__ __launch_bounds__(FLD_BT) void k_kpsplen(const unsigned long long* __restrict__ off, unsigned long long n, FPSpec P, KVSpec V,
                                                    const unsigned long long* __restrict__ d0, const unsigned long long* __restrict__ nf,
                                                    const unsigned long long* __restrict__ poff, const kx_batch_doc* __restrict__ drec,
                                                    kx_batch_doc* __restrict__ rec, uint32_t* __restrict__ fail_field, BDoc* __restrict__ len,
                                                    unsigned long long* __restrict__ ctr) {
  for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < n; base += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long i = base + threadIdx.x;
    bool rejected = false;
    if (i < n) {
      kx_batch_doc r;
      unsigned long long K;
      BDoc d{fp_splen_lane(P, off, i, d0, nf, poff, drec, &r, &K, &V), 0, BM_RUN, 0};
      rejected = r.status != 0;
      rec[i] = r;
      if (fail_field) fail_field[i] = (uint32_t)K;
      len[i] = d;
    }
    const unsigned long long bal = __ballot(rejected);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&ctr[FC_REJECTED], (unsigned long long)__popcll(bal));
  }
}

__global__ __launch_bounds__(FLD_GT) void k_kpsplice(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                     unsigned long long n, FPSpec P, KVSpec V, const unsigned long long* __restrict__ d0,
                                                     const uint8_t* __restrict__ pout, const unsigned long long* __restrict__ poff,
                                                     const unsigned long long* __restrict__ ooff, unsigned long long total,
                                                     uint8_t* __restrict__ out) {
  const unsigned long long ng = ((unsigned long long)((uintptr_t)out & 15) + total + 15) >> 4;
  for (unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += (unsigned long long)gridDim.x * blockDim.x)
    fp_splice_lane(P, in, off, n, d0, pout, poff, ooff, total, out, g, &V);
}
