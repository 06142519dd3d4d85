// kx_field_list_host.inc — host driver of field mode with a list of fields (kx_run_batch_field_list, include/kxhip.h; kernels in
// kx_field_list.inc).  Included at the end of kx_engine.hip between kx_fields_host.inc and kx_records_host.inc.
//
// k_fcheck → k_flcount → scan of the document counts (d0, ndocs) → k_fllocate → scan of the documents' lengths → k_fgather into
// the compact buffer → kx_run_batch over it into the second workspace buffer (its document records are a workspace array of ndocs
// entries) → k_flsplen → scan of the output lengths into the caller's offsets → k_flsplice.  Host round trips of its own: the
// offset check, the documents' total, the fields' total, the output's total.  With no document (every record too short) the steps
// from k_fllocate to kx_run_batch are skipped.  HIP-event times add into kx_fields_stats's groups (count and locate: locate_ms).
// The driver, runFieldList, is also kx_run_batch_field_values's (kx_field_values_host.inc): with a codec the program runs on the
// fields' values, and their spellings are spliced.

#include "kx_field_list.h"

namespace {

// the rules of a kx_batch_field_list (`who`), found before any device work: the list's own, then checkFields's for the rest
int checkFieldList(const kx_batch_field_list& l, const char* who) {
  auto no = [&](const char* what) { return setErr(KX_E_ARG, std::string(who) + ": " + what); };
  if (l.size != sizeof(kx_batch_field_list)) return no("kx_batch_field_list::size is not this library's");
  if (l.n_ranges < 1 || l.n_ranges > KX_FIELD_RANGES) return no("the field list has 1 to 8 ranges");
  if (!kxFieldListIsNormal(l.ranges, l.n_ranges)) return no("the field list is not in normal form (sorted, disjoint, not adjacent, only the last range open)");
  kx_batch_fields f{};
  f.size = sizeof f; f.field = l.ranges[0].lo; f.fs = l.fs;
  memcpy(f.pad, l.pad, sizeof f.pad);
  f.quote = l.quote; f.escape = l.escape; f.sep_len = l.sep_len; f.last_whole = l.last_whole; f.keep_sep = l.keep_sep;
  f.suffix_len = l.suffix_len;
  memcpy(f.reserved, l.reserved, sizeof f.reserved);
  return checkFields(f, who);
}

// The driver of kx_run_batch_field_list (codec = null) and of kx_run_batch_field_values (kx_field_values_host.inc; `who` names the
// entry point, whose checks of `l` and `codec` have passed).  With a codec the documents the program runs on are the fields' VALUES
// — k_fvdeclen, a scan and k_fvdecode take k_fgather's place — and k_fvenclen, a scan and k_fvencode spell the program's outputs
// before k_flsplen and k_flsplice, which then take the spellings and their offsets for the outputs and theirs (kx_field_values.inc).
// Without one, the kernels and their arguments are the list's own.  With `words` (kx_run_batch_field_words, kx_field_words_host.inc)
// the fields are the body's words: k_fwcount and k_fwlocate (kx_field_words.inc) take the place of k_flcount and k_fllocate, l->fs
// is not used, and the value kernels' field separator is the space.  Nothing else differs.  With `proj`
// (kx_run_batch_field_project, kx_field_project_host.inc, whose checks have passed) steps 1 to 4v are the same but for the value
// kernels' field separator, which is the OFS byte, and steps 5 and 6 are k_fpsplen and k_fpsplice (kx_field_project.inc) over the
// items' table; without it every launch and every argument is what it is without the parameter.  With `identity`
// (kx_run_batch_field_header; with `proj` only) step 4 is left out: the gathered fields — with a codec the decoded values — and
// their offsets stand in for the program's outputs and theirs, and the document records are zeroed (every one accepted); steps 4v,
// 5 and 6 run as they are.  Without it every launch and every argument is what it is without the parameter.  With `keyed`
// (kx_run_batch_field_keys, kx_field_keys_host.inc, whose checks have passed; l->n_ranges is 0 and the ranges' table is not read)
// steps 1 and 2 are k_kvcount and k_kvlocate (kx_field_keys.inc; `words` says how fields are cut), nf holds the masks of the names
// found, a record without a document may be an accepted one, step 5 is k_kvsplen or with `proj` k_kpsplen, and with `proj` step 6
// is k_kpsplice; a call without any document skips steps 2 to 4v as ever and still writes its accepted records.  Without it
// every launch and every argument is what it is without the parameter.
struct KeyedRun {
  uint8_t tab[64 + 16 * 255];    // KVSpec::tab: 16 lengths, 16 offsets (16 bits each), the names' bytes
  uint32_t all, req, kv;         // the masks of the listed and of the required names; the key separator
};

int runFieldList(kx_program* p, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_field_list* l,
                 const kx_field_codec* codec, void* d_out, size_t cap, uint64_t* d_out_off, kx_batch_doc* d_docs, uint32_t* d_fail_field,
                 size_t* out_len, kx_batch_stats* stats, void* stream, const char* who, bool words = false,
                 const kx_field_project* proj = nullptr, bool identity = false, const KeyedRun* keyed = nullptr) {
  if (n_docs && (!d_in_off || !d_out_off || !d_docs)) return setErr(KX_E_ARG, std::string(who) + ": offsets, output offsets and document records are required");
  if (n_docs >= 0xFFFFFFFFull) return setErr(KX_E_ARG, std::string(who) + ": at most 2^32 - 2 documents per call");
  *out_len = 0;
  const hipStream_t sm = (hipStream_t)stream;
  if (n_docs == 0) {
    if (d_out_off) { HIPCHECK(hipMemsetAsync(d_out_off, 0, 8, sm)); HIPCHECK(hipStreamSynchronize(sm)); }
    if (stats) { kx_batch_stats z{}; *stats = z; }
    return 0;
  }
  if (!p->field_list) p->field_list = new FieldListWs;
  if (!p->fields) p->fields = new FieldWs;   // (its times are kx_fields_stats's)
  if (codec && !p->field_values) p->field_values = new FieldValuesWs;
  FieldListWs& W = *p->field_list;
  FieldValuesWs* const V = codec ? p->field_values : nullptr;
  const bool timing = p->cfg.collect_timing != 0;
  if (timing && !W.have_events) {
    for (auto& e : W.ev) HIPCHECK(hipEventCreate(&e));
    W.have_events = true;
  }
  if (timing && V && !V->have_events) {
    for (auto& e : V->ev) HIPCHECK(hipEventCreate(&e));
    V->have_events = true;
  }
  const uint64_t nd = n_docs;
  int rc = BatchWs::ensure(W.ctr, FC_N * 8);
  if (!rc) rc = BatchWs::ensure(W.rng, 16 * 8);
  if (!rc && proj) rc = BatchWs::ensure(W.itm, 32 * 8);
  if (!rc && keyed) rc = BatchWs::ensure(W.ktab, sizeof keyed->tab);
  if (!rc && keyed && proj) rc = BatchWs::ensure(W.kdoc, nd * 16);
  if (!rc) rc = BatchWs::ensure(W.d0, (nd + 1) * 8);
  if (!rc) rc = BatchWs::ensure(W.nf, nd * 8);
  if (!rc) rc = BatchWs::ensure(W.cnt, nd * sizeof(BDoc));
  for (BatchWs::Buf* b : {&W.wsum, &W.woff}) if (!rc) rc = BatchWs::ensure(*b, (size_t)((nd + 1 + 1023) / 1024) * 8);
  if (!rc) rc = BatchWs::ensure(W.flags, sizeof(Flags));
  if (rc) return rc;
  unsigned long long* ctr = (unsigned long long*)W.ctr.p;
  unsigned long long *d0 = (unsigned long long*)W.d0.p, *nf = (unsigned long long*)W.nf.p;
  BDoc* cnt = (BDoc*)W.cnt.p;
  Flags* fl = (Flags*)W.flags.p;
  const unsigned long long* off = (const unsigned long long*)d_in_off;
  FLSpec L{};
  L.rng = (const unsigned long long*)W.rng.p;
  unsigned long long hrng[16];   // the table: lo[0..7], hi[0..7]
  L.F = FSpec{0, l->sep_len, l->last_whole ? nd - 1 : FLD_NONE, l->fs, l->quote < 0 ? 256u : (uint32_t)l->quote,
              l->escape < 0 ? 256u : (uint32_t)l->escape, l->keep_sep ? 1u : 0u};
  for (uint32_t j = 0; j < 8; ++j) {
    const bool in = j < l->n_ranges, open = in && l->ranges[j].hi == 0;
    hrng[j] = in ? l->ranges[j].lo : FL_OPEN;
    hrng[8 + j] = in && !open ? l->ranges[j].hi : FL_OPEN;
    if (open) L.open_lo = l->ranges[j].lo;
    if (in && !open) L.closed += (unsigned long long)l->ranges[j].hi - l->ranges[j].lo + 1;
    if (in) L.need = open ? l->ranges[j].lo : l->ranges[j].hi;   // (the last range's: the largest)
  }
  unsigned long long sfx8 = 0;
  for (uint32_t i = 0; i < l->suffix_len; ++i) sfx8 |= (unsigned long long)l->suffix[i] << (8 * i);
  FPSpec P{};                    // with a projection: the items' table rank[0..15], size[0..15], and the framing once more
  unsigned long long hitm[32];
  if (proj) {
    P = FPSpec{L.rng, (const unsigned long long*)W.itm.p, L.F.sep_len, L.F.whole, 0ull, sfx8, proj->n_items, proj->ofs_len, l->suffix_len, L.F.keep};
    for (uint32_t i = 0; i < proj->ofs_len; ++i) P.ofs8 |= (unsigned long long)proj->ofs[i] << (8 * i);
    for (uint32_t j = 0; j < 16; ++j) {
      const bool in = j < proj->n_items;
      unsigned long long rk = 0;   // the members of S below the item's lo: the ranges in front of the one that holds it, and its part of that
      for (uint32_t k = 0; in && k < l->n_ranges && l->ranges[k].lo <= proj->items[j].lo; ++k) {
        const bool holds = l->ranges[k].hi == 0 || l->ranges[k].hi >= proj->items[j].lo;
        rk += (unsigned long long)(holds ? proj->items[j].lo : l->ranges[k].hi + 1ull) - l->ranges[k].lo;
      }
      hitm[j] = rk;
      hitm[16 + j] = !in ? 0ull : proj->items[j].hi ? (unsigned long long)proj->items[j].hi - proj->items[j].lo + 1 : FL_OPEN;
      if (keyed) { hitm[j] = in ? proj->items[j].hi : 0ull; hitm[16 + j] = in ? 1ull : 0ull; }   // (an item is a name: its index, one document)
    }
  }
  KVSpec KV{};                   // keyed: the names' table; dkey and kdoc once they are allocated
  if (keyed) KV = KVSpec{(const uint8_t*)W.ktab.p, nullptr, proj ? (const uint8_t*)W.kdoc.p : nullptr, keyed->all, keyed->req, keyed->kv};
  // the offsets, checked on the device before any kernel reads a record
  HIPCHECK(hipMemsetAsync(ctr, 0, FC_N * 8, sm));
  HIPCHECK(hipMemcpyAsync(W.rng.p, hrng, sizeof hrng, hipMemcpyHostToDevice, sm));   // (hrng lives until the sync below)
  if (proj) HIPCHECK(hipMemcpyAsync(W.itm.p, hitm, sizeof hitm, hipMemcpyHostToDevice, sm));   // (and hitm)
  if (keyed) HIPCHECK(hipMemcpyAsync(W.ktab.p, keyed->tab, sizeof keyed->tab, hipMemcpyHostToDevice, sm));   // (the caller's: it outlives the call)
  hipLaunchKernelGGL(k_fcheck, dim3((uint32_t)((nd + 255) / 256)), dim3(256), 0, sm, off, (unsigned long long)nd, L.F, ctr);
  HIPCHECK(hipGetLastError());
  unsigned long long hc[FC_N] = {}, ends[2] = {0, 0};
  HIPCHECK(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(&ends[0], d_in_off, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(&ends[1], d_in_off + nd, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  if (hc[FC_BADOFF] || ends[1] < ends[0]) return setErr(KX_E_ARG, std::string(who) + ": the document offsets decrease");
  if (hc[FC_SHORT]) return setErr(KX_E_ARG, std::string(who) + ": a record's range is shorter than its separator");
  if (ends[1] > ends[0] && !d_in) return setErr(KX_E_ARG, std::string(who) + ": null input");
  const uint8_t* in = (const uint8_t*)d_in;
  const uint32_t bgrid = (uint32_t)std::min<uint64_t>((nd + FLD_BT - 1) / FLD_BT, (uint64_t)p->ncu * 4);
  auto granGrid = [&](unsigned long long bytes) {
    const unsigned long long g = ((bytes + 31) / 16 + FLD_GT - 1) / FLD_GT;
    return dim3((uint32_t)std::min<unsigned long long>(g ? g : 1, (unsigned long long)p->ncu * 16));
  };
  // exclusive scan of the k lengths in `len` into o (o[k] = the total, also left in Flags::total_len)
  auto scanLens = [&](const BDoc* len, unsigned long long k, unsigned long long* o) {
    const uint32_t ng = (uint32_t)((k + 1023) / 1024), g1024 = (uint32_t)((k + 1 + 1023) / 1024);
    hipLaunchKernelGGL(k_bscan_reduce, dim3(ng), dim3(1024), 0, sm, k, len, (unsigned long long*)W.wsum.p, (const kx_batch_doc*)nullptr, 0ull);
    hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(1024), 0, sm, ng, (const unsigned long long*)W.wsum.p, (unsigned long long*)W.woff.p, fl);
    hipLaunchKernelGGL(k_bscan_down, dim3(g1024), dim3(1024), 0, sm, k, len, (const unsigned long long*)W.woff.p, (const Flags*)fl, o,
                       (const kx_batch_doc*)nullptr, 0ull);
  };
  const int mode = l->escape >= 0 ? FLD_ESCAPED : l->quote >= 0 ? FLD_QUOTED : FLD_PLAIN;
  // 1. the records' documents: how many, and the first one's index
  if (timing) HIPCHECK(hipEventRecord(W.ev[0], sm));
  auto* const count = words ? (mode == FLD_ESCAPED ? &k_fwcount<FLD_ESCAPED> : mode == FLD_QUOTED ? &k_fwcount<FLD_QUOTED> : &k_fwcount<FLD_PLAIN>)
                            : (mode == FLD_ESCAPED ? &k_flcount<FLD_ESCAPED> : mode == FLD_QUOTED ? &k_flcount<FLD_QUOTED> : &k_flcount<FLD_PLAIN>);
  if (keyed) {
    auto* const kcount = words ? (mode == FLD_ESCAPED ? &k_kvcount<FLD_ESCAPED, true> : mode == FLD_QUOTED ? &k_kvcount<FLD_QUOTED, true> : &k_kvcount<FLD_PLAIN, true>)
                               : (mode == FLD_ESCAPED ? &k_kvcount<FLD_ESCAPED, false> : mode == FLD_QUOTED ? &k_kvcount<FLD_QUOTED, false> : &k_kvcount<FLD_PLAIN, false>);
    hipLaunchKernelGGL(kcount, dim3(bgrid), dim3(FLD_BT), 0, sm, in, off, (unsigned long long)nd, L.F, KV, cnt, nf);
  } else
  hipLaunchKernelGGL(count, dim3(bgrid), dim3(FLD_BT), 0, sm, in, off, (unsigned long long)nd, L, cnt, nf);
  if (timing) HIPCHECK(hipEventRecord(W.ev[1], sm));
  scanLens(cnt, nd, d0);
  if (timing) HIPCHECK(hipEventRecord(W.ev[2], sm));
  HIPCHECK(hipGetLastError());
  unsigned long long ndocs = 0;
  HIPCHECK(hipMemcpyAsync(&ndocs, &fl->total_len, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  if (ndocs >= 0xFFFFFFFFull) return setErr(KX_E_ARG, std::string(who) + ": the records select more than 2^32 - 2 fields in total");
  kx_batch_stats bst{};
  unsigned long long *fb = nullptr, *fe = nullptr, *coff = nullptr, *poff = nullptr;
  kx_batch_doc* drec = nullptr;
  const uint8_t* spliced = nullptr;   // with a codec: the spellings, which k_flsplice takes for the program's outputs
  const uint8_t* pbytes = nullptr;    // the program's outputs (with `identity`: the documents themselves)
  if (ndocs) {
    // 2. the documents' bounds, and the scan of their lengths
    for (BatchWs::Buf* b : {&W.fb, &W.fe}) if (!rc) rc = BatchWs::ensure(*b, ndocs * 8);
    for (BatchWs::Buf* b : {&W.coff, &W.poff}) if (!rc) rc = BatchWs::ensure(*b, (ndocs + 1) * 8);
    if (!rc) rc = BatchWs::ensure(W.len, ndocs * sizeof(BDoc));
    if (!rc) rc = BatchWs::ensure(W.drec, ndocs * sizeof(kx_batch_doc));
    if (!rc && keyed) rc = BatchWs::ensure(W.dkey, ndocs);
    for (BatchWs::Buf* b : {&W.wsum, &W.woff}) if (!rc) rc = BatchWs::ensure(*b, (size_t)((ndocs + 1 + 1023) / 1024) * 8);
    if (rc) return rc;
    fb = (unsigned long long*)W.fb.p; fe = (unsigned long long*)W.fe.p; coff = (unsigned long long*)W.coff.p; poff = (unsigned long long*)W.poff.p;
    drec = (kx_batch_doc*)W.drec.p;
    BDoc* len = (BDoc*)W.len.p;
    FVSpec C{};           // with a codec only: the bytes of the value kernels, and their grid (lane = document)
    uint32_t dgrid = 0;
    if (V) {
      C = FVSpec{proj ? (uint32_t)proj->ofs[0] : words ? 0x20u : (uint32_t)l->fs, L.F.quote, L.F.escape, codec->n_special, 0ull};
      for (uint32_t i = 0; i < C.nsp; ++i) C.sp8 |= (unsigned long long)codec->special[i] << (8 * i);
      dgrid = (uint32_t)std::min<uint64_t>((ndocs + FLD_BT - 1) / FLD_BT, (uint64_t)p->ncu * 4);
    }
    if (timing) HIPCHECK(hipEventRecord(W.ev[3], sm));
    auto* const locate = words ? (mode == FLD_ESCAPED ? &k_fwlocate<FLD_ESCAPED> : mode == FLD_QUOTED ? &k_fwlocate<FLD_QUOTED> : &k_fwlocate<FLD_PLAIN>)
                               : (mode == FLD_ESCAPED ? &k_fllocate<FLD_ESCAPED> : mode == FLD_QUOTED ? &k_fllocate<FLD_QUOTED> : &k_fllocate<FLD_PLAIN>);
    if (keyed) {
      KV.dkey = (const uint8_t*)W.dkey.p;
      auto* const klocate = words ? (mode == FLD_ESCAPED ? &k_kvlocate<FLD_ESCAPED, true> : mode == FLD_QUOTED ? &k_kvlocate<FLD_QUOTED, true> : &k_kvlocate<FLD_PLAIN, true>)
                                  : (mode == FLD_ESCAPED ? &k_kvlocate<FLD_ESCAPED, false> : mode == FLD_QUOTED ? &k_kvlocate<FLD_QUOTED, false> : &k_kvlocate<FLD_PLAIN, false>);
      hipLaunchKernelGGL(klocate, dim3(bgrid), dim3(FLD_BT), 0, sm, in, off, (unsigned long long)nd, L.F, KV, (const unsigned long long*)d0, fb, fe, len,
                         (uint8_t*)W.dkey.p, proj ? (uint8_t*)W.kdoc.p : nullptr);
    } else
    hipLaunchKernelGGL(locate, dim3(bgrid), dim3(FLD_BT), 0, sm, in, off, (unsigned long long)nd, L, (const unsigned long long*)d0, fb, fe, len);
    if (timing) HIPCHECK(hipEventRecord(W.ev[4], sm));
    scanLens(len, ndocs, coff);
    if (timing) HIPCHECK(hipEventRecord(W.ev[5], sm));
    HIPCHECK(hipGetLastError());
    unsigned long long ctotal = 0;
    HIPCHECK(hipMemcpyAsync(&ctotal, &fl->total_len, 8, hipMemcpyDeviceToHost, sm));
    HIPCHECK(hipStreamSynchronize(sm));
    // 3. the compact buffer: the fields' bytes, or their values
    const void* docs_in = nullptr;                // what the program runs on: ndocs documents at docs_off, docs_total bytes
    const unsigned long long* docs_off = coff;
    unsigned long long docs_total = ctotal;
    if (!V) {
      rc = BatchWs::ensure(W.comp, ctotal + 32);
      if (rc) return rc;
      if (timing) HIPCHECK(hipEventRecord(W.ev[6], sm));
      hipLaunchKernelGGL(k_fgather, granGrid(ctotal), dim3(FLD_GT), 0, sm, in, (const unsigned long long*)fb, (const unsigned long long*)coff,
                         ndocs, ctotal, (uint8_t*)W.comp.p);
      if (timing) HIPCHECK(hipEventRecord(W.ev[7], sm));
      HIPCHECK(hipGetLastError());
      docs_in = W.comp.p;
    } else {
      for (BatchWs::Buf* b : {&V->uoff, &V->qoff}) if (!rc) rc = BatchWs::ensure(*b, (ndocs + 1) * 8);
      if (!rc) rc = BatchWs::ensure(V->vflag, ndocs);
      if (rc) return rc;
      unsigned long long* uoff = (unsigned long long*)V->uoff.p;
      if (timing) HIPCHECK(hipEventRecord(V->ev[0], sm));
      auto* const declen = mode == FLD_ESCAPED ? &k_fvdeclen<FLD_ESCAPED> : &k_fvdeclen<FLD_QUOTED>;
      hipLaunchKernelGGL(declen, dim3(dgrid), dim3(FLD_BT), 0, sm, in, (const unsigned long long*)fb, (const unsigned long long*)fe, ndocs, C, len,
                         (uint8_t*)V->vflag.p);   // (the fields' lengths have been scanned into coff)
      scanLens(len, ndocs, uoff);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipMemcpyAsync(&docs_total, &fl->total_len, 8, hipMemcpyDeviceToHost, sm));
      HIPCHECK(hipStreamSynchronize(sm));
      rc = BatchWs::ensure(V->ucomp, docs_total + 32);
      if (rc) return rc;
      auto* const decode = mode == FLD_ESCAPED ? &k_fvdecode<FLD_ESCAPED> : &k_fvdecode<FLD_QUOTED>;
      hipLaunchKernelGGL(decode, dim3(dgrid), dim3(FLD_BT), 0, sm, in, (const unsigned long long*)fb, (const unsigned long long*)fe, ndocs, C,
                         (const unsigned long long*)uoff, (uint8_t*)V->ucomp.p);
      if (timing) HIPCHECK(hipEventRecord(V->ev[1], sm));
      HIPCHECK(hipGetLastError());
      docs_in = V->ucomp.p; docs_off = uoff;
    }
    // 4. the program on every selected field
    if (identity) {                               // (both compact buffers end in 32 bytes of slack)
      HIPCHECK(hipMemsetAsync(drec, 0, ndocs * sizeof(kx_batch_doc), sm));
      pbytes = (const uint8_t*)docs_in;
      poff = const_cast<unsigned long long*>(docs_off);
    } else {
      size_t pl = 0;
      const size_t slack = V ? 16 : 0;              // (k_fvenclen and k_fvencode read the outputs' last granule whole)
      rc = BatchWs::ensure(W.pout, docs_total + docs_total / 2 + 4096 + slack);
      if (rc) return rc;
      rc = kx_run_batch(p, docs_in, (const uint64_t*)docs_off, ndocs, W.pout.p, W.pout.cap - slack, (uint64_t*)poff, drec, &pl, &bst, stream);
      if (rc == KX_E_CAPACITY) {
        rc = BatchWs::ensure(W.pout, pl + 16 + slack);
        if (rc) return rc;
        rc = kx_run_batch(p, docs_in, (const uint64_t*)docs_off, ndocs, W.pout.p, W.pout.cap - slack, (uint64_t*)poff, drec, &pl, &bst, stream);
      }
      if (rc != 0 && rc != KX_MATCH_ERROR) return rc;
      pbytes = (const uint8_t*)W.pout.p;
    }
    // 4v. the spellings of the outputs take the outputs' place
    if (V) {
      unsigned long long* qoff = (unsigned long long*)V->qoff.p;
      if (timing) HIPCHECK(hipEventRecord(V->ev[2], sm));
      hipLaunchKernelGGL(k_fvenclen, dim3(dgrid), dim3(FLD_BT), 0, sm, pbytes, (const unsigned long long*)poff, (const kx_batch_doc*)drec,
                         ndocs, C, (uint8_t*)V->vflag.p, len);
      scanLens(len, ndocs, qoff);
      HIPCHECK(hipGetLastError());
      unsigned long long qtotal = 0;
      HIPCHECK(hipMemcpyAsync(&qtotal, &fl->total_len, 8, hipMemcpyDeviceToHost, sm));
      HIPCHECK(hipStreamSynchronize(sm));
      rc = BatchWs::ensure(V->qout, qtotal + 16);
      if (rc) return rc;
      hipLaunchKernelGGL(k_fvencode, dim3(dgrid), dim3(FLD_BT), 0, sm, pbytes, (const unsigned long long*)poff, (const kx_batch_doc*)drec,
                         ndocs, C, (const uint8_t*)V->vflag.p, (const unsigned long long*)qoff, (uint8_t*)V->qout.p);
      if (timing) HIPCHECK(hipEventRecord(V->ev[3], sm));
      HIPCHECK(hipGetLastError());
      poff = qoff; spliced = (const uint8_t*)V->qout.p;
    }
  }
  // 5. the records' results and output lengths, and their scan into the caller's offsets
  BDoc* rlen = cnt;   // (the counts have been scanned into d0)
  if (timing) HIPCHECK(hipEventRecord(W.ev[8], sm));
  if (keyed && proj)
    hipLaunchKernelGGL(k_kpsplen, dim3(bgrid), dim3(FLD_BT), 0, sm, off, (unsigned long long)nd, P, KV, (const unsigned long long*)d0,
                       (const unsigned long long*)nf, (const unsigned long long*)poff, (const kx_batch_doc*)drec, d_docs, d_fail_field, rlen, ctr);
  else if (keyed)
    hipLaunchKernelGGL(k_kvsplen, dim3(bgrid), dim3(FLD_BT), 0, sm, off, (unsigned long long)nd, L.F, KV, (const unsigned long long*)d0,
                       (const unsigned long long*)nf, (const unsigned long long*)coff, (const unsigned long long*)poff, (const kx_batch_doc*)drec,
                       d_docs, d_fail_field, (unsigned long long)l->suffix_len, rlen, ctr);
  else if (proj)
    hipLaunchKernelGGL(k_fpsplen, dim3(bgrid), dim3(FLD_BT), 0, sm, off, (unsigned long long)nd, P, (const unsigned long long*)d0,
                       (const unsigned long long*)nf, (const unsigned long long*)poff, (const kx_batch_doc*)drec, d_docs, d_fail_field, rlen, ctr);
  else
    hipLaunchKernelGGL(k_flsplen, dim3(bgrid), dim3(FLD_BT), 0, sm, off, (unsigned long long)nd, L, (const unsigned long long*)d0,
                       (const unsigned long long*)nf, (const unsigned long long*)coff, (const unsigned long long*)poff, (const kx_batch_doc*)drec,
                       d_docs, d_fail_field, (unsigned long long)l->suffix_len, rlen, ctr);
  scanLens(rlen, nd, (unsigned long long*)d_out_off);
  if (timing) HIPCHECK(hipEventRecord(W.ev[9], sm));
  HIPCHECK(hipGetLastError());
  unsigned long long total = 0, rej = 0;
  HIPCHECK(hipMemcpyAsync(&total, &fl->total_len, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(&rej, ctr + FC_REJECTED, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  *out_len = total;
  bst.docs = nd;
  bst.docs_rejected = rej;
  bst.in_bytes = ends[1] - ends[0];
  bst.out_bytes = total;
  if (stats) *stats = bst;
  if (total > cap || (total && !d_out)) return setErr(KX_E_CAPACITY, "output buffer too small");
  // 6. the splice
  if (timing) HIPCHECK(hipEventRecord(W.ev[10], sm));
  if (total && proj && keyed)
    hipLaunchKernelGGL(k_kpsplice, granGrid(total), dim3(FLD_GT), 0, sm, in, off, (unsigned long long)nd, P, KV, (const unsigned long long*)d0,
                       spliced ? spliced : pbytes, (const unsigned long long*)poff, (const unsigned long long*)d_out_off, total,
                       (uint8_t*)d_out);
  else if (total && proj)
    hipLaunchKernelGGL(k_fpsplice, granGrid(total), dim3(FLD_GT), 0, sm, in, off, (unsigned long long)nd, P, (const unsigned long long*)d0,
                       spliced ? spliced : pbytes, (const unsigned long long*)poff, (const unsigned long long*)d_out_off, total,
                       (uint8_t*)d_out);
  else if (total)
    hipLaunchKernelGGL(k_flsplice, granGrid(total), dim3(FLD_GT), 0, sm, in, off, (unsigned long long)nd, L.F, (const unsigned long long*)d0,
                       (const unsigned long long*)fb, (const unsigned long long*)fe, (const unsigned long long*)coff,
                       spliced ? spliced : pbytes, (const unsigned long long*)poff, (const unsigned long long*)d_out_off, total, sfx8, (uint8_t*)d_out);
  if (timing) HIPCHECK(hipEventRecord(W.ev[11], sm));
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(sm));
  if (timing) {
    FieldWs& T = *p->fields;
    T.locate_ms += evMs(W.ev[0], W.ev[1]) + (ndocs ? evMs(W.ev[3], W.ev[4]) : 0.f);
    T.scan_ms += evMs(W.ev[1], W.ev[2]) + (ndocs ? evMs(W.ev[4], W.ev[5]) : 0.f) + evMs(W.ev[8], W.ev[9]);   // (the last with k_flsplen, which feeds it)
    T.gather_ms += ndocs && !V ? evMs(W.ev[6], W.ev[7]) : 0.f;   // (with a codec nothing is gathered: the two events are not recorded)
    T.splice_ms += evMs(W.ev[10], W.ev[11]);
    if (V && ndocs) {   // (the values' decoding counts with the gather it replaces, the outputs' spelling with the splice it feeds)
      T.gather_ms += evMs(V->ev[0], V->ev[1]);
      T.splice_ms += evMs(V->ev[2], V->ev[3]);
    }
    ++T.calls;
  }
  return rej ? KX_MATCH_ERROR : 0;
}

}  // namespace

extern "C" int kx_run_batch_field_list(kx_program* p, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_field_list* l,
                                       void* d_out, size_t cap, uint64_t* d_out_off, kx_batch_doc* d_docs, uint32_t* d_fail_field, size_t* out_len,
                                       kx_batch_stats* stats, void* stream) {
  static const char* const who = "kx_run_batch_field_list";
  if (!p || !out_len || !l) return setErr(KX_E_ARG, "null argument");
  if (const int rc = checkFieldList(*l, who)) return rc;
  return runFieldList(p, d_in, d_in_off, n_docs, l, nullptr, d_out, cap, d_out_off, d_docs, d_fail_field, out_len, stats, stream, who);
}
