// kx_fields_host.inc — host driver of field mode (kx_run_batch_fields, include/kxhip.h; kernels in kx_fields.inc).  Included at
// the end of kx_engine.hip between kx_batch_host.inc and kx_records_host.inc.
//
// k_fcheck → k_flocate → scan of the field lengths → k_fgather into the compact buffer → kx_run_batch over it into the second
// workspace buffer (documents over batch_doc_max and register-action stages as kx_run_batch handles them; its document records are
// the caller's) → k_fsplen → scan of the output lengths into the caller's offsets → k_fsplice.  Host round trips of its own: the
// offset check, the fields' total, the output's total.  The batch kernels never see a (begin, end) pair.

namespace {

// the rules of a kx_batch_fields (`who`), found before any device work
int checkFields(const kx_batch_fields& f, const char* who) {
  auto no = [&](const char* what) { return setErr(KX_E_ARG, std::string(who) + ": " + what); };
  if (f.size != sizeof(kx_batch_fields)) return no("kx_batch_fields::size is not this library's");
  if (f.field == 0) return no("field numbers start at 1");
  if (f.quote < -1 || f.quote > 255) return no("quote must be a byte value or -1");
  if (f.escape < -1 || f.escape > 255) return no("escape must be a byte value or -1");
  if (f.quote == (int)f.fs) return no("the field separator cannot be the quote byte");
  if (f.escape == (int)f.fs) return no("the field separator cannot be the escape byte");
  if (f.quote >= 0 && f.quote == f.escape) return no("the escape byte cannot be the quote byte");
  if (f.sep_len > 8) return no("the record separator is at most 8 bytes");
  if (f.suffix_len > 8) return no("the suffix is at most 8 bytes");
  if (f.pad[0] || f.pad[1] || f.pad[2]) return no("reserved words must be 0");
  for (uint32_t r : f.reserved) if (r) return no("reserved words must be 0");
  return 0;
}

}  // namespace

extern "C" int kx_run_batch_fields(kx_program* p, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_fields* f,
                                   void* d_out, size_t cap, uint64_t* d_out_off, kx_batch_doc* d_docs, size_t* out_len, kx_batch_stats* stats,
                                   void* stream) {
  if (!p || !out_len || !f) return setErr(KX_E_ARG, "null argument");
  if (const int rc = checkFields(*f, "kx_run_batch_fields")) return rc;
  if (n_docs && (!d_in_off || !d_out_off || !d_docs)) return setErr(KX_E_ARG, "kx_run_batch_fields: offsets, output offsets and document records are required");
  if (n_docs >= 0xFFFFFFFFull) return setErr(KX_E_ARG, "kx_run_batch_fields: at most 2^32 - 2 documents per call");
  *out_len = 0;
  const hipStream_t sm = (hipStream_t)stream;
  if (n_docs == 0) {
    if (d_out_off) { HIPCHECK(hipMemsetAsync(d_out_off, 0, 8, sm)); HIPCHECK(hipStreamSynchronize(sm)); }
    if (stats) { kx_batch_stats z{}; *stats = z; }
    return 0;
  }
  if (!p->fields) p->fields = new FieldWs;
  FieldWs& W = *p->fields;
  const bool timing = p->cfg.collect_timing != 0;
  if (timing && !W.have_events) {
    for (auto& e : W.ev) HIPCHECK(hipEventCreate(&e));
    W.have_events = true;
  }
  const uint64_t nd = n_docs;
  const uint32_t ng = (uint32_t)((nd + 1023) / 1024), g1024 = (uint32_t)((nd + 1 + 1023) / 1024);
  int rc = BatchWs::ensure(W.ctr, FC_N * 8);
  for (BatchWs::Buf* b : {&W.fb, &W.fe}) if (!rc) rc = BatchWs::ensure(*b, nd * 8);
  for (BatchWs::Buf* b : {&W.coff, &W.poff}) if (!rc) rc = BatchWs::ensure(*b, (nd + 1) * 8);
  if (!rc) rc = BatchWs::ensure(W.len, nd * sizeof(BDoc));
  for (BatchWs::Buf* b : {&W.wsum, &W.woff}) if (!rc) rc = BatchWs::ensure(*b, (size_t)g1024 * 8);
  if (!rc) rc = BatchWs::ensure(W.flags, sizeof(Flags));
  if (rc) return rc;
  unsigned long long* ctr = (unsigned long long*)W.ctr.p;
  unsigned long long *fb = (unsigned long long*)W.fb.p, *fe = (unsigned long long*)W.fe.p, *coff = (unsigned long long*)W.coff.p,
                     *poff = (unsigned long long*)W.poff.p;
  BDoc* len = (BDoc*)W.len.p;
  Flags* fl = (Flags*)W.flags.p;
  const unsigned long long* off = (const unsigned long long*)d_in_off;
  FSpec F{f->field, f->sep_len, f->last_whole ? nd - 1 : FLD_NONE, f->fs, f->quote < 0 ? 256u : (uint32_t)f->quote,
          f->escape < 0 ? 256u : (uint32_t)f->escape, f->keep_sep ? 1u : 0u};
  unsigned long long sfx8 = 0;
  for (uint32_t i = 0; i < f->suffix_len; ++i) sfx8 |= (unsigned long long)f->suffix[i] << (8 * i);
  // the offsets, checked on the device before any kernel reads a record
  HIPCHECK(hipMemsetAsync(ctr, 0, FC_N * 8, sm));
  hipLaunchKernelGGL(k_fcheck, dim3((uint32_t)((nd + 255) / 256)), dim3(256), 0, sm, off, (unsigned long long)nd, F, ctr);
  HIPCHECK(hipGetLastError());
  unsigned long long hc[FC_N] = {}, ends[2] = {0, 0};
  HIPCHECK(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(&ends[0], d_in_off, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(&ends[1], d_in_off + nd, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  if (hc[FC_BADOFF] || ends[1] < ends[0]) return setErr(KX_E_ARG, "kx_run_batch_fields: the document offsets decrease");
  if (hc[FC_SHORT]) return setErr(KX_E_ARG, "kx_run_batch_fields: a record's range is shorter than its separator");
  if (ends[1] > ends[0] && !d_in) return setErr(KX_E_ARG, "kx_run_batch_fields: null input");
  const uint8_t* in = (const uint8_t*)d_in;
  const uint32_t bgrid = (uint32_t)std::min<uint64_t>((nd + FLD_BT - 1) / FLD_BT, (uint64_t)p->ncu * 4);
  auto granGrid = [&](unsigned long long bytes) {
    const unsigned long long g = ((bytes + 31) / 16 + FLD_GT - 1) / FLD_GT;
    return dim3((uint32_t)std::min<unsigned long long>(g ? g : 1, (unsigned long long)p->ncu * 16));
  };
  // exclusive scan of the lengths in `len` into o (o[nd] = the total, also left in Flags::total_len)
  auto scanLens = [&](unsigned long long* o) {
    hipLaunchKernelGGL(k_bscan_reduce, dim3(ng), dim3(1024), 0, sm, (unsigned long long)nd, (const BDoc*)len, (unsigned long long*)W.wsum.p,
                       (const kx_batch_doc*)d_docs, 0ull);
    hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(1024), 0, sm, ng, (const unsigned long long*)W.wsum.p, (unsigned long long*)W.woff.p, fl);
    hipLaunchKernelGGL(k_bscan_down, dim3(g1024), dim3(1024), 0, sm, (unsigned long long)nd, (const BDoc*)len, (const unsigned long long*)W.woff.p,
                       (const Flags*)fl, o, (const kx_batch_doc*)d_docs, 0ull);
  };
  // 1. the fields, and their scan
  if (timing) HIPCHECK(hipEventRecord(W.ev[0], sm));
  auto* const locate = f->escape >= 0 ? &k_flocate<FLD_ESCAPED> : f->quote >= 0 ? &k_flocate<FLD_QUOTED> : &k_flocate<FLD_PLAIN>;
  hipLaunchKernelGGL(locate, dim3(bgrid), dim3(FLD_BT), 0, sm, in, off, (unsigned long long)nd, F, fb, fe, len);
  if (timing) HIPCHECK(hipEventRecord(W.ev[1], sm));
  scanLens(coff);
  if (timing) HIPCHECK(hipEventRecord(W.ev[2], sm));
  HIPCHECK(hipGetLastError());
  unsigned long long ctotal = 0;
  HIPCHECK(hipMemcpyAsync(&ctotal, &fl->total_len, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  // 2. the compact buffer
  rc = BatchWs::ensure(W.comp, ctotal + 32);
  if (rc) return rc;
  if (timing) HIPCHECK(hipEventRecord(W.ev[3], sm));
  hipLaunchKernelGGL(k_fgather, granGrid(ctotal), dim3(FLD_GT), 0, sm, in, (const unsigned long long*)fb, (const unsigned long long*)coff,
                     (unsigned long long)nd, ctotal, (uint8_t*)W.comp.p);
  if (timing) HIPCHECK(hipEventRecord(W.ev[4], sm));
  HIPCHECK(hipGetLastError());
  // 3. the program on every field (a record without the field: an empty document, its result overwritten below)
  kx_batch_stats bst{};
  size_t pl = 0;
  rc = BatchWs::ensure(W.pout, ctotal + ctotal / 2 + 4096);
  if (rc) return rc;
  rc = kx_run_batch(p, W.comp.p, (const uint64_t*)coff, nd, W.pout.p, W.pout.cap, (uint64_t*)poff, d_docs, &pl, &bst, stream);
  if (rc == KX_E_CAPACITY) {
    rc = BatchWs::ensure(W.pout, pl + 16);
    if (rc) return rc;
    rc = kx_run_batch(p, W.comp.p, (const uint64_t*)coff, nd, W.pout.p, W.pout.cap, (uint64_t*)poff, d_docs, &pl, &bst, stream);
  }
  if (rc != 0 && rc != KX_MATCH_ERROR) return rc;
  // 4. the records' output lengths, and their scan into the caller's offsets
  if (timing) HIPCHECK(hipEventRecord(W.ev[5], sm));
  hipLaunchKernelGGL(k_fsplen, dim3(bgrid), dim3(FLD_BT), 0, sm, off, (unsigned long long)nd, F, (const unsigned long long*)fb,
                     (const unsigned long long*)fe, (const unsigned long long*)poff, d_docs, (unsigned long long)f->suffix_len, len, ctr);
  scanLens((unsigned long long*)d_out_off);
  if (timing) HIPCHECK(hipEventRecord(W.ev[6], sm));
  HIPCHECK(hipGetLastError());
  unsigned long long total = 0, rej = 0;
  HIPCHECK(hipMemcpyAsync(&total, &fl->total_len, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(&rej, ctr + FC_REJECTED, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  *out_len = total;
  bst.docs_rejected = rej;
  bst.in_bytes = ends[1] - ends[0];
  bst.out_bytes = total;
  if (stats) *stats = bst;
  if (total > cap || (total && !d_out)) return setErr(KX_E_CAPACITY, "output buffer too small");
  // 5. the splice
  if (timing) HIPCHECK(hipEventRecord(W.ev[7], sm));
  if (total)
    hipLaunchKernelGGL(k_fsplice, granGrid(total), dim3(FLD_GT), 0, sm, in, off, (unsigned long long)nd, F, (const unsigned long long*)fb,
                       (const unsigned long long*)fe, (const uint8_t*)W.pout.p, (const unsigned long long*)poff,
                       (const unsigned long long*)d_out_off, total, sfx8, (uint8_t*)d_out);
  if (timing) HIPCHECK(hipEventRecord(W.ev[8], sm));
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(sm));
  if (timing) {
    W.locate_ms += evMs(W.ev[0], W.ev[1]);
    W.scan_ms += evMs(W.ev[1], W.ev[2]) + evMs(W.ev[5], W.ev[6]);   // (the second with k_fsplen, which feeds it)
    W.gather_ms += evMs(W.ev[3], W.ev[4]);
    W.splice_ms += evMs(W.ev[7], W.ev[8]);
    ++W.calls;
  }
  return rej ? KX_MATCH_ERROR : 0;
}

extern "C" int kx_fields_stats(const kx_program* p, kx_fields_kernel_stats* out) {
  if (!p || !out) return setErr(KX_E_ARG, "null argument");
  kx_fields_kernel_stats s{};
  if (p->fields) {
    const FieldWs& W = *p->fields;
    s.locate_ms = W.locate_ms; s.gather_ms = W.gather_ms; s.scan_ms = W.scan_ms; s.splice_ms = W.splice_ms; s.calls = W.calls;
  }
  *out = s;
  return 0;
}
