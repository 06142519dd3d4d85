// kx_records_host.inc — host side of record mode (include/kxhip.h: kx_split_records, kx_run_records_fd; kernels in
// kx_records.inc).  Included at the end of kx_engine.hip, behind kx_batch_host.inc.
//
// kx_run_records_fd reuses FdStream's reader and writer threads and its buffer pool (kx_run_fd); only the compute step differs.
// Windows are independent: per window, kx_split_records → kx_run_batch over the complete records → one output window → one
// report line per rejected record.  The record that straddles a window's end is carried (device memory, grown as needed) and
// run as a one-document batch in front of the next window's records.  With a quote byte (kx_run_records_fd_quoted) the split is
// kx_split_records_quoted, and the quote parity at the end of each window is the parity_in of the next; nothing else differs.
// With an escape byte (kx_run_records_fd_escaped) the split is kx_split_records_escaped, and the state it ends in (quote parity,
// escape) is the state_in of the next window's split.  With a multi-byte separator (kx_run_records_fd_rs) the split is
// kx_split_records_rs, and the context it leaves (the last bytes of the unfinished record, fewer than the separator has) is the
// context of the next window's split: a separator may straddle windows, and the carried record is then completed by a first
// record that may be a single byte long.
//
// Framing (kx_run_records_fd_opts): with `chomp` every batch is a framed one (kx_run_batch_framed) whose trim is the separator's
// length — the batch kernels run each record without its separator, no byte is moved — and with `ors` its suffix is the output
// separator.  Only the stream's tail keeps its whole range: the last window's batch has last_whole = 1 when the split reported a
// tail, and the carried record is left whole when it is that tail (the last window brought no separator).  The splitters know
// nothing of this.

namespace {

struct RecWs {   // grow-only device workspace of a split (tile counts, their offsets, the scan's Flags)
  BatchWs::Buf tcount, toff, flags;
  ~RecWs() { for (BatchWs::Buf* b : {&tcount, &toff, &flags}) if (b->p) (void)hipFree(b->p); }
};

// the split; *nsep = separators in the buffer, *nrec = records (nsep, or nsep + 1 with a non-empty tail)
int splitRecords(const uint8_t* d_in, size_t n, uint8_t sep, uint64_t base, uint64_t* d_off, uint64_t cap, uint64_t* nrec,
                 uint64_t* nsep, RecWs& W, hipStream_t sm) {
  *nrec = 0; *nsep = 0;
  if (n == 0) {
    if (cap < 1) return setErr(KX_E_CAPACITY, "kx_split_records: offsets buffer too small");
    HIPCHECK(hipMemcpyAsync(d_off, &base, 8, hipMemcpyHostToDevice, sm));
    HIPCHECK(hipStreamSynchronize(sm));
    return 0;
  }
  const uint8_t* a0 = (const uint8_t*)((uintptr_t)d_in & ~(uintptr_t)15);
  const unsigned long long lo = (unsigned long long)(d_in - a0), hi = lo + n, ng = (hi + 15) / 16;
  const unsigned long long ntiles = (ng + REC_TILE - 1) / REC_TILE;
  if (ntiles > 0x7FFFFFFFull) return setErr(KX_E_ARG, "kx_split_records: buffer too large");
  int rc = BatchWs::ensure(W.tcount, ntiles * 8);
  if (!rc) rc = BatchWs::ensure(W.toff, ntiles * 8);
  if (!rc) rc = BatchWs::ensure(W.flags, sizeof(Flags));
  if (rc) return rc;
  const uint32_t pat = 0x01010101u * sep;
  hipLaunchKernelGGL(k_rcount, dim3((uint32_t)ntiles), dim3(REC_BT), 0, sm, a0, ng, lo, hi, pat, (unsigned long long*)W.tcount.p);
  hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(1024), 0, sm, (uint32_t)ntiles, (const unsigned long long*)W.tcount.p,
                     (unsigned long long*)W.toff.p, (Flags*)W.flags.p);
  HIPCHECK(hipGetLastError());
  unsigned long long total = 0;
  uint8_t lastb = 0;
  HIPCHECK(hipMemcpyAsync(&total, &((Flags*)W.flags.p)->total_len, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(&lastb, d_in + n - 1, 1, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  const int tail = lastb != sep;
  *nsep = total;
  *nrec = total + (uint64_t)tail;
  if (cap < *nrec + 1 || !d_off) return setErr(KX_E_CAPACITY, "kx_split_records: offsets buffer too small");
  hipLaunchKernelGGL(k_rwrite, dim3((uint32_t)ntiles), dim3(REC_BT), 0, sm, a0, ng, lo, hi, pat, (const unsigned long long*)W.toff.p,
                     (unsigned long long)base, total, tail, (unsigned long long*)d_off);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(sm));
  return 0;
}

struct RecQWs {   // grow-only device workspace of a quoted split: RecWs (tcount = the selected counts) plus the per-tile quote counts,
                  // their scan, the separators and the separators outside quotes from an even start; flags holds two Flags
  RecWs base;
  BatchWs::Buf tq, tqoff, tsep, teven;
  ~RecQWs() { for (BatchWs::Buf* b : {&tq, &tqoff, &tsep, &teven}) if (b->p) (void)hipFree(b->p); }
};

// the quoted split (quote != sep, parity_in ≤ 1); *nsep = separators outside quotes, *nrec = records, *parity_out = parity_in ^ the
// quote count's parity
int splitRecordsQuoted(const uint8_t* d_in, size_t n, uint8_t sep, uint8_t quote, uint32_t parity_in, uint64_t base, uint64_t* d_off,
                       uint64_t cap, uint64_t* nrec, uint64_t* nsep, uint32_t* parity_out, RecQWs& W, hipStream_t sm) {
  *nrec = 0; *nsep = 0; *parity_out = parity_in;
  if (n == 0) {
    if (cap < 1) return setErr(KX_E_CAPACITY, "kx_split_records_quoted: offsets buffer too small");
    HIPCHECK(hipMemcpyAsync(d_off, &base, 8, hipMemcpyHostToDevice, sm));
    HIPCHECK(hipStreamSynchronize(sm));
    return 0;
  }
  const uint8_t* a0 = (const uint8_t*)((uintptr_t)d_in & ~(uintptr_t)15);
  const unsigned long long lo = (unsigned long long)(d_in - a0), hi = lo + n, ng = (hi + 15) / 16;
  const unsigned long long ntiles = (ng + REC_TILE - 1) / REC_TILE;
  if (ntiles > 0x7FFFFFFFull) return setErr(KX_E_ARG, "kx_split_records_quoted: buffer too large");
  int rc = 0;
  for (BatchWs::Buf* b : {&W.base.tcount, &W.base.toff, &W.tq, &W.tqoff, &W.tsep, &W.teven}) if (!rc) rc = BatchWs::ensure(*b, ntiles * 8);
  if (!rc) rc = BatchWs::ensure(W.base.flags, 2 * sizeof(Flags));
  if (rc) return rc;
  const uint32_t spat = 0x01010101u * sep, qpat = 0x01010101u * quote;
  auto U = [](BatchWs::Buf& b) { return (unsigned long long*)b.p; };
  Flags* fl = (Flags*)W.base.flags.p;
  hipLaunchKernelGGL(k_rqcount, dim3((uint32_t)ntiles), dim3(REC_BT), 0, sm, a0, ng, lo, hi, spat, qpat, U(W.tq), U(W.tsep), U(W.teven));
  hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(1024), 0, sm, (uint32_t)ntiles, (const unsigned long long*)W.tq.p, U(W.tqoff), fl);
  hipLaunchKernelGGL(k_rqselect, dim3((uint32_t)((ntiles + 255) / 256)), dim3(256), 0, sm, (uint32_t)ntiles, (const unsigned long long*)W.tqoff.p,
                     (const unsigned long long*)W.tsep.p, (const unsigned long long*)W.teven.p, parity_in, U(W.base.tcount));
  hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(1024), 0, sm, (uint32_t)ntiles, (const unsigned long long*)W.base.tcount.p, U(W.base.toff),
                     fl + 1);
  HIPCHECK(hipGetLastError());
  unsigned long long quotes = 0, total = 0;
  uint8_t lastb = 0;
  HIPCHECK(hipMemcpyAsync(&quotes, &fl[0].total_len, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(&total, &fl[1].total_len, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(&lastb, d_in + n - 1, 1, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  *parity_out = parity_in ^ (uint32_t)(quotes & 1u);
  const int tail = !(lastb == sep && *parity_out == 0);   // (a last separator byte inside quotes ends no record)
  *nsep = total;
  *nrec = total + (uint64_t)tail;
  if (cap < *nrec + 1 || !d_off) return setErr(KX_E_CAPACITY, "kx_split_records_quoted: offsets buffer too small");
  hipLaunchKernelGGL(k_rqwrite, dim3((uint32_t)ntiles), dim3(REC_BT), 0, sm, a0, ng, lo, hi, spat, qpat, (const unsigned long long*)W.tqoff.p,
                     parity_in, (const unsigned long long*)W.base.toff.p, (unsigned long long)base, total, tail, (unsigned long long*)d_off);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(sm));
  return 0;
}

struct RecEWs {   // grow-only device workspace of an escaped split: RecQWs plus the per-tile flag words and the info word
  RecQWs q;
  BatchWs::Buf tflag, info;
  ~RecEWs() { for (BatchWs::Buf* b : {&tflag, &info}) if (b->p) (void)hipFree(b->p); }
};

// the escaped split (escape != sep, escape != quote, quote != sep; quote < 0: none; state_in ≤ 3, bit 0 only with a quote);
// *nsep = valid separators, *nrec = records, *state_out = the quote parity (bit 0) and the escape state (bit 1) after the buffer
int splitRecordsEscaped(const uint8_t* d_in, size_t n, uint8_t sep, int quote, uint8_t escape, uint32_t state_in, uint64_t base,
                        uint64_t* d_off, uint64_t cap, uint64_t* nrec, uint64_t* nsep, uint32_t* state_out, RecEWs& W, hipStream_t sm) {
  *nrec = 0; *nsep = 0; *state_out = state_in;
  if (n == 0) {
    if (cap < 1) return setErr(KX_E_CAPACITY, "kx_split_records_escaped: offsets buffer too small");
    HIPCHECK(hipMemcpyAsync(d_off, &base, 8, hipMemcpyHostToDevice, sm));
    HIPCHECK(hipStreamSynchronize(sm));
    return 0;
  }
  const uint8_t* a0 = (const uint8_t*)((uintptr_t)d_in & ~(uintptr_t)15);
  const unsigned long long lo = (unsigned long long)(d_in - a0), hi = lo + n, ng = (hi + 15) / 16;
  const unsigned long long ntiles = (ng + REC_TILE - 1) / REC_TILE;
  if (ntiles > 0x7FFFFFFFull) return setErr(KX_E_ARG, "kx_split_records_escaped: buffer too large");
  RecQWs& Q = W.q;
  int rc = 0;
  for (BatchWs::Buf* b : {&Q.base.tcount, &Q.base.toff, &Q.tq, &Q.tqoff, &Q.tsep, &Q.teven}) if (!rc) rc = BatchWs::ensure(*b, ntiles * 8);
  if (!rc) rc = BatchWs::ensure(Q.base.flags, 2 * sizeof(Flags));
  if (!rc) rc = BatchWs::ensure(W.tflag, ntiles * 4);
  if (!rc) rc = BatchWs::ensure(W.info, 4);
  if (rc) return rc;
  const uint32_t spat = 0x01010101u * sep, qpat = 0x01010101u * (uint8_t)(quote < 0 ? 0 : quote), epat = 0x01010101u * escape;
  const uint32_t qkeep = quote < 0 ? 0u : 0xFFFF0000u, x = state_in >> 1, parity_in = state_in & 1u;
  auto U = [](BatchWs::Buf& b) { return (unsigned long long*)b.p; };
  auto C = [](BatchWs::Buf& b) { return (const unsigned long long*)b.p; };
  Flags* fl = (Flags*)Q.base.flags.p;
  uint32_t* tflag = (uint32_t*)W.tflag.p;
  hipLaunchKernelGGL(k_recount, dim3((uint32_t)ntiles), dim3(REC_BT), 0, sm, a0, ng, lo, hi, spat, qpat, qkeep, epat, x, U(Q.tq), U(Q.tsep),
                     U(Q.teven), tflag);
  hipLaunchKernelGGL(k_rescan, dim3(1), dim3(1024), 0, sm, (uint32_t)ntiles, lo == 0 ? x : 0u, tflag, U(Q.tq));
  hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(1024), 0, sm, (uint32_t)ntiles, C(Q.tq), U(Q.tqoff), fl);
  hipLaunchKernelGGL(k_reselect, dim3((uint32_t)((ntiles + 255) / 256)), dim3(256), 0, sm, (uint32_t)ntiles, (const uint32_t*)tflag, C(Q.tq),
                     C(Q.tqoff), C(Q.tsep), C(Q.teven), parity_in, U(Q.base.tcount), (uint32_t*)W.info.p);
  hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(1024), 0, sm, (uint32_t)ntiles, C(Q.base.tcount), U(Q.base.toff), fl + 1);
  HIPCHECK(hipGetLastError());
  unsigned long long total = 0;
  uint32_t info = 0;
  HIPCHECK(hipMemcpyAsync(&total, &fl[1].total_len, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(&info, W.info.p, 4, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  *state_out = (info >> 1) & 3u;
  const int tail = !(info & 1u);   // (an escaped separator, or one inside quotes, as the last byte ends no record)
  *nsep = total;
  *nrec = total + (uint64_t)tail;
  if (cap < *nrec + 1 || !d_off) return setErr(KX_E_CAPACITY, "kx_split_records_escaped: offsets buffer too small");
  hipLaunchKernelGGL(k_rewrite, dim3((uint32_t)ntiles), dim3(REC_BT), 0, sm, a0, ng, lo, hi, spat, qpat, qkeep, epat, x, (const uint32_t*)tflag,
                     C(Q.tqoff), parity_in, C(Q.base.toff), (unsigned long long)base, total, tail, (unsigned long long*)d_off);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(sm));
  return 0;
}

struct RecRsWs {   // grow-only device workspace of a multi-byte split: RecWs plus the per-tile maps / states, counts per state, info
  RecWs base;
  BatchWs::Buf tmap, tcnt, info;
  ~RecRsWs() { for (BatchWs::Buf* b : {&tmap, &tcnt, &info}) if (b->p) (void)hipFree(b->p); }
};

// no proper prefix of rs is also a suffix: copies of rs cannot overlap
bool rsBorderFree(const uint8_t* rs, uint32_t m) {
  for (uint32_t b = 1; b < m; ++b) if (!memcmp(rs, rs + m - b, b)) return false;
  return true;
}

// the multi-byte split (1 ≤ m ≤ 8, k < m; rs, ctx, ctx_out host memory); *nsep = selected separators, *nrec = records.  On
// success *ctx_out_len bytes of ctx_out (7 bytes) = the context for the buffer behind this one and *tail_len = the bytes of this
// buffer behind its last selected separator (host.split_rs_records_model).
int splitRecordsRs(const uint8_t* d_in, size_t n, const uint8_t* rs, uint32_t m, const uint8_t* ctx, uint32_t k, uint64_t base,
                   uint64_t* d_off, uint64_t cap, uint64_t* nrec, uint64_t* nsep, uint8_t* ctx_out, uint32_t* ctx_out_len, uint64_t* tail_len,
                   RecRsWs& W, hipStream_t sm) {
  *nrec = 0; *nsep = 0;
  if (n == 0) {
    if (cap < 1) return setErr(KX_E_CAPACITY, "kx_split_records_rs: offsets buffer too small");
    HIPCHECK(hipMemcpyAsync(d_off, &base, 8, hipMemcpyHostToDevice, sm));
    HIPCHECK(hipStreamSynchronize(sm));
    memmove(ctx_out, ctx, k);
    *ctx_out_len = k;
    *tail_len = 0;
    return 0;
  }
  const uint8_t* a0 = (const uint8_t*)((uintptr_t)d_in & ~(uintptr_t)15);
  const unsigned long long lo = (unsigned long long)(d_in - a0), hi = lo + n, ng = (hi + 15) / 16;
  const unsigned long long ntiles = (ng + REC_TILE - 1) / REC_TILE;
  if (ntiles > 0x7FFFFFFFull) return setErr(KX_E_ARG, "kx_split_records_rs: buffer too large");
  const bool overlap = !rsBorderFree(rs, m);
  int rc = BatchWs::ensure(W.base.tcount, ntiles * 8);
  if (!rc) rc = BatchWs::ensure(W.base.toff, ntiles * 8);
  if (!rc) rc = BatchWs::ensure(W.base.flags, sizeof(Flags));
  if (!rc && overlap) rc = BatchWs::ensure(W.tmap, ntiles * 4);
  if (!rc && overlap) rc = BatchWs::ensure(W.tcnt, ntiles * 32);
  if (!rc && overlap) rc = BatchWs::ensure(W.info, 4);
  if (rc) return rc;
  unsigned long long rs8 = 0, ctx8 = 0;
  for (uint32_t i = 0; i < m; ++i) rs8 |= (unsigned long long)rs[i] << (8 * i);
  for (uint32_t i = 0; i < k; ++i) ctx8 |= (unsigned long long)ctx[i] << (8 * i);
  unsigned long long* tcount = (unsigned long long*)W.base.tcount.p;
  unsigned long long* toff = (unsigned long long*)W.base.toff.p;
  if (overlap) {
    hipLaunchKernelGGL(k_rocount, dim3((uint32_t)ntiles), dim3(REC_BT), 0, sm, a0, ng, lo, hi, rs8, m, ctx8, k, (uint32_t*)W.tmap.p,
                       (uint32_t*)W.tcnt.p);
    hipLaunchKernelGGL(k_rsscan, dim3(1), dim3(1024), 0, sm, (uint32_t)ntiles, m, (uint32_t*)W.tmap.p, (const uint32_t*)W.tcnt.p, tcount,
                       (uint32_t*)W.info.p);
  } else {
    hipLaunchKernelGGL(k_rbcount, dim3((uint32_t)ntiles), dim3(REC_BT), 0, sm, a0, ng, lo, hi, rs8, m, ctx8, k, tcount);
  }
  hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(1024), 0, sm, (uint32_t)ntiles, (const unsigned long long*)tcount, toff, (Flags*)W.base.flags.p);
  HIPCHECK(hipGetLastError());
  unsigned long long total = 0;
  uint32_t info = 0;
  uint8_t endb[16] = {};   // the context, then the buffer's last nl bytes: every byte that ctx_out or the last candidate can hold
  const size_t nl = n < 8 ? n : 8;
  memcpy(endb, ctx, k);
  HIPCHECK(hipMemcpyAsync(&total, &((Flags*)W.base.flags.p)->total_len, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(endb + k, d_in + n - nl, nl, hipMemcpyDeviceToHost, sm));
  if (overlap) HIPCHECK(hipMemcpyAsync(&info, W.info.p, 4, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  const uint8_t* end = endb + k + nl;                                   // (behind the buffer's last byte)
  const size_t known = n < 8 ? k + n : 8;                               // bytes before `end` that belong to the unfinished record or the buffer
  // border-free: every copy is selected, so the buffer ends in a separator iff its last m bytes (the context's included) are rs
  const int tail = overlap ? !(info & 1u) : !(known >= m && !memcmp(end - m, rs, m));
  *nsep = total;
  *nrec = total + (uint64_t)tail;
  if (cap < *nrec + 1 || !d_off) return setErr(KX_E_CAPACITY, "kx_split_records_rs: offsets buffer too small");
  if (overlap)
    hipLaunchKernelGGL(k_rowrite, dim3((uint32_t)ntiles), dim3(REC_BT), 0, sm, a0, ng, lo, hi, rs8, m, ctx8, k, (const uint32_t*)W.tmap.p,
                       (const unsigned long long*)toff, (unsigned long long)base, total, tail, (unsigned long long*)d_off);
  else
    hipLaunchKernelGGL(k_rbwrite, dim3((uint32_t)ntiles), dim3(REC_BT), 0, sm, a0, ng, lo, hi, rs8, m, ctx8, k, (const unsigned long long*)toff,
                       (unsigned long long)base, total, tail, (unsigned long long*)d_off);
  HIPCHECK(hipGetLastError());
  uint64_t e = base;   // the last selected separator's end
  if (tail && total) HIPCHECK(hipMemcpyAsync(&e, d_off + total, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  const uint64_t tl = tail ? n - (e - base) : 0;
  size_t unfinished = total ? tl : k + n;                               // the unfinished record so far (without a separator: the context's bytes too)
  if (!tail) unfinished = 0;
  const size_t co = unfinished < m - 1 ? unfinished : m - 1;            // (≤ 7 ≤ known whenever unfinished ≥ 7)
  uint8_t tmp[8];
  memcpy(tmp, end - co, co);
  memcpy(ctx_out, tmp, co);
  *ctx_out_len = (uint32_t)co;
  *tail_len = tl;
  return 0;
}

// the compute step of kx_run_records_fd, kx_run_records_fd_quoted and kx_run_records_fd_escaped
struct RecordsRun {
  kx_program* p = nullptr;
  FdStream* fs = nullptr;
  uint8_t sep = '\n';
  int quote = -1;                                      // the quote byte, -1: none (kx_run_records_fd)
  int escape = -1;                                     // the escape byte, -1: none
  uint32_t state = 0;                                  // at the start of the next window: bit 0 quote parity, bit 1 escaped
  uint8_t rs[8] = {}, ctx[8] = {};                     // the multi-byte separator (kx_run_records_fd_rs) and the next window's context
  uint32_t rs_len = 0, ctx_len = 0;                    // rs_len 0: a one-byte mode
  bool chomp = false;                                  // records run without their separator
  uint8_t ors[8] = {};                                 // what follows every accepted record's output
  uint32_t ors_len = 0;
  RecQWs qws;
  RecEWs ews;
  RecRsWs rws;
  int report_fd = -1;
  RecWs ws;
  BatchWs::Buf off, ooff, docs, carry, one, longest;   // offsets; output offsets; doc records; the straddling record; its offsets
  uint64_t carry_len = 0, recno = 0;                   // records reported so far (R of the next record is recno + 1)
  double ratio = 4.0;                                  // output bytes per input byte, from the previous window
  bool rejected = false;
  kx_records_stats st{};
  hipEvent_t ev[4] = {};
  bool timing = false;

  ~RecordsRun() {
    for (BatchWs::Buf* b : {&off, &ooff, &docs, &carry, &one, &longest}) if (b->p) (void)hipFree(b->p);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
  }

  int report(const kx_batch_doc* d, uint64_t n, uint64_t first_rec) {
    if (report_fd < 0) return 0;
    std::string s;
    for (uint64_t i = 0; i < n; ++i)
      if (d[i].status) s += "Match error at input symbol " + std::to_string(d[i].fail_pos) + " in record " + std::to_string(first_rec + i) + "!\n";
    for (size_t w = 0; w < s.size();) {
      const ssize_t r = write(report_fd, s.data() + w, s.size() - w);
      if (r < 0) { if (errno == EINTR) continue; return setErr(KX_E_IO, "write of the record report failed"); }
      w += (size_t)r;
    }
    return 0;
  }

  // kx_run_batch of ndocs records (offsets d_o) into *out at byte pos; a buffer too small is replaced by one of the size needed,
  // its first pos bytes kept.  Reports the rejected records (numbered from first_rec) and advances *pos.  tail: the last of
  // these records is the stream's tail (it has no separator to strip).
  int batch(const uint8_t* in, const uint64_t* d_o, uint64_t ndocs, DevBuf* out, size_t* pos, uint64_t first_rec, bool tail) {
    if (ndocs == 0) return 0;
    kx_batch_frame fr{};
    fr.trim = chomp ? (rs_len ? rs_len : 1u) : 0u;
    fr.last_whole = tail ? 1u : 0u;
    fr.suffix_len = ors_len;
    memcpy(fr.suffix, ors, ors_len);
    const kx_batch_frame* frp = fr.trim || fr.suffix_len ? &fr : nullptr;
    int rc = BatchWs::ensure(ooff, (ndocs + 1) * 8);
    if (!rc) rc = BatchWs::ensure(docs, ndocs * sizeof(kx_batch_doc));
    if (rc) return rc;
    kx_batch_stats bs{};
    size_t ol = 0;
    if (timing) HIPCHECK(hipEventRecord(ev[2], nullptr));
    rc = kx_run_batch_framed(p, in, d_o, ndocs, frp, out->d + *pos, out->cap - *pos, (uint64_t*)ooff.p, (kx_batch_doc*)docs.p, &ol, &bs, nullptr);
    if (rc == KX_E_CAPACITY) {
      DevBuf nb;
      rc = fs->pool.get(*pos + ol + ol / 8 + 4096, &nb);
      if (rc) return rc;
      if (*pos) HIPCHECK(hipMemcpy(nb.d, out->d, *pos, hipMemcpyDeviceToDevice));
      fs->pool.put(*out);
      *out = nb;
      rc = kx_run_batch_framed(p, in, d_o, ndocs, frp, out->d + *pos, out->cap - *pos, (uint64_t*)ooff.p, (kx_batch_doc*)docs.p, &ol, &bs, nullptr);
    }
    if (timing) { HIPCHECK(hipEventRecord(ev[3], nullptr)); HIPCHECK(hipEventSynchronize(ev[3])); st.batch_ms += evMs(ev[2], ev[3]); }
    if (rc != 0 && rc != KX_MATCH_ERROR) return rc;
    st.records += ndocs;
    st.records_routed += bs.docs_routed;
    st.out_bytes += ol;
    *pos += ol;
    if (bs.docs_rejected) {
      rejected = true;
      st.records_rejected += bs.docs_rejected;
      std::vector<kx_batch_doc> h(ndocs);
      HIPCHECK(hipMemcpy(h.data(), docs.p, ndocs * sizeof(kx_batch_doc), hipMemcpyDeviceToHost));
      return report(h.data(), ndocs, first_rec);
    }
    return 0;
  }

  // window b (n bytes; ownership taken)
  int window(DevBuf b, size_t n, bool last) {
    struct PutOnExit { BufPool& pool; DevBuf& b; ~PutOnExit() { pool.put(b); } } put_in{fs->pool, b};
    const uint8_t* in = (const uint8_t*)b.d;
    ++st.windows;
    st.in_bytes += n;
    // 1. the records of the window (offsets relative to b.d)
    uint64_t nrec = 0, nsep = 0;
    if (off.cap < 16) { int rc = BatchWs::ensure(off, (n / 32 + 2) * 8); if (rc) return rc; }
    if (timing) HIPCHECK(hipEventRecord(ev[0], nullptr));
    uint32_t sout = state;
    uint8_t cout[8] = {};
    uint32_t cout_len = 0;
    uint64_t tail_len = 0;
    auto split = [&] {
      if (rs_len)
        return splitRecordsRs(in, n, rs, rs_len, ctx, ctx_len, 0, (uint64_t*)off.p, off.cap / 8, &nrec, &nsep, cout, &cout_len, &tail_len, rws,
                              nullptr);
      if (escape >= 0)
        return splitRecordsEscaped(in, n, sep, quote, (uint8_t)escape, state, 0, (uint64_t*)off.p, off.cap / 8, &nrec, &nsep, &sout, ews, nullptr);
      return quote < 0 ? splitRecords(in, n, sep, 0, (uint64_t*)off.p, off.cap / 8, &nrec, &nsep, ws, nullptr)
                       : splitRecordsQuoted(in, n, sep, (uint8_t)quote, state, 0, (uint64_t*)off.p, off.cap / 8, &nrec, &nsep, &sout, qws, nullptr);
    };
    int rc = split();
    if (rc == KX_E_CAPACITY) {
      rc = BatchWs::ensure(off, (nrec + 1) * 8);
      if (!rc) rc = split();
    }
    if (rc) return rc;
    state = sout;
    memcpy(ctx, cout, 8);
    ctx_len = cout_len;
    if (timing) { HIPCHECK(hipEventRecord(ev[1], nullptr)); HIPCHECK(hipEventSynchronize(ev[1])); st.split_ms += evMs(ev[0], ev[1]); }
    const uint64_t complete = last ? nrec : nsep;   // (a tail that is not the stream's end continues in the next window)
    const uint64_t* d_off = (const uint64_t*)off.p;
    // 2. the carried record: its rest is this window's first record (or all of the window, if it holds no separator)
    if (carry_len && complete == 0 && !last) {
      rc = BatchWs::grow(carry, carry_len, carry_len + n, nullptr);
      if (!rc && n) HIPCHECK(hipMemcpy((uint8_t*)carry.p + carry_len, in, n, hipMemcpyDeviceToDevice));
      if (rc) return rc;
      carry_len += n;
      st.longest_record = carry_len > st.longest_record ? carry_len : st.longest_record;
      return 0;
    }
    DevBuf out;
    const size_t est = (size_t)((double)(n + carry_len) * ratio) + 4096;
    rc = fs->pool.get(est, &out);
    if (rc) return rc;
    struct PutOut { BufPool& pool; DevBuf& b; bool own = true; ~PutOut() { if (own) pool.put(b); } } put_out{fs->pool, out};
    size_t pos = 0;
    uint64_t first = 0;
    const uint64_t in_used = n + carry_len;
    if (carry_len) {
      uint64_t e = 0;
      if (complete) HIPCHECK(hipMemcpy(&e, d_off + 1, 8, hipMemcpyDeviceToHost));
      rc = BatchWs::grow(carry, carry_len, carry_len + e, nullptr);
      if (!rc) rc = BatchWs::ensure(one, 16);
      if (rc) return rc;
      if (e) HIPCHECK(hipMemcpy((uint8_t*)carry.p + carry_len, in, e, hipMemcpyDeviceToDevice));
      carry_len += e;
      const uint64_t o2[2] = {0, carry_len};
      HIPCHECK(hipMemcpy(one.p, o2, 16, hipMemcpyHostToDevice));
      st.longest_record = carry_len > st.longest_record ? carry_len : st.longest_record;
      rc = batch((const uint8_t*)carry.p, (const uint64_t*)one.p, 1, &out, &pos, recno + 1, last && nsep == 0);   // (no separator ever came: the tail)
      if (rc) return rc;
      ++recno;
      carry_len = 0;
      first = complete ? 1 : 0;
    }
    // 3. the window's complete records
    const uint64_t nd = complete - first;
    if (nd) {
      rc = BatchWs::ensure(longest, 8);
      if (rc) return rc;
      HIPCHECK(hipMemsetAsync(longest.p, 0, 8, nullptr));
      const uint64_t g = (nd + 255) / 256;
      hipLaunchKernelGGL(k_rlongest, dim3((uint32_t)(g < 1024 ? g : 1024)), dim3(256), 0, nullptr, (const unsigned long long*)(d_off + first),
                         (unsigned long long)nd, (unsigned long long*)longest.p);
      HIPCHECK(hipGetLastError());
      rc = batch(in, d_off + first, nd, &out, &pos, recno + 1, last && nrec > nsep);
      if (rc) return rc;
      recno += nd;
      uint64_t lr = 0;
      HIPCHECK(hipMemcpy(&lr, longest.p, 8, hipMemcpyDeviceToHost));
      st.longest_record = lr > st.longest_record ? lr : st.longest_record;
    }
    // 4. the tail that continues in the next window
    if (!last && nrec > nsep) {
      uint64_t s = 0;
      HIPCHECK(hipMemcpy(&s, d_off + nsep, 8, hipMemcpyDeviceToHost));
      carry_len = n - s;
      rc = BatchWs::grow(carry, 0, carry_len, nullptr);
      if (rc) return rc;
      HIPCHECK(hipMemcpy(carry.p, in + s, carry_len, hipMemcpyDeviceToDevice));
    }
    // 5. the output window
    const uint64_t used = in_used - carry_len;
    if (used) ratio = (double)pos / (double)used * 1.0625;
    if (pos == 0) return 0;
    put_out.own = false;
    if (!fs->outq.push(FdStream::OutWin{out, pos})) { fs->pool.put(out); return KX_E_IO; }   // (closed: the writer failed; its error is reported)
    return 0;
  }
};

}  // namespace

extern "C" int kx_split_records(const void* d_in, size_t n, uint8_t sep, uint64_t base, uint64_t* d_off, uint64_t cap, uint64_t* n_records,
                                void* stream) {
  if (!n_records) return setErr(KX_E_ARG, "null argument");
  *n_records = 0;
  if (n && !d_in) return setErr(KX_E_ARG, "kx_split_records: null input");
  if (cap && !d_off) return setErr(KX_E_ARG, "kx_split_records: null offsets with a capacity");
  RecWs ws;
  uint64_t nsep = 0;
  return splitRecords((const uint8_t*)d_in, n, sep, base, d_off, cap, n_records, &nsep, ws, (hipStream_t)stream);
}

extern "C" int kx_split_records_quoted(const void* d_in, size_t n, uint8_t sep, uint8_t quote, uint32_t parity_in, uint64_t base,
                                       uint64_t* d_off, uint64_t cap, uint64_t* n_records, uint32_t* parity_out, void* stream) {
  if (!n_records) return setErr(KX_E_ARG, "null argument");
  *n_records = 0;
  if (parity_out) *parity_out = 0;
  if (quote == sep) return setErr(KX_E_ARG, "kx_split_records_quoted: the quote byte cannot be the separator");
  if (parity_in > 1) return setErr(KX_E_ARG, "kx_split_records_quoted: parity_in must be 0 or 1");
  if (n && !d_in) return setErr(KX_E_ARG, "kx_split_records_quoted: null input");
  if (cap && !d_off) return setErr(KX_E_ARG, "kx_split_records_quoted: null offsets with a capacity");
  RecQWs ws;
  uint64_t nsep = 0;
  uint32_t po = parity_in;
  const int rc = splitRecordsQuoted((const uint8_t*)d_in, n, sep, quote, parity_in, base, d_off, cap, n_records, &nsep, &po, ws,
                                    (hipStream_t)stream);
  if (parity_out && (rc == 0 || rc == KX_E_CAPACITY)) *parity_out = po;
  return rc;
}

extern "C" int kx_split_records_escaped(const void* d_in, size_t n, uint8_t sep, int quote, uint8_t escape, uint32_t state_in, uint64_t base,
                                        uint64_t* d_off, uint64_t cap, uint64_t* n_records, uint32_t* state_out, void* stream) {
  if (!n_records) return setErr(KX_E_ARG, "null argument");
  *n_records = 0;
  if (state_out) *state_out = 0;
  if (quote < -1 || quote > 255) return setErr(KX_E_ARG, "kx_split_records_escaped: quote must be a byte value or -1");
  if (quote == sep) return setErr(KX_E_ARG, "kx_split_records_escaped: the quote byte cannot be the separator");
  if (escape == sep) return setErr(KX_E_ARG, "kx_split_records_escaped: the escape byte cannot be the separator");
  if (quote == escape) return setErr(KX_E_ARG, "kx_split_records_escaped: the escape byte cannot be the quote byte");
  if (state_in > 3 || (quote < 0 && (state_in & 1u))) return setErr(KX_E_ARG, "kx_split_records_escaped: state_in must be 0-3, bit 0 only with a quote");
  if (n && !d_in) return setErr(KX_E_ARG, "kx_split_records_escaped: null input");
  if (cap && !d_off) return setErr(KX_E_ARG, "kx_split_records_escaped: null offsets with a capacity");
  RecEWs ws;
  uint64_t nsep = 0;
  uint32_t so = state_in;
  const int rc = splitRecordsEscaped((const uint8_t*)d_in, n, sep, quote, escape, state_in, base, d_off, cap, n_records, &nsep, &so, ws,
                                     (hipStream_t)stream);
  if (state_out && (rc == 0 || rc == KX_E_CAPACITY)) *state_out = so;
  return rc;
}

extern "C" int kx_split_records_rs(const void* d_in, size_t n, const uint8_t* rs, uint32_t rs_len, const uint8_t* ctx_in, uint32_t ctx_in_len,
                                   uint64_t base, uint64_t* d_off, uint64_t cap, uint64_t* n_records, uint8_t* ctx_out, uint32_t* ctx_out_len,
                                   uint64_t* tail_len, void* stream) {
  if (!n_records) return setErr(KX_E_ARG, "null argument");
  *n_records = 0;
  if (ctx_out_len) *ctx_out_len = 0;
  if (tail_len) *tail_len = 0;
  if (!rs || rs_len < 1 || rs_len > 8) return setErr(KX_E_ARG, "kx_split_records_rs: the separator must be 1 to 8 bytes");
  if (ctx_in_len >= rs_len || (ctx_in_len && !ctx_in)) return setErr(KX_E_ARG, "kx_split_records_rs: the context must be shorter than the separator");
  if (n && !d_in) return setErr(KX_E_ARG, "kx_split_records_rs: null input");
  if (cap && !d_off) return setErr(KX_E_ARG, "kx_split_records_rs: null offsets with a capacity");
  RecRsWs ws;
  uint64_t nsep = 0, tl = 0;
  uint8_t co[8] = {}, ci[8] = {};
  uint32_t col = 0;
  if (ctx_in_len) memcpy(ci, ctx_in, ctx_in_len);
  const int rc = splitRecordsRs((const uint8_t*)d_in, n, rs, rs_len, ci, ctx_in_len, base, d_off, cap, n_records, &nsep, co, &col, &tl, ws,
                                (hipStream_t)stream);
  if (rc == 0) {
    if (ctx_out) memcpy(ctx_out, co, col);
    if (ctx_out_len) *ctx_out_len = col;
    if (tail_len) *tail_len = tl;
  }
  return rc;
}

namespace {

// kx_run_records_fd (quote < 0, escape < 0), kx_run_records_fd_quoted (escape < 0), kx_run_records_fd_escaped and, with rs_len > 0,
// kx_run_records_fd_rs (sep, quote and escape unused)
int runRecordsFd(kx_program* p, int in_fd, int out_fd, uint8_t sep, int quote, int escape, int report_fd, kx_records_stats* stats,
                 const uint8_t* rs = nullptr, uint32_t rs_len = 0, bool chomp = false, const uint8_t* ors = nullptr, uint32_t ors_len = 0) {
  if (!p) return setErr(KX_E_ARG, "null argument");
  if (p->cfg.phase) return setErr(KX_E_ARG, "record mode runs every phase: kx_config::phase must be 0");
  const double t_begin = FdStream::nowMs();
  FdStream fsr;
  fsr.p = p; fsr.in_fd = in_fd; fsr.out_fd = out_fd;
  size_t window = p->cfg.window_bytes ? p->cfg.window_bytes : (size_t)1 << 30;
  if (const char* ev = getenv("KX_WINDOW_BYTES")) { long long v = atoll(ev); if (v > 0) window = (size_t)v; }
  if (window < 4096) window = 4096;
  if (fsr.CH > window) fsr.CH = (window + 4095) & ~(size_t)4095;
  fsr.window = (window + fsr.CH - 1) / fsr.CH * fsr.CH;
  (void)hipGetDevice(&fsr.dev);
  RecordsRun R;
  R.p = p; R.fs = &fsr; R.sep = sep; R.quote = quote; R.escape = escape; R.report_fd = report_fd;
  if (rs_len) { memcpy(R.rs, rs, rs_len); R.rs_len = rs_len; }
  R.chomp = chomp;
  if (ors_len) { memcpy(R.ors, ors, ors_len); R.ors_len = ors_len; }
  R.timing = p->cfg.collect_timing != 0;
  int rc = 0;
  if (R.timing) for (auto& e : R.ev) if (hipEventCreate(&e) != hipSuccess) rc = setErr(KX_E_HIP, "hipEventCreate failed");
  std::thread reader([&] { fsr.readerMain(); });
  std::thread writer([&] { fsr.writerMain(); });
  FdStream::InWin w;
  for (;;) {
    const bool ok = !rc && fsr.inq.pop(&w);
    if (!ok) break;
    rc = R.window(w.b, w.n, w.last);
  }
  if (rc) fsr.fail(rc); else fsr.outq.finish();
  reader.join(); writer.join();
  R.st.total_ms = (float)(FdStream::nowMs() - t_begin);
  if (stats) *stats = R.st;
  if (rc) return rc;
  if (fsr.err) { g_err = fsr.emsg; return fsr.err; }   // (the first error, whichever thread met it)
  return R.rejected ? KX_MATCH_ERROR : 0;
}

}  // namespace

extern "C" int kx_run_records_fd(kx_program* p, int in_fd, int out_fd, uint8_t sep, int report_fd, kx_records_stats* stats) {
  return runRecordsFd(p, in_fd, out_fd, sep, -1, -1, report_fd, stats);
}

extern "C" int kx_run_records_fd_quoted(kx_program* p, int in_fd, int out_fd, uint8_t sep, uint8_t quote, int report_fd,
                                        kx_records_stats* stats) {
  if (quote == sep) return setErr(KX_E_ARG, "kx_run_records_fd_quoted: the quote byte cannot be the separator");
  return runRecordsFd(p, in_fd, out_fd, sep, quote, -1, report_fd, stats);
}

extern "C" int kx_run_records_fd_escaped(kx_program* p, int in_fd, int out_fd, uint8_t sep, int quote, uint8_t escape, int report_fd,
                                         kx_records_stats* stats) {
  if (quote < -1 || quote > 255) return setErr(KX_E_ARG, "kx_run_records_fd_escaped: quote must be a byte value or -1");
  if (quote == sep) return setErr(KX_E_ARG, "kx_run_records_fd_escaped: the quote byte cannot be the separator");
  if (escape == sep) return setErr(KX_E_ARG, "kx_run_records_fd_escaped: the escape byte cannot be the separator");
  if (quote == escape) return setErr(KX_E_ARG, "kx_run_records_fd_escaped: the escape byte cannot be the quote byte");
  return runRecordsFd(p, in_fd, out_fd, sep, quote, escape, report_fd, stats);
}

extern "C" int kx_run_records_fd_rs(kx_program* p, int in_fd, int out_fd, const uint8_t* rs, uint32_t rs_len, int report_fd,
                                    kx_records_stats* stats) {
  if (!rs || rs_len < 1 || rs_len > 8) return setErr(KX_E_ARG, "kx_run_records_fd_rs: the separator must be 1 to 8 bytes");
  return runRecordsFd(p, in_fd, out_fd, 0, -1, -1, report_fd, stats, rs, rs_len);
}

extern "C" int kx_run_records_fd_opts(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, int report_fd, kx_records_stats* stats) {
  if (!o) return setErr(KX_E_ARG, "null argument");
  if (o->size != sizeof(kx_records_opts)) return setErr(KX_E_ARG, "kx_run_records_fd_opts: kx_records_opts::size is not this library's");
  if (o->pad[0] || o->pad[1] || o->pad[2]) return setErr(KX_E_ARG, "kx_run_records_fd_opts: reserved words must be 0");
  for (uint32_t r : o->reserved) if (r) return setErr(KX_E_ARG, "kx_run_records_fd_opts: reserved words must be 0");
  if (o->ors_len > 8) return setErr(KX_E_ARG, "kx_run_records_fd_opts: the output separator is at most 8 bytes");
  if (o->chomp > 1) return setErr(KX_E_ARG, "kx_run_records_fd_opts: chomp must be 0 or 1");
  const bool chomp = o->chomp != 0;
  const int sep = o->sep, quote = o->quote, escape = o->escape;
  switch (o->mode) {
    case KX_RECORDS_BYTE:
      return runRecordsFd(p, in_fd, out_fd, o->sep, -1, -1, report_fd, stats, nullptr, 0, chomp, o->ors, o->ors_len);
    case KX_RECORDS_QUOTED:
      if (quote < 0 || quote > 255) return setErr(KX_E_ARG, "kx_run_records_fd_opts: quote must be a byte value");
      if (quote == sep) return setErr(KX_E_ARG, "kx_run_records_fd_opts: the quote byte cannot be the separator");
      return runRecordsFd(p, in_fd, out_fd, o->sep, quote, -1, report_fd, stats, nullptr, 0, chomp, o->ors, o->ors_len);
    case KX_RECORDS_ESCAPED:
      if (quote < -1 || quote > 255) return setErr(KX_E_ARG, "kx_run_records_fd_opts: quote must be a byte value or -1");
      if (escape < 0 || escape > 255) return setErr(KX_E_ARG, "kx_run_records_fd_opts: escape must be a byte value");
      if (quote == sep) return setErr(KX_E_ARG, "kx_run_records_fd_opts: the quote byte cannot be the separator");
      if (escape == sep) return setErr(KX_E_ARG, "kx_run_records_fd_opts: the escape byte cannot be the separator");
      if (quote == escape) return setErr(KX_E_ARG, "kx_run_records_fd_opts: the escape byte cannot be the quote byte");
      return runRecordsFd(p, in_fd, out_fd, o->sep, quote, escape, report_fd, stats, nullptr, 0, chomp, o->ors, o->ors_len);
    case KX_RECORDS_RS:
      if (o->rs_len < 1 || o->rs_len > 8) return setErr(KX_E_ARG, "kx_run_records_fd_opts: the separator must be 1 to 8 bytes");
      return runRecordsFd(p, in_fd, out_fd, 0, -1, -1, report_fd, stats, o->rs, o->rs_len, chomp, o->ors, o->ors_len);
    default:
      return setErr(KX_E_ARG, "kx_run_records_fd_opts: no such split mode");
  }
}
