// kx_records_host.inc — host side of record mode (include/kxhip.h: kx_split_records*, kx_run_records_fd*; kernels in
// kx_records.inc, kx_records_quoted.inc, kx_records_escaped.inc, kx_records_rs.inc).  Included at the end of kx_engine.hip, behind
// kx_batch_host.inc.
//
// A split is described once: a SplitSpec (the mode and its bytes) and a SplitCarry (what a buffer hands the one behind it: the
// quote parity and escape state, or the context of a multi-byte separator).  checkSplit is the one place that knows which are
// allowed; every entry point calls it.  splitRecords is the one driver: the empty buffer, the alignment, the workspace, the total's
// read-back, the capacity refusal and the final sync are its own; per mode it has the kernels that count, the tail decision with
// the outgoing carry, and the kernel that writes.  One flat RecWs holds every mode's buffers; a mode grows the ones it uses.
//
// kx_run_records_fd* reuse FdStream's reader and writer threads and its buffer pool (kx_run_fd); only the compute step differs.
// Windows are independent: per window, the split → kx_run_batch over the complete records → one output window → one report line
// per rejected record.  The record that straddles a window's end is carried (device memory, grown as needed) and run as a
// one-document batch in front of the next window's records.  The SplitCarry a window's split ends in is the next window's: quotes,
// an escape or a multi-byte separator may straddle windows, and with the last the carried record is completed by a first record
// that may be a single byte long.
//
// Framing (kx_run_records_fd_opts): with `chomp` every batch is a framed one (kx_run_batch_framed) whose trim is the separator's
// length — the batch kernels run each record without its separator, no byte is moved — and with `ors` its suffix is the output
// separator.  Only the stream's tail keeps its whole range: the last window's batch has last_whole = 1 when the split reported a
// tail, and the carried record is left whole when it is that tail (the last window brought no separator).  The splitters know
// nothing of this.
//
// Field mode (kx_run_records_fd_fields): RecordsRun::batch calls kx_run_batch_fields (kx_fields_host.inc) instead — the carried
// record and the window's records alike — with the split's quote and escape byte, the separator's length and, unless `chomp`, the
// separator kept behind the record's output.  A record without the field is reported in a line of its own kind.  With a list of
// fields (kx_run_records_fd_field_list) it calls kx_run_batch_field_list the same way; the report lines name the field.  On unquoted
// values (kx_run_records_fd_field_values) it calls kx_run_batch_field_values with the list and a codec whose one special byte is the
// record separator.  On words (kx_run_records_fd_field_words) it calls kx_run_batch_field_words with the list, fs = 0 and, with
// `unquote`, that codec; checkRecordsOpts has the blank rules.  By key (kx_run_records_fd_field_keys) RecordsRun holds a
// kx_field_keys with its own copy of the names, calls kx_run_batch_field_keys's driver and names the field of a report line by
// its key.  Projected (kx_run_records_fd_field_project) RecordsRun holds the
// kx_field_project beside the ranges, which are the normal form of its items' union, and calls kx_run_batch_field_project for the
// carried record and the window's records alike, with the codec and the words flag as above.
//
// Header records (kx_run_records_fd_table): RecordsRun::batch splits a call whose records reach below `header` into a header part
// and a data part; the tail flag goes to the part that holds the last record, and the carried record takes the same path, so a
// header record may straddle windows.  A header record that is only copied is placed with device-to-device copies; projected, it
// runs through kx_run_batch_field_header.  Record `header`'s bytes come to the host once, where kx_field_names.h cuts its cells and
// resolves the names of the items; the run's ranges and projection are filled in from that, and the records behind it launch what
// the numeric call launches.  No kernel is the header's own.

#include "kx_field_names.h"

namespace {

// which split, with which bytes: a split reads the front part of kx_records_opts, and of that only its mode's fields (sep: BYTE,
// QUOTED, ESCAPED; quote: QUOTED, and ESCAPED, where -1 is none; escape: ESCAPED; rs, rs_len: RS)
typedef kx_records_opts SplitSpec;

struct SplitCarry {   // what a buffer hands the one behind it
  uint32_t state = 0;    // QUOTED, ESCAPED: bit 0 the quote parity, bit 1 the next byte is escaped
  uint8_t ctx[8] = {};   // RS: the last bytes of the unfinished record, fewer than rs has
  uint32_t ctx_len = 0;
};

// the rules of every record entry point (`who`): KX_E_ARG unless splitRecords can run this spec from this carry
int checkSplit(const SplitSpec& s, const SplitCarry& in, const char* who) {
  auto no = [&](const char* what) { return setErr(KX_E_ARG, std::string(who) + ": " + what); };
  switch (s.mode) {
    case KX_RECORDS_BYTE:
      return 0;
    case KX_RECORDS_QUOTED:
      if (s.quote < 0 || s.quote > 255) return no("quote must be a byte value");
      if (s.quote == s.sep) return no("the quote byte cannot be the separator");
      if (in.state > 1) return no("parity_in must be 0 or 1");
      return 0;
    case KX_RECORDS_ESCAPED:
      if (s.quote < -1 || s.quote > 255) return no("quote must be a byte value or -1");
      if (s.escape < 0 || s.escape > 255) return no("escape must be a byte value");
      if (s.quote == s.sep) return no("the quote byte cannot be the separator");
      if (s.escape == s.sep) return no("the escape byte cannot be the separator");
      if (s.quote == s.escape) return no("the escape byte cannot be the quote byte");
      if (in.state > 3 || (s.quote < 0 && (in.state & 1u))) return no("state_in must be 0-3, bit 0 only with a quote");
      return 0;
    case KX_RECORDS_RS:
      if (s.rs_len < 1 || s.rs_len > 8) return no("the separator must be 1 to 8 bytes");
      if (in.ctx_len >= s.rs_len) return no("the context must be shorter than the separator");
      return 0;
    default:
      return no("no such split mode");
  }
}

struct RecWs {   // grow-only device workspace of a split; a mode grows only the buffers it uses
  BatchWs::Buf tcount, toff, flags;     // every mode: the selected separators per tile, their scan, the scans' Flags (two with quotes)
  BatchWs::Buf tq, tqoff, tsep, teven;  // QUOTED, ESCAPED: per tile the quotes, their scan, the separators, those outside quotes from an even start
  BatchWs::Buf tflag;                   // ESCAPED: the per-tile flag words
  BatchWs::Buf tmap, tcnt;              // RS with overlapping copies: the per-tile maps / states, the counts per state
  BatchWs::Buf info;                    // ESCAPED, overlapping RS: the info word (how the buffer ends)
  ~RecWs() {
    for (BatchWs::Buf* b : {&tcount, &toff, &flags, &tq, &tqoff, &tsep, &teven, &tflag, &tmap, &tcnt, &info}) if (b->p) (void)hipFree(b->p);
  }
};

// no proper prefix of rs is also a suffix: copies of rs cannot overlap
bool rsBorderFree(const uint8_t* rs, uint32_t m) {
  for (uint32_t b = 1; b < m; ++b) if (!memcmp(rs, rs + m - b, b)) return false;
  return true;
}

// the split of d_in[0, n) (checkSplit has passed): *nsep = selected separators, *nrec = records (nsep, or nsep + 1 with a
// non-empty tail), d_off[0 .. *nrec] their offsets from base.  *out = the carry for the buffer behind this one: its state is set
// on 0 and on KX_E_CAPACITY, its context and *tail_len (RS: the bytes of this buffer behind its last selected separator,
// host.split_rs_records_model) only on 0.  KX_E_CAPACITY (cap < *nrec + 1) writes nothing to d_off.
int splitRecords(const SplitSpec& s, const SplitCarry in, const uint8_t* d_in, size_t n, uint64_t base, uint64_t* d_off, uint64_t cap,
                 uint64_t* nrec, uint64_t* nsep, SplitCarry* out, uint64_t* tail_len, RecWs& W, hipStream_t sm) {
  static const char* const name[4] = {"kx_split_records", "kx_split_records_quoted", "kx_split_records_escaped", "kx_split_records_rs"};
  auto err = [&](int code, const char* what) { return setErr(code, std::string(name[s.mode]) + ": " + what); };
  *nrec = 0; *nsep = 0; *out = in; *tail_len = 0;
  if (n == 0) {
    if (cap < 1) return err(KX_E_CAPACITY, "offsets buffer too small");
    HIPCHECK(hipMemcpyAsync(d_off, &base, 8, hipMemcpyHostToDevice, sm));
    HIPCHECK(hipStreamSynchronize(sm));
    return 0;
  }
  const uint8_t* a0 = (const uint8_t*)((uintptr_t)d_in & ~(uintptr_t)15);
  const unsigned long long lo = (unsigned long long)(d_in - a0), hi = lo + n, ng = (hi + 15) / 16;
  const unsigned long long ntiles = (ng + REC_TILE - 1) / REC_TILE;
  if (ntiles > 0x7FFFFFFFull) return err(KX_E_ARG, "buffer too large");
  const bool quoted = s.mode == KX_RECORDS_QUOTED, escaped = s.mode == KX_RECORDS_ESCAPED, multi = s.mode == KX_RECORDS_RS;
  const bool overlap = multi && !rsBorderFree(s.rs, s.rs_len);
  // the workspace
  int rc = 0;
  for (BatchWs::Buf* b : {&W.tcount, &W.toff}) if (!rc) rc = BatchWs::ensure(*b, ntiles * 8);
  for (BatchWs::Buf* b : {&W.tq, &W.tqoff, &W.tsep, &W.teven}) if (!rc && (quoted || escaped)) rc = BatchWs::ensure(*b, ntiles * 8);
  if (!rc) rc = BatchWs::ensure(W.flags, (quoted || escaped ? 2 : 1) * sizeof(Flags));
  if (!rc && escaped) rc = BatchWs::ensure(W.tflag, ntiles * 4);
  if (!rc && overlap) rc = BatchWs::ensure(W.tmap, ntiles * 4);
  if (!rc && overlap) rc = BatchWs::ensure(W.tcnt, ntiles * 32);
  if (!rc && (escaped || overlap)) rc = BatchWs::ensure(W.info, 4);
  if (rc) return rc;
  auto U = [](BatchWs::Buf& b) { return (unsigned long long*)b.p; };
  auto C = [](BatchWs::Buf& b) { return (const unsigned long long*)b.p; };
  Flags* fl = (Flags*)W.flags.p;
  uint32_t* tflag = (uint32_t*)W.tflag.p;
  const dim3 tiles((uint32_t)ntiles), pertile((uint32_t)((ntiles + 255) / 256));
  // the mode's bytes as the kernels take them (ESCAPED without a quote: no byte is one)
  const uint32_t spat = 0x01010101u * s.sep, qpat = 0x01010101u * (uint8_t)(s.quote < 0 ? 0 : s.quote), epat = 0x01010101u * (uint8_t)s.escape;
  const uint32_t qkeep = s.quote < 0 ? 0u : 0xFFFF0000u, x = in.state >> 1, parity_in = in.state & 1u;
  const uint32_t m = multi ? s.rs_len : 0, k = multi ? in.ctx_len : 0;
  unsigned long long rs8 = 0, ctx8 = 0;
  for (uint32_t i = 0; i < m; ++i) rs8 |= (unsigned long long)s.rs[i] << (8 * i);
  for (uint32_t i = 0; i < k; ++i) ctx8 |= (unsigned long long)in.ctx[i] << (8 * i);
  // the count step: per tile the selected separators in tcount, then their scan in toff and their total in `flt`
  switch (s.mode) {
    case KX_RECORDS_BYTE:
      hipLaunchKernelGGL(k_rcount, tiles, dim3(REC_BT), 0, sm, a0, ng, lo, hi, spat, U(W.tcount));
      break;
    case KX_RECORDS_QUOTED:
      hipLaunchKernelGGL(k_rqcount, tiles, dim3(REC_BT), 0, sm, a0, ng, lo, hi, spat, qpat, U(W.tq), U(W.tsep), U(W.teven));
      hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(1024), 0, sm, (uint32_t)ntiles, C(W.tq), U(W.tqoff), fl);
      hipLaunchKernelGGL(k_rqselect, pertile, dim3(256), 0, sm, (uint32_t)ntiles, C(W.tqoff), C(W.tsep), C(W.teven), parity_in, U(W.tcount));
      break;
    case KX_RECORDS_ESCAPED:
      hipLaunchKernelGGL(k_recount, tiles, dim3(REC_BT), 0, sm, a0, ng, lo, hi, spat, qpat, qkeep, epat, x, U(W.tq), U(W.tsep), U(W.teven), tflag);
      hipLaunchKernelGGL(k_rescan, dim3(1), dim3(1024), 0, sm, (uint32_t)ntiles, lo == 0 ? x : 0u, tflag, U(W.tq));
      hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(1024), 0, sm, (uint32_t)ntiles, C(W.tq), U(W.tqoff), fl);
      hipLaunchKernelGGL(k_reselect, pertile, dim3(256), 0, sm, (uint32_t)ntiles, (const uint32_t*)tflag, C(W.tq), C(W.tqoff), C(W.tsep),
                         C(W.teven), parity_in, U(W.tcount), (uint32_t*)W.info.p);
      break;
    default:
      if (overlap) {
        hipLaunchKernelGGL(k_rocount, tiles, dim3(REC_BT), 0, sm, a0, ng, lo, hi, rs8, m, ctx8, k, (uint32_t*)W.tmap.p, (uint32_t*)W.tcnt.p);
        hipLaunchKernelGGL(k_rsscan, dim3(1), dim3(1024), 0, sm, (uint32_t)ntiles, m, (uint32_t*)W.tmap.p, (const uint32_t*)W.tcnt.p, U(W.tcount),
                           (uint32_t*)W.info.p);
      } else {
        hipLaunchKernelGGL(k_rbcount, tiles, dim3(REC_BT), 0, sm, a0, ng, lo, hi, rs8, m, ctx8, k, U(W.tcount));
      }
  }
  Flags* flt = quoted || escaped ? fl + 1 : fl;   // (with quotes the first Flags is the quote scan's)
  hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(1024), 0, sm, (uint32_t)ntiles, C(W.tcount), U(W.toff), flt);
  HIPCHECK(hipGetLastError());
  // the total, and what the mode's tail decision reads
  unsigned long long total = 0, quotes = 0;
  uint32_t info = 0;
  uint8_t lastb = 0, endb[16] = {};   // RS: the context, then the buffer's last nl bytes: every byte that out->ctx or the last candidate can hold
  const size_t nl = n < 8 ? n : 8;
  const uint8_t* end = endb + k + nl;   // (behind the buffer's last byte)
  HIPCHECK(hipMemcpyAsync(&total, &flt->total_len, 8, hipMemcpyDeviceToHost, sm));
  if (quoted) HIPCHECK(hipMemcpyAsync(&quotes, &fl->total_len, 8, hipMemcpyDeviceToHost, sm));
  if (!escaped && !multi) HIPCHECK(hipMemcpyAsync(&lastb, d_in + n - 1, 1, hipMemcpyDeviceToHost, sm));
  if (multi) {
    memcpy(endb, in.ctx, k);
    HIPCHECK(hipMemcpyAsync(endb + k, d_in + n - nl, nl, hipMemcpyDeviceToHost, sm));
  }
  if (escaped || overlap) HIPCHECK(hipMemcpyAsync(&info, W.info.p, 4, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  // the tail (the buffer's end is no record's end) and the state handed on
  int tail = 0;
  switch (s.mode) {
    case KX_RECORDS_BYTE:
      tail = lastb != s.sep;
      break;
    case KX_RECORDS_QUOTED:
      out->state = parity_in ^ (uint32_t)(quotes & 1u);
      tail = !(lastb == s.sep && out->state == 0);   // (a last separator byte inside quotes ends no record)
      break;
    case KX_RECORDS_ESCAPED:
      out->state = (info >> 1) & 3u;
      tail = !(info & 1u);   // (an escaped separator, or one inside quotes, as the last byte ends no record)
      break;
    default: {
      const size_t known = n < 8 ? k + n : 8;   // bytes before `end` that belong to the unfinished record or the buffer
      // border-free: every copy is selected, so the buffer ends in a separator iff its last m bytes (the context's included) are rs
      tail = overlap ? !(info & 1u) : !(known >= m && !memcmp(end - m, s.rs, m));
    }
  }
  *nsep = total;
  *nrec = total + (uint64_t)tail;
  if (cap < *nrec + 1 || !d_off) return err(KX_E_CAPACITY, "offsets buffer too small");
  // the write step
  const unsigned long long ubase = base;
  unsigned long long* uoff = (unsigned long long*)d_off;
  switch (s.mode) {
    case KX_RECORDS_BYTE:
      hipLaunchKernelGGL(k_rwrite, tiles, dim3(REC_BT), 0, sm, a0, ng, lo, hi, spat, C(W.toff), ubase, total, tail, uoff);
      break;
    case KX_RECORDS_QUOTED:
      hipLaunchKernelGGL(k_rqwrite, tiles, dim3(REC_BT), 0, sm, a0, ng, lo, hi, spat, qpat, C(W.tqoff), parity_in, C(W.toff), ubase, total, tail, uoff);
      break;
    case KX_RECORDS_ESCAPED:
      hipLaunchKernelGGL(k_rewrite, tiles, dim3(REC_BT), 0, sm, a0, ng, lo, hi, spat, qpat, qkeep, epat, x, (const uint32_t*)tflag, C(W.tqoff),
                         parity_in, C(W.toff), ubase, total, tail, uoff);
      break;
    default:
      if (overlap)
        hipLaunchKernelGGL(k_rowrite, tiles, dim3(REC_BT), 0, sm, a0, ng, lo, hi, rs8, m, ctx8, k, (const uint32_t*)W.tmap.p, C(W.toff), ubase, total,
                           tail, uoff);
      else
        hipLaunchKernelGGL(k_rbwrite, tiles, dim3(REC_BT), 0, sm, a0, ng, lo, hi, rs8, m, ctx8, k, C(W.toff), ubase, total, tail, uoff);
  }
  HIPCHECK(hipGetLastError());
  uint64_t e = base;   // RS: the last selected separator's end
  if (multi && tail && total) HIPCHECK(hipMemcpyAsync(&e, d_off + total, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  if (multi) {   // the context handed on, and the tail's length
    const uint64_t tl = tail ? n - (e - base) : 0;
    size_t unfinished = total ? tl : k + n;                       // the unfinished record so far (without a separator: the context's bytes too)
    if (!tail) unfinished = 0;
    const size_t co = unfinished < m - 1 ? unfinished : m - 1;    // (≤ 7 ≤ known whenever unfinished ≥ 7)
    memcpy(out->ctx, end - co, co);
    out->ctx_len = (uint32_t)co;
    *tail_len = tl;
  }
  return 0;
}

// the compute step of the kx_run_records_fd* entry points
struct RecordsRun {
  kx_program* p = nullptr;
  FdStream* fs = nullptr;
  kx_records_opts o{};                                 // the split, and the framing: chomp, ors (checkRecordsOpts has passed)
  uint32_t field = 0;                                  // field mode: the program runs on field `field` (0: on the record)
  uint8_t fsep = 0;                                    //   ... of the fields that `fsep` separates
  kx_field_range ranges[8] = {};                       // field mode with a list: the program runs on the fields of ranges[0, n_ranges)
  uint32_t n_ranges = 0;                               //   (0: no list; `field` is 0 with a list)
  kx_field_codec codec{};                              // ... on their values (size != 0: kx_run_batch_field_values; special = the separator)
  bool words = false;                                  // ... which are the body's words (kx_run_batch_field_words; fsep is not used)
  kx_field_project proj{};                             // ... projected (size != 0: kx_run_batch_field_project; ranges = the items' union)
  kx_field_keys keys{};                                // field mode by key (size != 0: kx_run_batch_field_keys; n_ranges is 0, proj's items are names)
  std::vector<std::string> key_names;                  //   ... whose names these are (keys.names point into them)
  uint64_t header = 0;                                 // the first `header` records are header records (kx_run_records_fd_table)
  kx_field_range titems[KX_FIELD_ITEMS] = {};          // ... and these items, some of them names (lo = 0, hi = the index into `names`),
  uint32_t n_titems = 0;                               //   become ranges (and proj.items) when record `header` is in hand
  std::vector<std::string> names;
  bool resolved = true;                                // (false: titems wait for that record)
  const char* who = "";                                // the entry point, for a resolution that fails
  BatchWs::Buf hstash, hoff;                           // projected by names: the header records held until the names are resolved
  std::vector<uint64_t> hends;                         //   ... and where each ends in hstash
  SplitCarry next;                                     // what the next window's split starts from
  int report_fd = -1;
  RecWs ws;
  BatchWs::Buf off, ooff, docs, carry, one, longest;   // offsets; output offsets; doc records; the straddling record; its offsets
  BatchWs::Buf ffield;                                 // with a list: the field number of every record's report line
  uint64_t carry_len = 0, recno = 0;                   // records reported so far (R of the next record is recno + 1)
  double ratio = 4.0;                                  // output bytes per input byte, from the previous window
  bool rejected = false;
  kx_records_stats st{};
  hipEvent_t ev[4] = {};
  bool timing = false;

  ~RecordsRun() {
    for (BatchWs::Buf* b : {&off, &ooff, &docs, &carry, &one, &longest, &ffield, &hstash, &hoff}) if (b->p) (void)hipFree(b->p);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
  }

  // ff: with a list, the field number of every record's line; by key, 1 + the index of the name the line names
  int report(const kx_batch_doc* d, uint64_t n, uint64_t first_rec, const uint32_t* ff = nullptr) {
    if (report_fd < 0) return 0;
    std::string s;
    auto name = [&](uint64_t i) { return ff[i] >= 1 && ff[i] <= key_names.size() ? kxPrintableName(key_names[ff[i] - 1]) : std::string("?"); };
    for (uint64_t i = 0; i < n; ++i)
      if (d[i].status == 2 && keys.size) s += "Record " + std::to_string(first_rec + i) + " has no field " + name(i) + "!\n";
      else if (d[i].status && keys.size)
        s += "Match error at input symbol " + std::to_string(d[i].fail_pos) + " in field " + name(i) + " of record " + std::to_string(first_rec + i) + "!\n";
      else if (d[i].status == 2) s += "Record " + std::to_string(first_rec + i) + " has no field " + std::to_string(ff ? ff[i] : field) + "!\n";
      else if (d[i].status && ff)
        s += "Match error at input symbol " + std::to_string(d[i].fail_pos) + " in field " + std::to_string(ff[i]) + " of record " +
             std::to_string(first_rec + i) + "!\n";
      else if (d[i].status) s += "Match error at input symbol " + std::to_string(d[i].fail_pos) + " in record " + std::to_string(first_rec + i) + "!\n";
    for (size_t w = 0; w < s.size();) {
      const ssize_t r = write(report_fd, s.data() + w, s.size() - w);
      if (r < 0) { if (errno == EINTR) continue; return setErr(KX_E_IO, "write of the record report failed"); }
      w += (size_t)r;
    }
    return 0;
  }

  // room for `need` more bytes in *out at byte pos: a buffer too small is replaced by a larger one, its first pos bytes kept
  int reserve(DevBuf* out, size_t pos, size_t need) {
    if (out->cap - pos >= need) return 0;
    DevBuf nb;
    const int rc = fs->pool.get(pos + need + need / 8 + 4096, &nb);
    if (rc) return rc;
    if (pos) HIPCHECK(hipMemcpy(nb.d, out->d, pos, hipMemcpyDeviceToDevice));
    fs->pool.put(*out);
    *out = nb;
    return 0;
  }

  // the names of titems against header record `header`, whose bytes are in[b, e) (its separator included unless it is the tail):
  // ranges, and with a projection its items, are filled in from the resolver (kx_field_names.h)
  int resolve(const uint8_t* in, uint64_t b, uint64_t e, bool tail) {
    const uint64_t sep_len = tail ? 0 : o.mode == KX_RECORDS_RS ? o.rs_len : 1u;
    std::vector<uint8_t> body(e - b - sep_len);
    if (!body.empty()) HIPCHECK(hipMemcpy(body.data(), in + b, body.size(), hipMemcpyDeviceToHost));
    const bool q = o.mode == KX_RECORDS_QUOTED || o.mode == KX_RECORDS_ESCAPED;
    std::vector<std::string> cells;
    kxHeaderCellNames(body.data(), body.size(), fsep, q ? o.quote : -1, o.mode == KX_RECORDS_ESCAPED ? o.escape : -1, words, header == 1, &cells);
    kx_field_range items[KX_FIELD_ITEMS] = {};
    uint32_t missing = 0;
    const int bad = kxResolveFieldNames(titems, n_titems, names, cells, items, ranges, &n_ranges, &missing);
    if (bad == 1)
      return setErr(KX_E_HEADER, std::string(who) + ": no cell of header record " + std::to_string(header) + " is named \"" +
                                     kxPrintableName(names[missing]) + "\"");
    if (bad) return setErr(KX_E_HEADER, std::string(who) + ": the fields that the names of header record " + std::to_string(header) +
                                            " select have more than 8 ranges in their normal form");
    if (proj.size) memcpy(proj.items, items, sizeof proj.items);
    resolved = true;
    return 0;
  }

  // the h header records in[d_o[0], d_o[h]) (numbered from first_rec; tail: the last one is the stream's tail).  Not projected,
  // each is placed with device-to-device copies: its body, its separator unless `chomp`, the `ors` bytes.  Projected, they run
  // through kx_run_batch_field_header — once the names are resolved, until when they are held in hstash.  Record `header` resolves.
  int headerPart(const uint8_t* in, const uint64_t* d_o, uint64_t h, DevBuf* out, size_t* pos, uint64_t first_rec, bool tail) {
    std::vector<uint64_t> ho(h + 1);
    HIPCHECK(hipMemcpy(ho.data(), d_o, (h + 1) * 8, hipMemcpyDeviceToHost));
    const bool resolves = !resolved && first_rec + h - 1 == header;
    if (resolves) if (const int rc = resolve(in, ho[h - 1], ho[h], tail)) return rc;
    if (proj.size && n_titems && !names.empty()) {   // projected by names: held, and run together when the names are resolved
      const uint64_t held = hends.empty() ? 0 : hends.back(), n = ho[h] - ho[0];
      int rc = BatchWs::grow(hstash, held, held + n, nullptr);
      if (rc) return rc;
      if (n) HIPCHECK(hipMemcpy((uint8_t*)hstash.p + held, in + ho[0], n, hipMemcpyDeviceToDevice));
      for (uint64_t i = 1; i <= h; ++i) hends.push_back(held + ho[i] - ho[0]);
      if (!resolves) { st.records += h; return 0; }
      std::vector<uint64_t> so(1, 0);
      so.insert(so.end(), hends.begin(), hends.end());
      rc = BatchWs::ensure(hoff, so.size() * 8);
      if (rc) return rc;
      HIPCHECK(hipMemcpy(hoff.p, so.data(), so.size() * 8, hipMemcpyHostToDevice));
      st.records -= so.size() - 1 - h;   // (runPart counts the held ones once more)
      hends.clear();
      return runPart((const uint8_t*)hstash.p, (const uint64_t*)hoff.p, so.size() - 1, out, pos, 1, tail, true);
    }
    if (proj.size) return runPart(in, d_o, h, out, pos, first_rec, tail, true);
    const uint64_t sep_len = o.mode == KX_RECORDS_RS ? o.rs_len : 1u, seps = h - (tail ? 1 : 0);
    const size_t need = (size_t)(ho[h] - ho[0] - (o.chomp ? seps * sep_len : 0) + h * o.ors_len);
    if (const int rc = reserve(out, *pos, need)) return rc;
    uint8_t* w = (uint8_t*)out->d + *pos;
    if (!o.chomp && !o.ors_len) {
      if (need) HIPCHECK(hipMemcpy(w, in + ho[0], need, hipMemcpyDeviceToDevice));
    } else {
      for (uint64_t i = 0; i < h; ++i) {
        const uint64_t n = ho[i + 1] - ho[i] - (o.chomp && !(tail && i == h - 1) ? sep_len : 0);
        if (n) HIPCHECK(hipMemcpy(w, in + ho[i], n, hipMemcpyDeviceToDevice));
        if (o.ors_len) HIPCHECK(hipMemcpy(w + n, o.ors, o.ors_len, hipMemcpyHostToDevice));
        w += n + o.ors_len;
      }
    }
    st.records += h;
    st.out_bytes += need;
    *pos += need;
    return 0;
  }

  // the records in[d_o[0], d_o[ndocs]) into *out at byte pos: the header records among them (headerPart), then the rest (runPart)
  int batch(const uint8_t* in, const uint64_t* d_o, uint64_t ndocs, DevBuf* out, size_t* pos, uint64_t first_rec, bool tail) {
    if (ndocs == 0) return 0;
    if (first_rec <= header) {
      const uint64_t h = std::min<uint64_t>(ndocs, header - first_rec + 1);
      if (const int rc = headerPart(in, d_o, h, out, pos, first_rec, tail && h == ndocs)) return rc;
      d_o += h; ndocs -= h; first_rec += h;
    }
    return runPart(in, d_o, ndocs, out, pos, first_rec, tail, false);
  }

  // kx_run_batch of ndocs records (offsets d_o) into *out at byte pos; a buffer too small is replaced by one of the size needed,
  // its first pos bytes kept.  Reports the rejected records (numbered from first_rec) and advances *pos.  tail: the last of
  // these records is the stream's tail (it has no separator to strip).  identity: they are header records under a projection
  // (kx_run_batch_field_header).
  int runPart(const uint8_t* in, const uint64_t* d_o, uint64_t ndocs, DevBuf* out, size_t* pos, uint64_t first_rec, bool tail, bool identity) {
    if (ndocs == 0) return 0;
    kx_batch_frame fr{};
    fr.trim = o.chomp ? (o.mode == KX_RECORDS_RS ? o.rs_len : 1u) : 0u;
    fr.last_whole = tail ? 1u : 0u;
    fr.suffix_len = o.ors_len;
    memcpy(fr.suffix, o.ors, o.ors_len);
    const kx_batch_frame* frp = fr.trim || fr.suffix_len ? &fr : nullptr;
    kx_batch_fields fl{};
    fl.size = sizeof fl; fl.field = field; fl.fs = fsep;
    fl.quote = o.mode == KX_RECORDS_QUOTED || o.mode == KX_RECORDS_ESCAPED ? o.quote : -1;
    fl.escape = o.mode == KX_RECORDS_ESCAPED ? o.escape : -1;
    fl.sep_len = o.mode == KX_RECORDS_RS ? o.rs_len : 1u;
    fl.last_whole = tail ? 1u : 0u;
    fl.keep_sep = o.chomp ? 0u : 1u;
    fl.suffix_len = o.ors_len;
    memcpy(fl.suffix, o.ors, o.ors_len);
    kx_batch_field_list ll{};
    ll.size = sizeof ll; ll.n_ranges = n_ranges; ll.fs = words ? (uint8_t)0 : fsep;
    memcpy(ll.ranges, ranges, sizeof ll.ranges);
    ll.quote = fl.quote; ll.escape = fl.escape; ll.sep_len = fl.sep_len; ll.last_whole = fl.last_whole; ll.keep_sep = fl.keep_sep;
    ll.suffix_len = fl.suffix_len;
    memcpy(ll.suffix, fl.suffix, sizeof ll.suffix);
    const bool listed = n_ranges || keys.size;       // the call fills ffield
    auto run = [&](void* d_out, size_t cap, size_t* ol, kx_batch_stats* bs) {
      if (keys.size)
        return fieldKeysEntry("kx_run_records_fd_field_keys", o.mode != KX_RECORDS_RS ? (int)o.sep : o.rs_len == 1 ? (int)o.rs[0] : -1, p, in, d_o, ndocs,
                              &ll, &keys, codec.size ? &codec : nullptr, proj.size ? &proj : nullptr, d_out, cap, (uint64_t*)ooff.p,
                              (kx_batch_doc*)docs.p, (uint32_t*)ffield.p, ol, bs, nullptr);
      if (identity)
        return kx_run_batch_field_header(p, in, d_o, ndocs, &ll, codec.size ? &codec : nullptr, &proj, d_out, cap, (uint64_t*)ooff.p,
                                         (kx_batch_doc*)docs.p, (uint32_t*)ffield.p, ol, bs, nullptr);
      if (n_ranges && proj.size)
        return kx_run_batch_field_project(p, in, d_o, ndocs, &ll, codec.size ? &codec : nullptr, &proj, d_out, cap, (uint64_t*)ooff.p,
                                          (kx_batch_doc*)docs.p, (uint32_t*)ffield.p, ol, bs, nullptr);
      if (n_ranges && words)
        return kx_run_batch_field_words(p, in, d_o, ndocs, &ll, codec.size ? &codec : nullptr, d_out, cap, (uint64_t*)ooff.p, (kx_batch_doc*)docs.p,
                                        (uint32_t*)ffield.p, ol, bs, nullptr);
      if (n_ranges && codec.size)
        return kx_run_batch_field_values(p, in, d_o, ndocs, &ll, &codec, d_out, cap, (uint64_t*)ooff.p, (kx_batch_doc*)docs.p, (uint32_t*)ffield.p, ol,
                                         bs, nullptr);
      if (n_ranges)
        return kx_run_batch_field_list(p, in, d_o, ndocs, &ll, d_out, cap, (uint64_t*)ooff.p, (kx_batch_doc*)docs.p, (uint32_t*)ffield.p, ol, bs,
                                       nullptr);
      return field ? kx_run_batch_fields(p, in, d_o, ndocs, &fl, d_out, cap, (uint64_t*)ooff.p, (kx_batch_doc*)docs.p, ol, bs, nullptr)
                   : kx_run_batch_framed(p, in, d_o, ndocs, frp, d_out, cap, (uint64_t*)ooff.p, (kx_batch_doc*)docs.p, ol, bs, nullptr);
    };
    int rc = BatchWs::ensure(ooff, (ndocs + 1) * 8);
    if (!rc) rc = BatchWs::ensure(docs, ndocs * sizeof(kx_batch_doc));
    if (!rc && listed) rc = BatchWs::ensure(ffield, ndocs * 4);
    if (rc) return rc;
    kx_batch_stats bs{};
    size_t ol = 0;
    if (timing) HIPCHECK(hipEventRecord(ev[2], nullptr));
    rc = run(out->d + *pos, out->cap - *pos, &ol, &bs);
    if (rc == KX_E_CAPACITY) {
      DevBuf nb;
      rc = fs->pool.get(*pos + ol + ol / 8 + 4096, &nb);
      if (rc) return rc;
      if (*pos) HIPCHECK(hipMemcpy(nb.d, out->d, *pos, hipMemcpyDeviceToDevice));
      fs->pool.put(*out);
      *out = nb;
      rc = run(out->d + *pos, out->cap - *pos, &ol, &bs);
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
      std::vector<uint32_t> hf(listed ? ndocs : 0);
      if (listed) HIPCHECK(hipMemcpy(hf.data(), ffield.p, ndocs * 4, hipMemcpyDeviceToHost));
      return report(h.data(), ndocs, first_rec, listed ? hf.data() : nullptr);
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
    SplitCarry end;
    uint64_t tail_len = 0;
    auto split = [&] { return splitRecords(o, next, in, n, 0, (uint64_t*)off.p, off.cap / 8, &nrec, &nsep, &end, &tail_len, ws, nullptr); };
    int rc = split();
    if (rc == KX_E_CAPACITY) {
      rc = BatchWs::ensure(off, (nrec + 1) * 8);
      if (!rc) rc = split();
    }
    if (rc) return rc;
    next = end;
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

// what the four kx_split_records* entry points share (n_records is not null): the rules, the pointers, a workspace of its own
// and the split from *c, which becomes the carry it ends in
int splitEntry(const char* who, const SplitSpec& s, SplitCarry* c, const void* d_in, size_t n, uint64_t base, uint64_t* d_off, uint64_t cap,
               uint64_t* n_records, uint64_t* tail_len, void* stream) {
  *n_records = 0;
  if (const int rc = checkSplit(s, *c, who)) return rc;
  if (n && !d_in) return setErr(KX_E_ARG, std::string(who) + ": null input");
  if (cap && !d_off) return setErr(KX_E_ARG, std::string(who) + ": null offsets with a capacity");
  RecWs ws;
  uint64_t nsep = 0;
  return splitRecords(s, *c, (const uint8_t*)d_in, n, base, d_off, cap, n_records, &nsep, c, tail_len, ws, (hipStream_t)stream);
}

// the options of a mode's own entry points: no framing
kx_records_opts plainOpts(uint32_t mode, uint8_t sep, int quote, int escape) {
  kx_records_opts o{};
  o.size = sizeof o; o.mode = mode; o.sep = sep; o.quote = quote; o.escape = escape;
  return o;
}

// ... with an entry point's (rs, rs_len); a null rs gives rs_len 0, which checkSplit refuses as any other bad length
kx_records_opts rsOpts(const uint8_t* rs, uint32_t rs_len) {
  kx_records_opts o = plainOpts(KX_RECORDS_RS, 0, -1, -1);
  o.rs_len = rs ? rs_len : 0;
  if (rs && rs_len <= 8) memcpy(o.rs, rs, rs_len);
  return o;
}

}  // namespace

extern "C" int kx_split_records(const void* d_in, size_t n, uint8_t sep, uint64_t base, uint64_t* d_off, uint64_t cap, uint64_t* n_records,
                                void* stream) {
  if (!n_records) return setErr(KX_E_ARG, "null argument");
  SplitCarry c;
  uint64_t tl = 0;
  return splitEntry("kx_split_records", plainOpts(KX_RECORDS_BYTE, sep, -1, -1), &c, d_in, n, base, d_off, cap, n_records, &tl, stream);
}

extern "C" int kx_split_records_quoted(const void* d_in, size_t n, uint8_t sep, uint8_t quote, uint32_t parity_in, uint64_t base,
                                       uint64_t* d_off, uint64_t cap, uint64_t* n_records, uint32_t* parity_out, void* stream) {
  if (!n_records) return setErr(KX_E_ARG, "null argument");
  if (parity_out) *parity_out = 0;
  SplitCarry c;
  c.state = parity_in;
  uint64_t tl = 0;
  const int rc = splitEntry("kx_split_records_quoted", plainOpts(KX_RECORDS_QUOTED, sep, quote, -1), &c, d_in, n, base, d_off, cap, n_records, &tl, stream);
  if (parity_out && (rc == 0 || rc == KX_E_CAPACITY)) *parity_out = c.state;
  return rc;
}

extern "C" int kx_split_records_escaped(const void* d_in, size_t n, uint8_t sep, int quote, uint8_t escape, uint32_t state_in, uint64_t base,
                                        uint64_t* d_off, uint64_t cap, uint64_t* n_records, uint32_t* state_out, void* stream) {
  if (!n_records) return setErr(KX_E_ARG, "null argument");
  if (state_out) *state_out = 0;
  SplitCarry c;
  c.state = state_in;
  uint64_t tl = 0;
  const int rc = splitEntry("kx_split_records_escaped", plainOpts(KX_RECORDS_ESCAPED, sep, quote, escape), &c, d_in, n, base, d_off, cap, n_records, &tl, stream);
  if (state_out && (rc == 0 || rc == KX_E_CAPACITY)) *state_out = c.state;
  return rc;
}

extern "C" int kx_split_records_rs(const void* d_in, size_t n, const uint8_t* rs, uint32_t rs_len, const uint8_t* ctx_in, uint32_t ctx_in_len,
                                   uint64_t base, uint64_t* d_off, uint64_t cap, uint64_t* n_records, uint8_t* ctx_out, uint32_t* ctx_out_len,
                                   uint64_t* tail_len, void* stream) {
  if (!n_records) return setErr(KX_E_ARG, "null argument");
  *n_records = 0;
  if (ctx_out_len) *ctx_out_len = 0;
  if (tail_len) *tail_len = 0;
  if (ctx_in_len && !ctx_in) return setErr(KX_E_ARG, "kx_split_records_rs: null context with a length");
  SplitCarry c;
  c.ctx_len = ctx_in_len;
  if (ctx_in_len && ctx_in_len < 8) memcpy(c.ctx, ctx_in, ctx_in_len);   // (8 and more: refused, whatever rs_len is)
  uint64_t tl = 0;
  const int rc = splitEntry("kx_split_records_rs", rsOpts(rs, rs_len), &c, d_in, n, base, d_off, cap, n_records, &tl, stream);
  if (rc == 0) {
    if (ctx_out) memcpy(ctx_out, c.ctx, c.ctx_len);
    if (ctx_out_len) *ctx_out_len = c.ctx_len;
    if (tail_len) *tail_len = tl;
  }
  return rc;
}

namespace {

// the rules of the kx_run_records_fd* entry points (`who`); fs: the field separator of field mode, or -1; blanks: the fields are
// the words between blanks (fs = -1), which the one-byte record separator, the quote and the escape byte of the mode cannot be
int checkRecordsOpts(const kx_records_opts& o, const char* who, int fs = -1, bool blanks = false) {
  auto no = [&](const char* what) { return setErr(KX_E_ARG, std::string(who) + ": " + what); };
  if (o.size != sizeof(kx_records_opts)) return no("kx_records_opts::size is not this library's");
  if (o.pad[0] || o.pad[1] || o.pad[2]) return no("reserved words must be 0");
  for (uint32_t r : o.reserved) if (r) return no("reserved words must be 0");
  if (o.ors_len > 8) return no("the output separator is at most 8 bytes");
  if (o.chomp > 1) return no("chomp must be 0 or 1");
  if (const int rc = checkSplit(o, SplitCarry{}, who)) return rc;
  if (blanks) {
    auto blank = [](int b) { return b == 0x20 || b == 0x09; };
    if (o.mode != KX_RECORDS_RS && blank(o.sep)) return no("the record separator cannot be a blank");
    if (o.mode == KX_RECORDS_RS && o.rs_len == 1 && blank(o.rs[0])) return no("the record separator cannot be a blank");
    if ((o.mode == KX_RECORDS_QUOTED || o.mode == KX_RECORDS_ESCAPED) && blank(o.quote)) return no("the quote byte cannot be a blank");
    if (o.mode == KX_RECORDS_ESCAPED && blank(o.escape)) return no("the escape byte cannot be a blank");
  }
  if (fs < 0) return 0;
  if (o.mode != KX_RECORDS_RS && fs == (int)o.sep) return no("the field separator cannot be the record separator");
  if (o.mode == KX_RECORDS_RS && o.rs_len == 1 && fs == (int)o.rs[0]) return no("the field separator cannot be the record separator");
  if ((o.mode == KX_RECORDS_QUOTED || o.mode == KX_RECORDS_ESCAPED) && fs == o.quote) return no("the field separator cannot be the quote byte");
  if (o.mode == KX_RECORDS_ESCAPED && fs == o.escape) return no("the field separator cannot be the escape byte");
  return 0;
}

// the stream on in_fd in record mode as `o` says (checkRecordsOpts has passed)
int runRecordsFd(kx_program* p, int in_fd, int out_fd, const kx_records_opts& o, int report_fd, kx_records_stats* stats, uint32_t field = 0,
                 uint8_t fsep = 0, const kx_field_range* ranges = nullptr, uint32_t n_ranges = 0, bool values = false, bool words = false,
                 const kx_field_project* proj = nullptr, const kx_records_table* t = nullptr, const char* who = "",
                 const kx_field_keys* keys = nullptr) {
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
  R.p = p; R.fs = &fsr; R.o = o; R.report_fd = report_fd; R.field = field; R.fsep = fsep;
  R.n_ranges = n_ranges; R.words = words;
  if (n_ranges) memcpy(R.ranges, ranges, n_ranges * sizeof(kx_field_range));
  if (proj) R.proj = *proj;
  if (keys) {   // (the names are copied: the batch calls read them window after window)
    R.keys = *keys;
    for (uint32_t j = 0; j < keys->n_names; ++j) R.key_names.emplace_back((const char*)keys->names[j], keys->name_len[j]);
    for (uint32_t j = 0; j < keys->n_names; ++j) R.keys.names[j] = (const uint8_t*)R.key_names[j].data();
  }
  if (t) {   // header records, and items that may be names (checkTable has passed): without a name the caller has resolved them
    R.header = t->header; R.who = who;
    for (uint32_t j = 0; j < t->n_items; ++j) if (t->items[j].lo == 0) R.resolved = false;
    if (!R.resolved) {
      R.n_titems = t->n_items;
      memcpy(R.titems, t->items, sizeof R.titems);
      for (uint32_t j = 0; j < t->n_names; ++j) R.names.emplace_back((const char*)t->names[j], t->name_len[j]);
    }
  }
  if (values) { R.codec.size = sizeof R.codec; R.codec.n_special = 1; R.codec.special[0] = o.sep; }
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

int runRecords(const char* who, kx_program* p, int in_fd, int out_fd, const kx_records_opts& o, int report_fd, kx_records_stats* stats) {
  if (const int rc = checkRecordsOpts(o, who)) return rc;
  return runRecordsFd(p, in_fd, out_fd, o, report_fd, stats);
}

}  // namespace

extern "C" int kx_run_records_fd(kx_program* p, int in_fd, int out_fd, uint8_t sep, int report_fd, kx_records_stats* stats) {
  return runRecords("kx_run_records_fd", p, in_fd, out_fd, plainOpts(KX_RECORDS_BYTE, sep, -1, -1), report_fd, stats);
}

extern "C" int kx_run_records_fd_quoted(kx_program* p, int in_fd, int out_fd, uint8_t sep, uint8_t quote, int report_fd,
                                        kx_records_stats* stats) {
  return runRecords("kx_run_records_fd_quoted", p, in_fd, out_fd, plainOpts(KX_RECORDS_QUOTED, sep, quote, -1), report_fd, stats);
}

extern "C" int kx_run_records_fd_escaped(kx_program* p, int in_fd, int out_fd, uint8_t sep, int quote, uint8_t escape, int report_fd,
                                         kx_records_stats* stats) {
  return runRecords("kx_run_records_fd_escaped", p, in_fd, out_fd, plainOpts(KX_RECORDS_ESCAPED, sep, quote, escape), report_fd, stats);
}

extern "C" int kx_run_records_fd_rs(kx_program* p, int in_fd, int out_fd, const uint8_t* rs, uint32_t rs_len, int report_fd,
                                    kx_records_stats* stats) {
  return runRecords("kx_run_records_fd_rs", p, in_fd, out_fd, rsOpts(rs, rs_len), report_fd, stats);
}

extern "C" int kx_run_records_fd_opts(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, int report_fd, kx_records_stats* stats) {
  if (!o) return setErr(KX_E_ARG, "null argument");
  return runRecords("kx_run_records_fd_opts", p, in_fd, out_fd, *o, report_fd, stats);
}

extern "C" int kx_run_records_fd_fields(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, uint32_t field, uint8_t fs, int report_fd,
                                        kx_records_stats* stats) {
  if (!o) return setErr(KX_E_ARG, "null argument");
  if (field == 0) return setErr(KX_E_ARG, "kx_run_records_fd_fields: field numbers start at 1");
  if (const int rc = checkRecordsOpts(*o, "kx_run_records_fd_fields", fs)) return rc;
  return runRecordsFd(p, in_fd, out_fd, *o, report_fd, stats, field, fs);
}

extern "C" int kx_run_records_fd_field_list(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, const kx_field_range* ranges,
                                            uint32_t n_ranges, uint8_t fs, int report_fd, kx_records_stats* stats) {
  if (!o || !ranges) return setErr(KX_E_ARG, "null argument");
  if (!kxFieldListIsNormal(ranges, n_ranges))
    return setErr(KX_E_ARG, "kx_run_records_fd_field_list: the field list is not in normal form (1 to 8 ranges: sorted, disjoint, not adjacent, only the last open)");
  if (const int rc = checkRecordsOpts(*o, "kx_run_records_fd_field_list", fs)) return rc;
  return runRecordsFd(p, in_fd, out_fd, *o, report_fd, stats, 0, fs, ranges, n_ranges);
}

extern "C" int kx_run_records_fd_field_values(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, const kx_field_range* ranges,
                                              uint32_t n_ranges, uint8_t fs, int report_fd, kx_records_stats* stats) {
  static const char* const who = "kx_run_records_fd_field_values";
  if (!o || !ranges) return setErr(KX_E_ARG, "null argument");
  if (!kxFieldListIsNormal(ranges, n_ranges))
    return setErr(KX_E_ARG, std::string(who) + ": the field list is not in normal form (1 to 8 ranges: sorted, disjoint, not adjacent, only the last open)");
  if (const int rc = checkRecordsOpts(*o, who, fs)) return rc;
  if (o->mode != KX_RECORDS_QUOTED && o->mode != KX_RECORDS_ESCAPED) return setErr(KX_E_ARG, std::string(who) + ": values need a quote or an escape byte");
  return runRecordsFd(p, in_fd, out_fd, *o, report_fd, stats, 0, fs, ranges, n_ranges, true);
}

extern "C" int kx_run_records_fd_field_words(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, const kx_field_range* ranges,
                                             uint32_t n_ranges, int unquote, int report_fd, kx_records_stats* stats) {
  static const char* const who = "kx_run_records_fd_field_words";
  if (!o || !ranges) return setErr(KX_E_ARG, "null argument");
  if (!kxFieldListIsNormal(ranges, n_ranges))
    return setErr(KX_E_ARG, std::string(who) + ": the field list is not in normal form (1 to 8 ranges: sorted, disjoint, not adjacent, only the last open)");
  if (const int rc = checkRecordsOpts(*o, who, -1, true)) return rc;
  if (unquote && o->mode != KX_RECORDS_QUOTED && o->mode != KX_RECORDS_ESCAPED) return setErr(KX_E_ARG, std::string(who) + ": values need a quote or an escape byte");
  return runRecordsFd(p, in_fd, out_fd, *o, report_fd, stats, 0, 0, ranges, n_ranges, unquote != 0, true);
}

extern "C" int kx_run_records_fd_field_project(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, const kx_field_range* items,
                                               uint32_t n_items, uint8_t fs, const uint8_t* ofs, uint32_t ofs_len, uint32_t flags, int report_fd,
                                               kx_records_stats* stats) {
  static const char* const who = "kx_run_records_fd_field_project";
  auto no = [&](const char* what) { return setErr(KX_E_ARG, std::string(who) + ": " + what); };
  if (!o || !items || (ofs_len && !ofs)) return setErr(KX_E_ARG, "null argument");
  if (flags & ~(KX_PROJECT_WORDS | KX_PROJECT_UNQUOTE)) return no("unknown flag bits");
  if (!kxFieldItemsAreValid(items, n_items)) return no("the list as written has 1 to 16 items, each with lo >= 1 and hi = 0 (open) or hi >= lo");
  if (ofs_len > 8) return no("the output field separator is at most 8 bytes");
  kx_field_range ranges[KX_FIELD_RANGES] = {};
  uint32_t n_ranges = 0;
  if (kxFieldItemsUnion(items, n_items, ranges, &n_ranges)) return no("the items' union has more than 8 ranges in its normal form");
  const bool words = (flags & KX_PROJECT_WORDS) != 0, unquote = (flags & KX_PROJECT_UNQUOTE) != 0;
  if (const int rc = words ? checkRecordsOpts(*o, who, -1, true) : checkRecordsOpts(*o, who, fs)) return rc;
  if (unquote) {
    if (o->mode != KX_RECORDS_QUOTED && o->mode != KX_RECORDS_ESCAPED) return no("values need a quote or an escape byte");
    if (ofs_len != 1) return no("on values the output field separator is exactly one byte");
    if (ofs[0] == o->sep) return no("the output field separator cannot be the record separator");
    if ((int)ofs[0] == o->quote) return no("the output field separator cannot be the quote byte");
    if (o->mode == KX_RECORDS_ESCAPED && (int)ofs[0] == o->escape) return no("the output field separator cannot be the escape byte");
    if (words && ofs[0] == 0x09) return no("on the values of words the output field separator cannot be the tab");
  }
  kx_field_project pr{};
  pr.size = sizeof pr; pr.n_items = n_items; pr.ofs_len = ofs_len; pr.flags = words ? KX_PROJECT_WORDS : 0u;
  memcpy(pr.items, items, n_items * sizeof(kx_field_range));
  if (ofs_len) memcpy(pr.ofs, ofs, ofs_len);
  return runRecordsFd(p, in_fd, out_fd, *o, report_fd, stats, 0, words ? (uint8_t)0 : fs, ranges, n_ranges, unquote, words, &pr);
}

extern "C" int kx_run_records_fd_field_keys(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, const kx_field_keys* keys, uint8_t fs,
                                            const uint32_t* items, uint32_t n_items, const uint8_t* ofs, uint32_t ofs_len, int report_fd,
                                            kx_records_stats* stats) {
  static const char* const who = "kx_run_records_fd_field_keys";
  auto no = [&](const char* what) { return setErr(KX_E_ARG, std::string(who) + ": " + what); };
  if (!o || !keys) return setErr(KX_E_ARG, "null argument");
  if (keys->size != sizeof(kx_field_keys)) return no("kx_field_keys::size is not this library's");
  if (keys->flags & ~(KX_KEYS_WORDS | KX_KEYS_UNQUOTE | KX_KEYS_ONLY)) return no("unknown flag bits");
  const bool words = (keys->flags & KX_KEYS_WORDS) != 0, unquote = (keys->flags & KX_KEYS_UNQUOTE) != 0, only = (keys->flags & KX_KEYS_ONLY) != 0;
  if (only && (!items || (ofs_len && !ofs))) return setErr(KX_E_ARG, "null argument");
  if (const int rc = words ? checkRecordsOpts(*o, who, -1, true) : checkRecordsOpts(*o, who, fs)) return rc;
  if (unquote && o->mode != KX_RECORDS_QUOTED && o->mode != KX_RECORDS_ESCAPED) return no("values need a quote or an escape byte");
  kx_field_keys k = *keys;
  k.flags = words ? KX_KEYS_WORDS : 0u;
  kx_batch_field_list fr{};   // the framing the batch calls will have, for the keys' own rules
  fr.size = sizeof fr; fr.fs = words ? (uint8_t)0 : fs;
  fr.quote = o->mode == KX_RECORDS_QUOTED || o->mode == KX_RECORDS_ESCAPED ? o->quote : -1;
  fr.escape = o->mode == KX_RECORDS_ESCAPED ? o->escape : -1;
  if (const int rc = checkFieldKeys(k, fr, o->mode != KX_RECORDS_RS ? (int)o->sep : o->rs_len == 1 ? (int)o->rs[0] : -1, who)) return rc;
  kx_field_project pr{};
  if (only) {
    if (n_items < 1 || n_items > KX_FIELD_ITEMS) return no("the list as written has 1 to 16 items");
    if (ofs_len > 8) return no("the output field separator is at most 8 bytes");
    pr.size = sizeof pr; pr.n_items = n_items; pr.ofs_len = ofs_len; pr.flags = words ? KX_PROJECT_WORDS : 0u;
    for (uint32_t j = 0; j < n_items; ++j) {
      if (items[j] >= k.n_names) return no("an item is the index of a name");
      pr.items[j] = kx_field_range{0u, items[j]};
    }
    if (ofs_len) memcpy(pr.ofs, ofs, ofs_len);
    if (unquote) {
      if (ofs_len != 1) return no("on values the output field separator is exactly one byte");
      if (ofs[0] == o->sep) return no("the output field separator cannot be the record separator");
      if ((int)ofs[0] == o->quote) return no("the output field separator cannot be the quote byte");
      if (o->mode == KX_RECORDS_ESCAPED && (int)ofs[0] == o->escape) return no("the output field separator cannot be the escape byte");
      if (words && ofs[0] == 0x09) return no("on the values of words the output field separator cannot be the tab");
    }
  }
  return runRecordsFd(p, in_fd, out_fd, *o, report_fd, stats, 0, words ? (uint8_t)0 : fs, nullptr, 0, unquote, words, only ? &pr : nullptr, nullptr, who, &k);
}

namespace {

// the rules of a kx_records_table beside its options, found before any device work
int checkTable(const kx_records_opts& o, const kx_records_table& t, const char* who) {
  auto no = [&](const char* what) { return setErr(KX_E_ARG, std::string(who) + ": " + what); };
  if (t.size != sizeof(kx_records_table)) return no("kx_records_table::size is not this library's");
  if (t.pad[0] || t.pad[1] || t.pad[2]) return no("reserved words must be 0");
  for (uint32_t r : t.reserved) if (r) return no("reserved words must be 0");
  if (t.flags & ~(KX_TABLE_WORDS | KX_TABLE_UNQUOTE | KX_TABLE_ONLY | KX_TABLE_SINGLE)) return no("unknown flag bits");
  if (t.n_items > KX_FIELD_ITEMS) return no("at most 16 items");
  if (t.n_names > KX_FIELD_ITEMS) return no("at most 16 names");
  if (t.ofs_len > 8) return no("the output field separator is at most 8 bytes");
  if (!t.n_items && t.flags) return no("flags need items");
  for (uint32_t j = 0; j < t.n_names; ++j) {
    if (!t.names[j]) return no("a null name pointer");
    if (t.name_len[j] < 1 || t.name_len[j] > KX_FIELD_NAME_MAX) return no("a name has 1 to 255 bytes");
  }
  bool named = false;
  for (uint32_t j = 0; j < t.n_items; ++j) {
    const kx_field_range& it = t.items[j];
    if (it.lo == 0) {
      named = true;
      if (it.hi >= t.n_names) return no("a name index is not below n_names");
    } else if (it.hi != 0 && it.hi < it.lo) {
      return no("a number item needs hi = 0 (open) or hi >= lo");
    }
  }
  if (named && !t.header) return no("names need header >= 1");
  if ((t.flags & KX_TABLE_SINGLE) && (t.flags != KX_TABLE_SINGLE || t.n_items != 1 || t.items[0].lo == 0 || t.items[0].hi != t.items[0].lo))
    return no("KX_TABLE_SINGLE comes alone, with one closed number item K-K");
  const bool words = (t.flags & KX_TABLE_WORDS) != 0, unquote = (t.flags & KX_TABLE_UNQUOTE) != 0, only = (t.flags & KX_TABLE_ONLY) != 0;
  if (const int rc = words ? checkRecordsOpts(o, who, -1, true) : checkRecordsOpts(o, who, t.n_items ? (int)t.fs : -1)) return rc;
  if (unquote && o.mode != KX_RECORDS_QUOTED && o.mode != KX_RECORDS_ESCAPED) return no("values need a quote or an escape byte");
  if (only && unquote) {
    if (t.ofs_len != 1) return no("on values the output field separator is exactly one byte");
    if (t.ofs[0] == o.sep) return no("the output field separator cannot be the record separator");
    if ((int)t.ofs[0] == o.quote) return no("the output field separator cannot be the quote byte");
    if (o.mode == KX_RECORDS_ESCAPED && (int)t.ofs[0] == o.escape) return no("the output field separator cannot be the escape byte");
    if (words && t.ofs[0] == 0x09) return no("on the values of words the output field separator cannot be the tab");
  }
  if (t.n_items && !named) {
    kx_field_range u[KX_FIELD_RANGES] = {};
    uint32_t nu = 0;
    if (kxFieldItemsUnion(t.items, t.n_items, u, &nu)) return no("the items' union has more than 8 ranges in its normal form");
  }
  return 0;
}

}  // namespace

extern "C" int kx_run_records_fd_table(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, const kx_records_table* t, int report_fd,
                                       kx_records_stats* stats) {
  static const char* const who = "kx_run_records_fd_table";
  if (!o || !t) return setErr(KX_E_ARG, "null argument");
  if (const int rc = checkTable(*o, *t, who)) return rc;
  const bool words = (t->flags & KX_TABLE_WORDS) != 0, unquote = (t->flags & KX_TABLE_UNQUOTE) != 0, only = (t->flags & KX_TABLE_ONLY) != 0;
  bool named = false;
  for (uint32_t j = 0; j < t->n_items; ++j) named |= t->items[j].lo == 0;
  kx_field_range ranges[KX_FIELD_RANGES] = {};
  uint32_t n_ranges = 0;
  if (t->n_items && !named) (void)kxFieldItemsUnion(t->items, t->n_items, ranges, &n_ranges);
  if (!t->header) {   // exactly the entry point the flags name
    if (!t->n_items) return kx_run_records_fd_opts(p, in_fd, out_fd, o, report_fd, stats);
    if (t->flags & KX_TABLE_SINGLE) return kx_run_records_fd_fields(p, in_fd, out_fd, o, t->items[0].lo, t->fs, report_fd, stats);
    if (only)
      return kx_run_records_fd_field_project(p, in_fd, out_fd, o, t->items, t->n_items, t->fs, t->ofs, t->ofs_len,
                                             (words ? KX_PROJECT_WORDS : 0u) | (unquote ? KX_PROJECT_UNQUOTE : 0u), report_fd, stats);
    if (words) return kx_run_records_fd_field_words(p, in_fd, out_fd, o, ranges, n_ranges, unquote ? 1 : 0, report_fd, stats);
    if (unquote) return kx_run_records_fd_field_values(p, in_fd, out_fd, o, ranges, n_ranges, t->fs, report_fd, stats);
    return kx_run_records_fd_field_list(p, in_fd, out_fd, o, ranges, n_ranges, t->fs, report_fd, stats);
  }
  if (!t->n_items) return runRecordsFd(p, in_fd, out_fd, *o, report_fd, stats, 0, 0, nullptr, 0, false, false, nullptr, t, who);
  if (t->flags & KX_TABLE_SINGLE) return runRecordsFd(p, in_fd, out_fd, *o, report_fd, stats, t->items[0].lo, t->fs, nullptr, 0, false, false, nullptr, t, who);
  kx_field_project pr{};   // (with names its items are filled in when they are resolved)
  pr.size = sizeof pr; pr.n_items = t->n_items; pr.ofs_len = t->ofs_len; pr.flags = words ? KX_PROJECT_WORDS : 0u;
  if (!named) memcpy(pr.items, t->items, sizeof pr.items);
  memcpy(pr.ofs, t->ofs, sizeof pr.ofs);
  return runRecordsFd(p, in_fd, out_fd, *o, report_fd, stats, 0, words ? (uint8_t)0 : t->fs, ranges, n_ranges, unquote, words, only ? &pr : nullptr, t, who);
}
