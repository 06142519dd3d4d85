// kx_batch_host.inc — host driver of batched runs (kx_run_batch, include/kxhip.h; kernels in kx_batch.inc).  Included at the
// end of kx_engine.hip.
//
// Per stage: k_bforward (lane = document) → [the routed documents, one at a time, through the single-document driver] →
// k_bback → scan of the document lengths → k_binit + k_bemit (lane = piece) + k_bplace.  Stage s + 1's batch is stage s's
// output batch (values + offsets); a document rejected at stage s is skipped by the later stages.  Three host round trips per
// stage (routed count, total length, end) plus one for the offset check: the call's fixed cost, whatever the number of documents.
//
// A stage with register actions, kx_config::batch_actions = 2 (kx_batch_actions.inc): the steps above place the documents' TOKEN
// STREAMS in a workspace batch; k_bact_measure → the scan again, now over the replayed lengths → k_bact_lanes + k_bact_waves
// write every document's replayed bytes to their final place.  One more round trip (the replayed total and the class counts).
// With batch_actions = 0 / 1 every document of such a stage goes through batchRouteOne.
//
// A framed batch (kx_run_batch_framed): stage 0 runs the <…, BFrame> instances of the kernels with the frame's trim (every later
// stage and every unframed call the instances without a frame, which are the kernels of before), and the route gets the trimmed lengths.  In the last stage the scan of the output
// lengths counts the suffix for every accepted document and k_bsuffix writes it next to the kernels that place output (inside
// emit_ms, or actions_ms for a replayed stage); the documents' own lengths (BDoc::len, BRoute::len) never include it.
// kx_batch_stats::in_bytes is the bytes of the ranges, the trimmed ones included.

namespace {

constexpr uint32_t BATCH_DOC_MAX_DEFAULT = 64u << 10;

// One document through one stage on the single-document driver (runPipeline's stage body on a shard that is first and last);
// its output is appended at a 16-byte aligned place of W.rout, *pos advanced past it.
int batchRouteOne(kx_program* p, uint32_t st, const uint8_t* d_doc, uint64_t n, hipStream_t sm, BatchWs& W, size_t& pos, BRoute& r) {
  Stage& S = p->stages[st];
  const void* src = d_doc;
  if (n && ((uintptr_t)d_doc & 15)) {   // the shard protocol wants 16-byte aligned input
    int rc = BatchWs::ensure(W.rin, n);
    if (rc) return rc;
    HIPCHECK(hipMemcpyAsync(W.rin.p, d_doc, n, hipMemcpyDeviceToDevice, sm));
    src = W.rin.p;
  }
  kx_shard* s = nullptr;
  int rc = shardBegin(p, st, src, n, 1, 1, sm, &s, true);
  if (rc) return rc;
  struct EndOnExit { kx_shard* s; ~EndOnExit() { kx_shard_end(s); } } end_on_exit{s};
  kx_fwd_summary fs; kx_bwd_summary bs; uint64_t ol = 0;
  rc = kx_shard_forward(s, &fs);
  if (!rc) rc = kx_shard_fix_head(s, 0, &fs);
  if (rc) return rc;
  if (fs.fail_pos != NOFAIL) { r.rejected = 1; r.fail = fs.fail_pos; r.len = 0; return 0; }
  rc = kx_shard_backward(s, &bs);
  if (!rc) rc = kx_shard_resolve(s, 0, &ol);
  if (rc) return rc;
  pos = (pos + 15) & ~(size_t)15;
  if (!S.act) {
    rc = BatchWs::grow(W.rout, pos, pos + ol + 16, sm);
    if (!rc) rc = kx_shard_emit(s, (uint8_t*)W.rout.p + pos, W.rout.cap - pos);
    if (rc) return rc;
    r.start = pos; r.len = ol; pos += ol;
    return 0;
  }
  // a token stream: emit it aside, replay the actions (the stage's ActionRunner, as runPipeline), append the result
  rc = BatchWs::ensure(W.tok, ol + 16);
  if (!rc) rc = kx_shard_emit(s, W.tok.p, W.tok.cap);
  if (rc) return rc;
  if (p->act_runners.size() < p->stages.size()) p->act_runners.resize(p->stages.size(), nullptr);
  ActionRunner*& ar = p->act_runners[st];
  if (!ar) { ar = new ActionRunner; ar->cfg = &p->cfg; rc = ar->init(S.act_regs); if (rc) { delete ar; ar = nullptr; return rc; } }
  else if ((rc = ar->reset())) return rc;
  size_t al = 0;
  rc = BatchWs::ensure(W.tokout, ol + ar->slack());
  if (!rc) rc = ar->run((const uint8_t*)W.tok.p, ol, (uint8_t*)W.tokout.p, &al, sm);
  if (!rc) rc = BatchWs::grow(W.rout, pos, pos + al + 16, sm);
  if (rc) return rc;
  if (al) {
    hipLaunchKernelGGL(k_copy_bytes, dim3(64), dim3(256), 0, sm, (uint8_t*)W.rout.p + pos, (const uint8_t*)W.tokout.p, (unsigned long long)al);
    HIPCHECK(hipGetLastError());
  }
  r.start = pos; r.len = al; pos += al;
  return 0;
}

// The batch replay of an action stage (kx_batch_actions.inc): `tok` / `toff` hold the documents' token streams (tok_total bytes),
// W.docs their records.  Measures, scans the replayed lengths into stage_off, and replays every document to its final place:
// the caller's d_out for the last stage, else the stage's workspace batch.  *dst_out / *total_out: where the replayed batch is.
int batchReplay(kx_program* p, uint32_t st, bool last, uint64_t nd, const uint8_t* cur, const unsigned long long* cur_off, const uint8_t* tok,
                const unsigned long long* toff, unsigned long long tok_total, unsigned long long* stage_off, void* d_out, size_t cap, size_t* out_len,
                unsigned long long nr, hipStream_t sm, BatchWs& W, kx_batch_stats& bst, uint8_t** dst_out, unsigned long long* total_out,
                BFrame fr, const kx_batch_doc* rec, unsigned long long sfx8, uint32_t sfx) {   // fr: the frame of `cur`; sfx8, sfx: the suffix of every accepted document and its length (last stage)
  Stage& S = p->stages[st];
  const bool timing = p->cfg.collect_timing != 0;
  const uint32_t nregs = S.act_regs;
  const bool small = nregs <= 32;   // (registers the chunk instance of actions_body keeps in LDS)
  const uint32_t mgrid = (uint32_t)std::min<uint64_t>((nd + BACT_MT - 1) / BACT_MT, (uint64_t)p->ncu * 4);
  const uint32_t wgrid_max = (uint32_t)p->ncu * (small ? 32u : 2u);
  const size_t tab_words = (size_t)mgrid * BACT_MT * (BACT_TAB_FRAMES + (nregs > LANE_REGS ? nregs - LANE_REGS : 0));
  int rc = BatchWs::ensure(W.actr, BA_N * 8);
  if (!rc) rc = BatchWs::ensure(W.atab, tab_words * 4);
  if (!rc) rc = BatchWs::ensure(W.awlist, nd * 4);
  if (!rc) rc = BatchWs::ensure(W.adeep, nd * 4);
  if (!rc) rc = BatchWs::ensure(W.aretry, nd * 4);
  if (rc) return rc;
  unsigned long long* actr = (unsigned long long*)W.actr.p;
  BDoc* docs = (BDoc*)W.docs.p;
  HIPCHECK(hipMemsetAsync(actr, 0, BA_N * 8, sm));
  if (timing) HIPCHECK(hipEventRecord(W.ev[8], sm));
  hipLaunchKernelGGL(k_bact_measure, dim3(mgrid), dim3(BACT_MT), 0, sm, tok, toff, (unsigned long long)nd, nregs, p->cfg.act_lanes, docs,
                     (uint32_t*)W.atab.p, (uint32_t*)W.awlist.p, (uint32_t*)W.adeep.p, actr);
  const uint32_t ng = (uint32_t)((nd + 1023) / 1024), g1024 = (uint32_t)((nd + 1 + 1023) / 1024);
  hipLaunchKernelGGL(k_bscan_reduce, dim3(ng), dim3(1024), 0, sm, (unsigned long long)nd, (const BDoc*)docs, (unsigned long long*)W.wsum.p, rec, (unsigned long long)sfx);
  hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(1024), 0, sm, ng, (const unsigned long long*)W.wsum.p, (unsigned long long*)W.woff.p, (Flags*)W.flags.p);
  hipLaunchKernelGGL(k_bscan_down, dim3(g1024), dim3(1024), 0, sm, (unsigned long long)nd, (const BDoc*)docs, (const unsigned long long*)W.woff.p,
                     (const Flags*)W.flags.p, stage_off, rec, (unsigned long long)sfx);
  HIPCHECK(hipGetLastError());
  unsigned long long hc[BA_N] = {}, total = 0;
  HIPCHECK(hipMemcpyAsync(hc, actr, sizeof hc, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(&total, &((Flags*)W.flags.p)->total_len, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  std::vector<uint32_t> ids;
  std::vector<BRoute> routes;
  // the route for the listed documents (`ids`, device list `d_ids`): results in `routes`, their outputs in W.rout from `rpos` on
  size_t rpos = 0;
  auto routeListed = [&](const void* d_ids, unsigned long long n_ids) -> int {
    ids.resize(n_ids);
    HIPCHECK(hipMemcpyAsync(ids.data(), d_ids, n_ids * 4, hipMemcpyDeviceToHost, sm));
    HIPCHECK(hipStreamSynchronize(sm));
    std::sort(ids.begin(), ids.end());
    routes.clear();
    for (uint32_t i : ids) {
      unsigned long long se[2];
      HIPCHECK(hipMemcpyAsync(se, cur_off + i, 16, hipMemcpyDeviceToHost, sm));
      HIPCHECK(hipStreamSynchronize(sm));
      BRoute r{se[0], se[1] - se[0] - (i == fr.whole ? 0ull : fr.trim), i, 0, 0};
      int e = batchRouteOne(p, st, cur + r.start, r.len, sm, W, rpos, r);
      if (e) return e;
      routes.push_back(r);
    }
    return 0;
  };
  if (hc[BA_DEEP]) {   // nested deeper than the replay's 64 frames: the route reports it, as for the document alone
    rc = routeListed(W.adeep.p, hc[BA_DEEP]);
    return rc ? rc : setErr(KX_E_ARG, "register redirections nested deeper than 64");
  }
  uint8_t* dst = nullptr;
  if (last) {
    *out_len = total;
    bst.out_bytes = total;
    if (total > cap || (total && !d_out)) return setErr(KX_E_CAPACITY, "output buffer too small");
    dst = (uint8_t*)d_out;
  } else {
    rc = BatchWs::ensure(W.vals[st & 1], total + 16);
    if (rc) return rc;
    dst = (uint8_t*)W.vals[st & 1].p;
  }
  const unsigned long long nw = hc[BA_WAVES];
  if (total) {
    // the documents' stretches of the two arenas (frames: n + 64, registers: 2 n + 1024 bytes each, as k_actions_lanes sizes them)
    rc = BatchWs::ensure(W.ascr, tok_total + 64 * (size_t)nd + 64);
    if (!rc) rc = BatchWs::ensure(W.aheap, 2 * tok_total + 1024 * (size_t)nd + 1024);
    if (rc) return rc;
    if (hc[BA_REPLAY] > nw)
      hipLaunchKernelGGL(k_bact_lanes, dim3(mgrid), dim3(BACT_MT), 0, sm, tok, toff, (unsigned long long)nd, nregs, (const BDoc*)docs,
                         (const unsigned long long*)stage_off, (uint8_t*)W.ascr.p, (uint8_t*)W.aheap.p, dst, (uint32_t*)W.aretry.p, actr);
    if (nw) {
      const uint32_t wgrid = (uint32_t)std::min<unsigned long long>(nw, wgrid_max);
      rc = BatchWs::ensure(W.astates, (size_t)wgrid * sizeof(ActState));
      if (rc) return rc;
      auto* const wave_kernel = small ? &k_bact_waves<1024, 32> : &k_bact_waves<16384, 256>;   // (the chunk instance / the streaming instance of actions_body)
      hipLaunchKernelGGL(wave_kernel, dim3(wgrid), dim3(64), 0, sm, tok, toff, nregs, (const BDoc*)docs,
                         (const unsigned long long*)stage_off, (const uint32_t*)W.awlist.p, (ActState*)W.astates.p, (uint8_t*)W.ascr.p,
                         (uint8_t*)W.aheap.p, dst, (uint32_t*)W.aretry.p, actr);
    }
    // the documents routed for their length hold their replayed output already
    if (nr) hipLaunchKernelGGL(k_bplace, dim3((uint32_t)nr), dim3(256), 0, sm, (const BRoute*)W.rres.p, (const uint8_t*)W.rout.p, (const unsigned long long*)stage_off, dst);
    // the accepted documents' suffixes (inside actions_ms and total_ms; a retried document's k_bplace below stops before its suffix)
    if (sfx) hipLaunchKernelGGL(k_bsuffix, dim3((uint32_t)((nd + 255) / 256)), dim3(256), 0, sm, (unsigned long long)nd, rec,
                                (const unsigned long long*)stage_off, dst, sfx8, sfx);
  }
  if (timing) HIPCHECK(hipEventRecord(W.ev[9], sm));
  HIPCHECK(hipGetLastError());
  unsigned long long nretry = 0;
  HIPCHECK(hipMemcpyAsync(&nretry, actr + BA_RETRY, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  if (timing) bst.actions_ms += evMs(W.ev[8], W.ev[9]);
  if (nretry) {   // a replay outgrew its document's arena: the route, to the same place (the measured length holds)
    const auto rt0 = std::chrono::steady_clock::now();
    rpos = 0;     // (the long documents' outputs have been placed)
    rc = routeListed(W.aretry.p, nretry);
    if (rc) return rc;
    std::vector<BDoc> hd(1);
    for (const BRoute& r : routes) {
      HIPCHECK(hipMemcpy(hd.data(), docs + r.doc, sizeof(BDoc), hipMemcpyDeviceToHost));
      if (r.rejected || r.len != hd[0].len) return setErr(KX_E_HIP, "kx_run_batch: the batch replay measured a length the single-document route does not give");
    }
    rc = BatchWs::ensure(W.rres, nretry * sizeof(BRoute));
    if (rc) return rc;
    HIPCHECK(hipMemcpyAsync(W.rres.p, routes.data(), nretry * sizeof(BRoute), hipMemcpyHostToDevice, sm));
    hipLaunchKernelGGL(k_bplace, dim3((uint32_t)nretry), dim3(256), 0, sm, (const BRoute*)W.rres.p, (const uint8_t*)W.rout.p, (const unsigned long long*)stage_off, dst);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(sm));
    bst.docs_routed += nretry;
    bst.routed_ms += (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - rt0).count();
  }
  bst.docs_replayed += hc[BA_REPLAY] - nretry;
  *dst_out = dst; *total_out = total;
  return 0;
}

// the shard drivers' per-stage engine choice (delayed form, its back-off, the entry layout), which routed documents may move
struct DfSaved { uint32_t streak, skip; bool armed, given_up; int use_alt; };

}  // namespace

namespace {

// kx_run_batch (frame == nullptr) and kx_run_batch_framed
int runBatch(kx_program* p, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_frame* frame, void* d_out, size_t cap,
             uint64_t* d_out_off, kx_batch_doc* d_docs, size_t* out_len, kx_batch_stats* stats, void* stream) {
  if (!p || !out_len) return setErr(KX_E_ARG, "null argument");
  uint32_t trim = 0, sfx_len = 0;
  bool last_whole = false;
  unsigned long long sfx8 = 0;
  if (frame) {
    if (frame->suffix_len > 8) return setErr(KX_E_ARG, "kx_run_batch_framed: the suffix is at most 8 bytes");
    for (uint32_t r : frame->reserved) if (r) return setErr(KX_E_ARG, "kx_run_batch_framed: reserved words must be 0");
    trim = frame->trim; last_whole = frame->last_whole != 0; sfx_len = frame->suffix_len;
    for (uint32_t i = 0; i < sfx_len; ++i) sfx8 |= (unsigned long long)frame->suffix[i] << (8 * i);
  }
  if (n_docs && (!d_in_off || !d_out_off || !d_docs)) return setErr(KX_E_ARG, "kx_run_batch: offsets, output offsets and document records are required");
  if (n_docs >= 0xFFFFFFFFull) return setErr(KX_E_ARG, "kx_run_batch: at most 2^32 - 2 documents per call");
  *out_len = 0;
  kx_batch_stats bst{};
  bst.docs = n_docs;
  const hipStream_t sm = (hipStream_t)stream;
  if (n_docs == 0) {
    if (d_out_off) { HIPCHECK(hipMemsetAsync(d_out_off, 0, 8, sm)); HIPCHECK(hipStreamSynchronize(sm)); }
    if (stats) *stats = bst;
    return 0;
  }
  if (!p->batch) p->batch = new BatchWs;
  BatchWs& W = *p->batch;
  const bool timing = p->cfg.collect_timing != 0;
  if (!W.have_events) {
    for (auto& e : W.ev) HIPCHECK(hipEventCreate(&e));
    W.have_events = true;
  }
  if (!W.lds_set) {   // (every stage's image fits what kx_load granted the general engine's kernels)
    size_t lds = 0;
    for (auto& s : p->stages) lds = s.lds_bytes > lds ? s.lds_bytes : lds;
    for (const void* fn : {(const void*)k_bforward<false>, (const void*)k_bforward<true>, (const void*)k_bback<false>, (const void*)k_bback<true>,
                           (const void*)k_bemit<false>, (const void*)k_bemit<true>,
                           (const void*)k_bforward<false, BFrame>, (const void*)k_bforward<true, BFrame>, (const void*)k_bback<false, BFrame>,
                           (const void*)k_bback<true, BFrame>, (const void*)k_bemit_fr<false, BFrame>, (const void*)k_bemit_fr<true, BFrame>}) {
      int rc = setLds(fn, lds);
      if (rc) return rc;
    }
    W.lds_set = true;
  }
  const uint32_t ns = (uint32_t)p->stages.size();
  std::vector<DfSaved> saved(ns);
  for (uint32_t i = 0; i < ns; ++i) {
    const Stage& S = p->stages[i];
    saved[i] = DfSaved{S.df_streak, S.df_skip, S.df_slow_armed, S.df_given_up, S.use_alt};
  }
  struct RestoreOnExit {
    kx_program* p; std::vector<DfSaved>& v;
    ~RestoreOnExit() {
      for (size_t i = 0; i < v.size(); ++i) {
        Stage& S = p->stages[i];
        S.df_streak = v[i].streak; S.df_skip = v[i].skip; S.df_slow_armed = v[i].armed; S.df_given_up = v[i].given_up; S.use_alt = v[i].use_alt;
      }
    }
  } restore{p, saved};

  const uint64_t nd = n_docs;
  const uint32_t g1024 = (uint32_t)((nd + 1 + 1023) / 1024);
  int rc = BatchWs::ensure(W.ctr, BC_N * 8);
  if (!rc) rc = BatchWs::ensure(W.flags, sizeof(Flags));
  if (!rc) rc = BatchWs::ensure(W.docs, nd * sizeof(BDoc));
  if (!rc) rc = BatchWs::ensure(W.routes, nd * sizeof(BRoute));
  if (!rc) rc = BatchWs::ensure(W.wsum, (size_t)g1024 * 8);
  if (!rc) rc = BatchWs::ensure(W.woff, (size_t)g1024 * 8);
  if (rc) return rc;
  unsigned long long* ctr = (unsigned long long*)W.ctr.p;
  HIPCHECK(hipMemsetAsync(ctr, 0, BC_N * 8, sm));
  // the offsets: non-decreasing, checked on the device before any kernel reads a document; the caller's records cleared
  // (a framed batch: also that no range is shorter than what the frame cuts from it)
  const BFrame fr0{trim, trim && last_whole ? nd - 1 : BATCH_NO_WHOLE};
  if (trim) hipLaunchKernelGGL(k_bcheck<BFrame>, dim3((uint32_t)((nd + 255) / 256)), dim3(256), 0, sm, (const unsigned long long*)d_in_off,
                               (unsigned long long)nd, d_docs, ctr, fr0);
  else hipLaunchKernelGGL(k_bcheck<>, dim3((uint32_t)((nd + 255) / 256)), dim3(256), 0, sm, (const unsigned long long*)d_in_off, (unsigned long long)nd, d_docs, ctr);
  HIPCHECK(hipGetLastError());
  unsigned long long hc[BC_N] = {0, 0, 0, 0}, ends[2] = {0, 0};
  HIPCHECK(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(&ends[0], d_in_off, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipMemcpyAsync(&ends[1], d_in_off + nd, 8, hipMemcpyDeviceToHost, sm));
  HIPCHECK(hipStreamSynchronize(sm));
  if (hc[BC_BADOFF] || ends[1] < ends[0]) return setErr(KX_E_ARG, "kx_run_batch: the document offsets decrease");
  if (hc[BC_SHORT]) return setErr(KX_E_ARG, "kx_run_batch_framed: a document's range is shorter than the trim");
  if (ends[1] > ends[0] && !d_in) return setErr(KX_E_ARG, "kx_run_batch: null input");
  bst.in_bytes = ends[1] - ends[0];

  const uint64_t doc_max = p->cfg.batch_doc_max ? p->cfg.batch_doc_max : BATCH_DOC_MAX_DEFAULT;
  const uint32_t bgrid = (uint32_t)p->ncu * 4;
  const uint8_t* cur = (const uint8_t*)d_in;
  const unsigned long long* cur_off = (const unsigned long long*)d_in_off;
  uint64_t cur_bytes = bst.in_bytes;
  std::vector<BRoute> routes;
  for (uint32_t st = 0; st < ns && rc == 0; ++st) {
    Stage& S = p->stages[st];
    const bool last = st + 1 == ns;
    const bool wide = S.general;
    const bool replay = S.act && p->cfg.batch_actions == 2;   // the batch replay; else every document of an action stage is routed
    const size_t lds = S.lds_bytes;
    const bool framed = st == 0 && trim != 0;                   // the <…, BFrame> instances: stage 0 of a batch with a trim
    const BFrame fr = framed ? fr0 : BFrame{0, BATCH_NO_WHOLE};
    const unsigned long long sfx = last ? sfx_len : 0;          // what the scan of the stage's OUTPUT lengths adds per accepted document
    const uint64_t nchk = (cur_bytes >> 5) + nd + 2, nslots = (cur_bytes >> 6) + nd;   // (k_bback writes every piece slot below nslots)
    rc = BatchWs::ensure(W.chk, nchk * 2);
    if (!rc) rc = BatchWs::ensure(W.brec, (nslots + 1) * sizeof(BRec));
    if (rc) break;
    unsigned long long* out_off = last ? (unsigned long long*)d_out_off : nullptr;
    if (!last) { rc = BatchWs::ensure(W.offs[st & 1], (nd + 1) * 8); if (rc) break; out_off = (unsigned long long*)W.offs[st & 1].p; }
    unsigned long long* const stage_off = out_off;   // (where the stage's output offsets go)
    if (replay) { rc = BatchWs::ensure(W.atoff, (nd + 1) * 8); if (rc) break; out_off = (unsigned long long*)W.atoff.p; }   // first the token streams'
    BDoc* docs = (BDoc*)W.docs.p; BRec* brec = (BRec*)W.brec.p; uint16_t* chk = (uint16_t*)W.chk.p;
    // forward: lane = document
    HIPCHECK(hipMemsetAsync(ctr + BC_ROUTED, 0, 8, sm));
    if (timing) HIPCHECK(hipEventRecord(W.ev[0], sm));
    if (framed)
      hipLaunchKernelGGL((wide ? k_bforward<true, BFrame> : k_bforward<false, BFrame>), dim3(bgrid), dim3(BATCH_BT), lds, sm, cur, cur_off, (unsigned long long)nd,
                         (unsigned long long)doc_max, S.act && !replay ? 1 : 0, st, (BDoc*)W.docs.p, d_docs, chk, (BRoute*)W.routes.p, ctr, S.T, fr);
    else
      hipLaunchKernelGGL(wide ? k_bforward<true> : k_bforward<false>, dim3(bgrid), dim3(BATCH_BT), lds, sm, cur, cur_off, (unsigned long long)nd,
                         (unsigned long long)doc_max, S.act && !replay ? 1 : 0, st, (BDoc*)W.docs.p, d_docs, chk, (BRoute*)W.routes.p, ctr, S.T);
    if (timing) HIPCHECK(hipEventRecord(W.ev[1], sm));
    HIPCHECK(hipGetLastError());
    unsigned long long nr = 0;
    HIPCHECK(hipMemcpyAsync(&nr, ctr + BC_ROUTED, 8, hipMemcpyDeviceToHost, sm));
    HIPCHECK(hipStreamSynchronize(sm));
    if (timing) bst.forward_ms += evMs(W.ev[0], W.ev[1]);
    // backward: lane = document
    if (timing) HIPCHECK(hipEventRecord(W.ev[2], sm));
    if (framed)
      hipLaunchKernelGGL((wide ? k_bback<true, BFrame> : k_bback<false, BFrame>), dim3(bgrid), dim3(BATCH_BT), lds, sm, cur, cur_off, (unsigned long long)nd, docs,
                         chk, brec, S.T, fr);
    else
      hipLaunchKernelGGL(wide ? k_bback<true> : k_bback<false>, dim3(bgrid), dim3(BATCH_BT), lds, sm, cur, cur_off, (unsigned long long)nd, docs, chk, brec, S.T);
    if (timing) HIPCHECK(hipEventRecord(W.ev[3], sm));
    HIPCHECK(hipGetLastError());
    // the routed documents, one at a time (in document order)
    size_t rpos = 0;
    routes.resize(nr);
    if (nr) {
      const auto rt0 = std::chrono::steady_clock::now();
      HIPCHECK(hipMemcpyAsync(routes.data(), W.routes.p, nr * sizeof(BRoute), hipMemcpyDeviceToHost, sm));
      HIPCHECK(hipStreamSynchronize(sm));
      std::sort(routes.begin(), routes.end(), [](const BRoute& a, const BRoute& b) { return a.doc < b.doc; });
      for (BRoute& r : routes) {
        rc = batchRouteOne(p, st, cur + r.start, r.len, sm, W, rpos, r);
        if (rc) break;
      }
      if (rc) break;
      bst.docs_routed += nr;
      rc = BatchWs::ensure(W.rres, nr * sizeof(BRoute));
      if (rc) break;
      HIPCHECK(hipMemcpyAsync(W.rres.p, routes.data(), nr * sizeof(BRoute), hipMemcpyHostToDevice, sm));
      hipLaunchKernelGGL(k_broute_set, dim3((uint32_t)((nr + 255) / 256)), dim3(256), 0, sm, (uint32_t)nr, (const BRoute*)W.rres.p, st, docs, d_docs, ctr);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipStreamSynchronize(sm));
      bst.routed_ms += (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - rt0).count();
    }
    // exclusive scan of the document lengths into `off` (off[nd] = the total, also left in Flags::total_len)
    const uint32_t ng = (uint32_t)((nd + 1023) / 1024);
    auto scanDocs = [&](unsigned long long* off, unsigned long long add) {
      hipLaunchKernelGGL(k_bscan_reduce, dim3(ng), dim3(1024), 0, sm, (unsigned long long)nd, (const BDoc*)docs, (unsigned long long*)W.wsum.p,
                         (const kx_batch_doc*)d_docs, add);
      hipLaunchKernelGGL(k_scan_groups, dim3(1), dim3(1024), 0, sm, ng, (const unsigned long long*)W.wsum.p, (unsigned long long*)W.woff.p, (Flags*)W.flags.p);
      hipLaunchKernelGGL(k_bscan_down, dim3(g1024), dim3(1024), 0, sm, (unsigned long long)nd, (const BDoc*)docs, (const unsigned long long*)W.woff.p,
                         (const Flags*)W.flags.p, off, (const kx_batch_doc*)d_docs, add);
    };
    if (timing) HIPCHECK(hipEventRecord(W.ev[4], sm));
    scanDocs(out_off, replay ? 0 : sfx);   // (a replayed stage: these are the token streams' lengths; batchReplay's scan adds the suffix)
    if (timing) HIPCHECK(hipEventRecord(W.ev[5], sm));
    HIPCHECK(hipGetLastError());
    unsigned long long total = 0;
    HIPCHECK(hipMemcpyAsync(&total, &((Flags*)W.flags.p)->total_len, 8, hipMemcpyDeviceToHost, sm));
    HIPCHECK(hipStreamSynchronize(sm));
    if (timing) { bst.back_ms += evMs(W.ev[2], W.ev[3]); bst.scan_ms += evMs(W.ev[4], W.ev[5]); }
    uint8_t* dst = nullptr;
    if (replay) {   // (the token streams: a workspace batch, whatever the stage's position)
      rc = BatchWs::ensure(W.atok, total + 16);
      if (rc) break;
      dst = (uint8_t*)W.atok.p;
    } else if (last) {
      *out_len = total;
      bst.out_bytes = total;
      if (total > cap || (total && !d_out)) { rc = setErr(KX_E_CAPACITY, "output buffer too small"); break; }
      dst = (uint8_t*)d_out;
    } else {
      rc = BatchWs::ensure(W.vals[st & 1], total + 16);
      if (rc) break;
      dst = (uint8_t*)W.vals[st & 1].p;
    }
    // placing: the initial constants, every piece (lane = piece), the routed documents' outputs
    if (timing) HIPCHECK(hipEventRecord(W.ev[6], sm));
    if (total) {
      hipLaunchKernelGGL(k_binit, dim3(bgrid), dim3(256), 0, sm, (unsigned long long)nd, (const BDoc*)docs, (const unsigned long long*)out_off, dst, S.T);
      const uint64_t eg = (nslots + BATCH_BT - 1) / BATCH_BT;
      if (framed)
        hipLaunchKernelGGL((wide ? k_bemit_fr<true, BFrame> : k_bemit_fr<false, BFrame>), dim3((uint32_t)(eg < bgrid ? eg : bgrid)), dim3(BATCH_BT), lds, sm, cur, cur_off,
                           (unsigned long long)nslots, (const BDoc*)docs, (const uint16_t*)chk, (const BRec*)brec, (const unsigned long long*)out_off, dst, S.T, fr);
      else
        hipLaunchKernelGGL(wide ? k_bemit<true> : k_bemit<false>, dim3((uint32_t)(eg < bgrid ? eg : bgrid)), dim3(BATCH_BT), lds, sm, cur, cur_off,
                           (unsigned long long)nslots, (const BDoc*)docs, (const uint16_t*)chk, (const BRec*)brec, (const unsigned long long*)out_off, dst, S.T);
      // (a replayed stage's routed documents hold their REPLAYED output: placed behind the replay, below)
      if (nr && !replay) hipLaunchKernelGGL(k_bplace, dim3((uint32_t)nr), dim3(256), 0, sm, (const BRoute*)W.rres.p, (const uint8_t*)W.rout.p, (const unsigned long long*)out_off, dst);
      // the accepted documents' suffixes (inside emit_ms and total_ms; a replayed stage's are written by batchReplay)
      if (sfx && !replay) hipLaunchKernelGGL(k_bsuffix, dim3((uint32_t)((nd + 255) / 256)), dim3(256), 0, sm, (unsigned long long)nd, (const kx_batch_doc*)d_docs,
                                             (const unsigned long long*)out_off, dst, sfx8, sfx_len);
    }
    if (timing) HIPCHECK(hipEventRecord(W.ev[7], sm));
    HIPCHECK(hipGetLastError());
    if (replay) {
      rc = batchReplay(p, st, last, nd, cur, cur_off, (const uint8_t*)dst, out_off, total, stage_off, d_out, cap, out_len, nr, sm, W, bst, &dst, &total,
                       fr, (const kx_batch_doc*)d_docs, sfx8, (uint32_t)sfx);
      if (rc) break;
      out_off = stage_off;
    }
    HIPCHECK(hipStreamSynchronize(sm));
    if (timing) { bst.emit_ms += evMs(W.ev[6], W.ev[7]); bst.total_ms += evMs(W.ev[0], replay ? W.ev[9] : W.ev[7]); }
    cur = dst; cur_off = out_off; cur_bytes = total;
  }
  if (rc == 0 || rc == KX_E_CAPACITY) {
    unsigned long long rej = 0;
    HIPCHECK(hipMemcpyAsync(&rej, ctr + BC_REJECTED, 8, hipMemcpyDeviceToHost, sm));
    HIPCHECK(hipStreamSynchronize(sm));
    bst.docs_rejected = rej;
    if (rc == 0 && rej) rc = KX_MATCH_ERROR;
  }
  if (stats) *stats = bst;
  return rc;
}

}  // namespace

extern "C" int kx_run_batch(kx_program* p, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, void* d_out, size_t cap,
                            uint64_t* d_out_off, kx_batch_doc* d_docs, size_t* out_len, kx_batch_stats* stats, void* stream) {
  return runBatch(p, d_in, d_in_off, n_docs, nullptr, d_out, cap, d_out_off, d_docs, out_len, stats, stream);
}

extern "C" int kx_run_batch_framed(kx_program* p, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_frame* frame,
                                   void* d_out, size_t cap, uint64_t* d_out_off, kx_batch_doc* d_docs, size_t* out_len, kx_batch_stats* stats,
                                   void* stream) {
  return runBatch(p, d_in, d_in_off, n_docs, frame, d_out, cap, d_out_off, d_docs, out_len, stats, stream);
}
