// kx_dfkernels.inc — device side of the DELAYED FORM (kx_delayed.h has the construction and the argument).  Included by
// kx_engine.hip inside its anonymous namespace, behind k_emit (it shares put_bytes, wave_scan_incl, load_piece, …).
//
//   k_dforward  lane = segment (as k_forward): the product state sequence from the segment's synchronisation point; per 64-byte
//               piece one 8-byte record {state entering the piece, state in its middle, output bytes of the piece and of its
//               first half, constants of either half} (DfRec); per 32 pieces one word: the output bytes of the block part before
//               the first of them (the WAVE BASE array); per block the output bytes of its two parts
//   k_dlen      block length = own part + spill part; the existing k_scan_* turn them into offsets
//   k_demit     lane = piece, persistent: ONE forward walk per piece that places the output as it goes (two chains, from the
//               two recorded states, write cursors running UP from the piece's output offset = the wave-iteration's base + the
//               prefix sum of the lengths of the pieces before it in the wave: the output is contiguous); staging, constants as
//               jobs and the flush are k_emit's
// Table image in LDS (address 0): class*8 u8[256] (class index where class*8 does not fit: DfDev::wide) | rows of C x {lo, hi}: lo = handle of the next state (its row's LDS address),
// hi = what this step writes, in the layout of a path entry of the general engine's `direct` form: bit 0 "no input byte
// copied", bits 10-22 the constant's pool offset / 16, bit 23 "a constant follows", bits 24-30 bytes appended (copy included).
// The copied byte of step s is input byte s-K.

// (struct DfDev: kx_stage.h, with the host code that fills it)
// A piece that the slow path resolved has no states to walk from: its record names a run of SIDE ENTRIES instead (one per path
// step: bit 0 copy, bits 1-30 the constant (>= sl_npc: none), bit 31 an entry without an input byte — a constant that was due),
// and k_demit's lane replays them straight into the output (a hole record, below).
constexpr uint32_t DF_HOLE_MAX = 4096, DF_HOLE_FIRST = 1024, DF_SL_LEAVES = 32;
// THE PIECE RECORD, 8 bytes.  The widths are the image's own limits (kx_delayed.h; dfRecFits checks them when a stage is loaded):
//   row handles   multiples of 8 below 64 KiB (rows of C x 8 bytes behind the 256-byte class table): handle >> 3 in 13 bits
//   len, lenA     bytes appended by the piece / by its first half: a step appends at most DF_STEP_MAX = 126 bytes (the entry's
//                 7-bit field, 127 never built), so len <= 64 * 126 fits 13 bits and lenA <= 32 * 126 fits 12
//   kA, kB        constants of the first / second half: at most 32 each, 6 bits
//   x = start >> 3 | middle >> 3 << 13 | kA << 26          y = len | lenA << 13 | kB << 25 | hole << 31
// A hole record:  x = index of the piece's first side entry       y = len (16 bits) | entries << 16 (14 bits) | first << 30 | 1 << 31
// (first: the first piece of a stretch, which also writes the K pending steps).  A piece has at most 64 + DF_MAX_K + (constants
// due) entries; a stretch with a piece beyond 16 bits of output or 14 bits of entries is "not resolvable here".
// Where a piece's output starts is not in its record: the output is contiguous, so k_demit adds up the lengths of the pieces in
// front of it in its wave-iteration, from ONE absolute offset per iteration: wbase[piece / 32] = the block-relative offset of
// every 32nd piece (bytes its block part — own or spill — holds before it) | DFREC_OWN if that part is the block's own.
struct __attribute__((aligned(8))) DfRec { uint32_t x, y; };
constexpr uint32_t DFREC_OWN = 0x80000000u, DFREC_HOLE = 0x80000000u, DFREC_HOLE_FIRST = 0x40000000u;
constexpr uint32_t DF_MERGE_WINDOW_MAX = 64;   // the largest kx_config::merge_window (window J + 1)
using kxst::DF_STEP_MAX;   // (kx_stage.h: dfRecFits checks an image against it when a stage is loaded)
constexpr uint32_t DF_HOLE_LEN_MAX = 0xFFFFu, DF_HOLE_CNT_MAX = 0x3FFFu, DF_WBASE_PIECES = 32;
constexpr DfRec dfrec_pack(uint32_t start, uint32_t middle, uint32_t lenA, uint32_t len, uint32_t kA, uint32_t kB) {
  return DfRec{(start >> 3) | ((middle >> 3) << 13) | (kA << 26), len | (lenA << 13) | (kB << 25)};
}
constexpr DfRec dfrec_pack_hole(uint32_t side_first, uint32_t entries, bool first, uint32_t len) {
  return DfRec{side_first, len | (entries << 16) | (first ? DFREC_HOLE_FIRST : 0u) | DFREC_HOLE};
}
constexpr bool dfrec_hole(DfRec r) { return (r.y & DFREC_HOLE) != 0; }
constexpr uint32_t dfrec_start(DfRec r) { return (r.x & 0x1FFFu) << 3; }
constexpr uint32_t dfrec_middle(DfRec r) { return ((r.x >> 13) & 0x1FFFu) << 3; }
constexpr uint32_t dfrec_kA(DfRec r) { return r.x >> 26; }
constexpr uint32_t dfrec_kB(DfRec r) { return (r.y >> 25) & 0x3Fu; }
constexpr uint32_t dfrec_len(DfRec r) { return r.y & 0x1FFFu; }
constexpr uint32_t dfrec_lenA(DfRec r) { return (r.y >> 13) & 0xFFFu; }
constexpr uint32_t dfrec_hole_side(DfRec r) { return r.x; }
constexpr uint32_t dfrec_hole_len(DfRec r) { return r.y & DF_HOLE_LEN_MAX; }
constexpr uint32_t dfrec_hole_entries(DfRec r) { return (r.y >> 16) & DF_HOLE_CNT_MAX; }
constexpr bool dfrec_hole_first(DfRec r) { return (r.y & DFREC_HOLE_FIRST) != 0; }
namespace dfrec_check {
constexpr uint32_t H = 65536 - 8, LA = HALF * DF_STEP_MAX, LN = PIECE * DF_STEP_MAX, KH = HALF;
constexpr DfRec top = dfrec_pack(H, H, LA, LN, KH, KH), one = dfrec_pack(8, 65536 - 16, 1, 2, 0, KH), zero = dfrec_pack(0, 0, 0, 0, 0, 0);
static_assert(sizeof(DfRec) == 8 && LN < (1u << 13) && LA < (1u << 12) && KH < (1u << 6), "piece record: a field outgrew its width");
static_assert(!dfrec_hole(top) && dfrec_start(top) == H && dfrec_middle(top) == H && dfrec_lenA(top) == LA && dfrec_len(top) == LN &&
              dfrec_kA(top) == KH && dfrec_kB(top) == KH, "piece record: every field at its maximum");
static_assert(!dfrec_hole(one) && dfrec_start(one) == 8 && dfrec_middle(one) == 65536 - 16 && dfrec_lenA(one) == 1 && dfrec_len(one) == 2 &&
              dfrec_kA(one) == 0 && dfrec_kB(one) == KH, "piece record: neighbouring fields do not bleed");
static_assert(!dfrec_hole(zero) && zero.x == 0 && zero.y == 0, "piece record: all fields zero");
constexpr DfRec htop = dfrec_pack_hole(0xFFFFFFFFu, DF_HOLE_CNT_MAX, true, DF_HOLE_LEN_MAX), hlow = dfrec_pack_hole(0, 0, false, 0);
static_assert(dfrec_hole(htop) && dfrec_hole_side(htop) == 0xFFFFFFFFu && dfrec_hole_entries(htop) == DF_HOLE_CNT_MAX && dfrec_hole_first(htop) &&
              dfrec_hole_len(htop) == DF_HOLE_LEN_MAX, "hole record: every field at its maximum");
static_assert(dfrec_hole(hlow) && dfrec_hole_side(hlow) == 0 && dfrec_hole_entries(hlow) == 0 && !dfrec_hole_first(hlow) && dfrec_hole_len(hlow) == 0, "hole record: all fields zero");
// entries of a piece: its 64 steps; the first piece of a stretch adds the K pending steps and the constants its state has due.  A
// constant waits at most J steps (J = kx_config::merge_window - 1 <= DF_MERGE_WINDOW_MAX - 1, checkConfig) and at most one joins per
// step: at most DF_MERGE_WINDOW_MAX are due.  (The 16-byte record had 15 bits for this count; 14 hold it with room to spare, and the
// slow path checks the count of every piece it records all the same.)
static_assert(PIECE + kxdf::DF_MAX_K + DF_MERGE_WINDOW_MAX <= DF_HOLE_CNT_MAX, "hole record: the entries of a piece fit");
static_assert((uint64_t)MAX_SEG * DF_STEP_MAX < DFREC_OWN, "wave base: a block part's output stays below the own flag");
static_assert(DF_WBASE_PIECES == HALF && 2 * DF_WBASE_PIECES == PIECE, "wave base: one word per wave-iteration of half pieces, two per iteration of pieces");
}  // namespace dfrec_check
struct DfLds {
  const uint8_t* base; uint32_t csh;
  __device__ __forceinline__ uint32_t c8(uint32_t byte) const { return (uint32_t)base[byte] << csh; }
  __device__ __forceinline__ uint2 ent(uint32_t a) const { return *reinterpret_cast<const uint2*>(base + a); }
};
__device__ __forceinline__ DfLds df_stage(const DfDev& D, uint32_t* smem) {
  for (uint32_t i = threadIdx.x; i < D.words; i += blockDim.x) smem[i] = D.img[i];
  __syncthreads();
  return DfLds{reinterpret_cast<const uint8_t*>(smem), D.wide ? 3u : 0u};
}

// 64 chained product transitions over one piece in registers: state after 32 and after 64 steps, bytes written by the first 32
// steps and by all 64 (compiler-scheduled form; classes are fetched one group of 8 ahead of the dependent chain)
__device__ __forceinline__ void df_run_piece(const uint32_t (&w)[16], uint32_t& h, uint32_t& mid, uint32_t& lenA, uint32_t& len, const DfLds& L) {
  uint32_t c[8], cn[8], sum = 0;
  static_for<0, 8>([&](auto ic) { constexpr int i = decltype(ic)::value; c[i] = L.c8(BYTE_AT_DEP(w, i, h)); });
  static_for<0, PIECE / 8>([&](auto gc) {
    constexpr int g = decltype(gc)::value;
    if constexpr (g + 1 < PIECE / 8)
      static_for<0, 8>([&](auto ic) { constexpr int i = decltype(ic)::value; cn[i] = L.c8(BYTE_AT_DEP(w, 8 * (g + 1) + i, h)); });
    static_for<0, 8>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      const uint2 e = L.ent(h + c[i]);
      h = e.x & 0xFFFFu; sum += e.y >> 24; tie(h, sum);
    });
    if constexpr (g == HALF / 8 - 1) { mid = h; lenA = sum; }
    if constexpr (g + 1 < PIECE / 8)
      static_for<0, 8>([&](auto ic) { constexpr int i = decltype(ic)::value; c[i] = cn[i]; });
  });
  len = sum;
}

// where lane j's own part starts (UNSYNC: it owns nothing and the lane before it runs through): the first piece boundary at
// least K + J symbols behind its synchronisation point — from there on its product state no longer depends on what was pending
// (K symbols) or due (J more: merged constants) before the synchronisation point — provided that lies inside its own segment
__device__ __forceinline__ uint64_t df_own_start(uint32_t j, uint64_t n, uint64_t seg, int first_known, const uint64_t* __restrict__ seg_pos,
                                                 const uint16_t* __restrict__ seg_state, const DfDev& D) {
  if (j == 0 && first_known) return 0;
  const uint64_t p = seg_pos[j];
  if (p == UNSYNC) return UNSYNC;
  const uint32_t q = (((uint32_t)seg_state[j] << D.hshift) - OFF_FWD) / D.orig_c4;
  if (q >= D.nstates || D.start_of_state[q] == 0xFFFFu) return UNSYNC;   // (q == nstates: synchronised on the absorbing "no transition" state — the lane before runs into the failure and reports it)
  const uint64_t b = (p + D.K + D.J + 63) & ~63ull;
  const uint64_t lim = ((uint64_t)j + 1) * seg < n ? ((uint64_t)j + 1) * seg : n;
  return b < lim ? b : UNSYNC;
}

// The resolving half of k_dforward's slow path (see the comment at its call site), kept OUT of line: its arrays and its long
// live ranges would otherwise cost the forward pass's hot loop registers (inlined: 150 spilled registers in k_dforward).
// (The slow path's map leaf -> leaf at the anchor, at most 32 bytes, lives in the lane's own record staging slot in LDS — free while the lane
//  is in here, its records flushed: an array indexed by a run-time value would otherwise go to scratch memory, i.e. through the memory system
//  that the kernel is saturating; kept in 8 registers behind select chains the compiler turned it into an indexed scratch read again.)
struct DfSlowIO {
  const uint8_t* in; uint64_t n, a, end; uint32_t h0, last, is_last;
  uint32_t h_behind; uint32_t* side; uint32_t side_cap; Flags* flags; const uint8_t* lds; uint32_t clsh; uint8_t* lmap; uint32_t max_steps;   // lmap: 64 bytes of LDS of the lane's own   // max_steps: the stretch's room (side entries are handed out before the walk)
  uint32_t base, nd, h_next; uint64_t e_out;   // out
};
__device__ __noinline__ int df_slow_resolve(DfSlowIO& io, const DfDev& D) {
  const uint8_t* __restrict__ in = io.in;
  const uint64_t n = io.n, a = io.a, end = io.end;
  const uint32_t h0 = io.h0;
  const bool last = io.last != 0, is_last = io.is_last != 0;
  uint32_t* side = io.side; const uint32_t side_cap = io.side_cap; Flags* flags = io.flags;
  if (!D.sl_on || !side) return 1;
  const uint32_t C = D.C, Lm = D.sl_Lm, K = D.K, NONE = D.sl_npc << 1;
  const uint32_t i0 = (h0 - 256u) / (C * 8u);
  uint32_t q = D.sl_q[i0];
  const uint32_t nd = D.sl_defoff[i0 + 1] - D.sl_defoff[i0];
  const uint64_t hard = a + io.max_steps < n ? a + io.max_steps : n;
  const uint32_t need = nd + K + (uint32_t)(hard - a) + 64u;
  const uint32_t base = atomicAdd(&flags->side_used, need);
  if ((uint64_t)base + need > side_cap) return 1;
  uint32_t* const E = side + base;
  uint32_t* const R = E + nd + K;   // R[u - a]: a step's back row while it is open, its kind (copy | constant << 1) once decided
  for (uint32_t d = 0; d < nd; ++d) E[d] = 0x80000000u | (D.sl_defpc[D.sl_defoff[i0] + d] << 1);
  uint8_t *M = io.lmap, *M2 = io.lmap + 32;
  uint16_t qb[DF_HOLE_MAX / 64 + 2];   // the SST state at a + 64 i
  uint32_t nl = D.sl_nleaves[q];
  for (uint32_t l = 0; l < DF_SL_LEAVES; ++l) M[l] = (uint8_t)l;
  uint64_t t = a, anchor = a, prev = a, inw = 0;
  // decide the steps [from, to) given the leaf at `to`; returns the leaf at `from`
  auto back_to = [&](uint64_t from, uint64_t to, uint32_t leaf) {
    uint64_t u = to;
    while (u > from) {   // (the rows 8 at a time; the chain is then one load per step)
      const uint32_t cnt = u - from < 8 ? (uint32_t)(u - from) : 8u;
      uint32_t rr[8];
#pragma unroll
      for (uint32_t k2 = 0; k2 < 8; ++k2) rr[k2] = k2 < cnt ? R[u - 1 - k2 - a] : 0u;
#pragma unroll
      for (uint32_t k2 = 0; k2 < 8; ++k2) if (k2 < cnt) {
        const uint32_t e = D.sl_back[(size_t)rr[k2] * Lm + leaf];
        R[u - 1 - k2 - a] = ((e >> 8) & 1u) | ((e >> 9) << 1);
        leaf = e & 0xFFu;
      }
      u -= cnt;
    }
    return leaf;
  };
  bool pend_done = false;
  auto anchor_known = [&](uint32_t leaf) {   // the leaf at `anchor` is known: the stretch behind it is decided
    if (anchor == a) { for (uint32_t jj = 0; jj < K; ++jj) E[nd + jj] = D.sl_pend[((size_t)i0 * K + jj) * Lm + leaf]; pend_done = true; }
    else back_to(prev, anchor, leaf);
  };
  // OUTPUT EQUIVALENCE at a piece boundary t: the leaf there may still be open (apache_log's "another record follows / this was the
  // last one" stay alive for a whole line) while every live leaf writes the SAME bytes on every open step — then the steps are decided
  // without it and the table can take over at t.  The (at most 4) live leaves' chains are walked back together over the open steps
  // [prev, t) (and the pending steps, if still open); on agreement the first chain's kinds are what the steps write.  Without this a
  // stretch ran to the end of the next line and a line further: ≈ 1 000 dependent trips to HBM instead of ≈ 200.
  auto agree_at = [&](uint64_t tt, uint32_t nlv) -> bool {
    uint32_t l0 = 0, l1 = 0, l2 = 0, l3 = 0, nlive = 0;   // (scalars, not an array filled at a run-time index: that would live in scratch memory)
    for (uint32_t l = 0; l < nlv; ++l) if (M[l] != 0xFFu) {
      if (nlive == 4) return false;
      if (nlive == 0) l0 = l1 = l2 = l3 = l; else if (nlive == 1) l1 = l; else if (nlive == 2) l2 = l; else l3 = l;
      ++nlive;
    }
    if (nlive == 0) return false;
    const uint32_t lv[1] = {l0};
    if (nlive > 1) {   // (one live leaf: nothing to compare)
      uint32_t cur[4] = {l0, l1, l2, l3};
      for (uint64_t u = tt; u-- > prev;) {
        const uint32_t* row = D.sl_back + (size_t)R[u - a] * Lm;
        const uint32_t e0 = row[cur[0]], e1 = row[cur[1]], e2 = row[cur[2]], e3 = row[cur[3]];
        if ((e0 >> 8) != (e1 >> 8) || (e0 >> 8) != (e2 >> 8) || (e0 >> 8) != (e3 >> 8)) return false;
        cur[0] = e0 & 0xFFu; cur[1] = e1 & 0xFFu; cur[2] = e2 & 0xFFu; cur[3] = e3 & 0xFFu;
      }
      if (!pend_done)
        for (uint32_t jj = 0; jj < K; ++jj) {
          const uint32_t* pr = D.sl_pend + ((size_t)i0 * K + jj) * Lm;
          if (pr[cur[0]] != pr[cur[1]] || pr[cur[0]] != pr[cur[2]] || pr[cur[0]] != pr[cur[3]]) return false;
        }
    }
    const uint32_t la = back_to(prev, tt, lv[0]);
    if (!pend_done) { for (uint32_t jj = 0; jj < K; ++jj) E[nd + jj] = D.sl_pend[((size_t)i0 * K + jj) * Lm + la]; pend_done = true; }
    return true;
  };
  uint64_t e_out = 0; int mode = 0;   // 1 the table takes over at e_out, 2 the part is handed over at `end`, 3 the input ends
  for (;;) {
    if (((t - a) & 63u) == 0) qb[(t - a) >> 6] = (uint16_t)q;
    if (t >= hard) {
      if (t != n) return 3;        // (no room: the caller may try once more with DF_HOLE_MAX steps)
      if (!is_last) return 1;
      if (D.sl_fin_leaf[q] == 0xFFu) { atomicMin(&flags->fail_pos, (unsigned long long)n); return 2; }   // (end of input in a state that is not final)
      const uint32_t fl = D.sl_fin_leaf[q];
      const uint32_t la = back_to(anchor, n, fl);   // (the steps since the anchor, from the final leaf; la = M[fl])
      anchor_known(la);
      if (last) { mode = 3; e_out = n; } else { mode = 2; e_out = end; }   // (a lane that is not the input's last hands its part over as ever)
      break;
    }
    // (one dependent global load per step: the fused transition {next state | leaves << 16, row}; the step's row entries are requested
    //  with it and only the map waits for them; the input arrives 8 bytes at a time)
    if ((t & 7u) == 0 || t == a) {
      const uint64_t a8 = t & ~7ull;
      if (a8 + 8 <= n) { const uint2 w8 = *reinterpret_cast<const uint2*>(in + a8); inw = (uint64_t)w8.x | ((uint64_t)w8.y << 32); }
      else { inw = 0; for (uint64_t i = a8; i < n; ++i) inw |= (uint64_t)in[i] << (8 * (i - a8)); }
    }
    const uint32_t c = (uint32_t)io.lds[(uint32_t)(inw >> (8 * (t & 7u))) & 0xFFu] >> io.clsh;   // (the class table of the delayed form's image, in LDS)
    // ONE memory round trip per step: the transition and the parent leaf of every leaf of its target arrive together (the kernel is
    // streaming the input at 4.5 TB/s beside this walk: nothing of these tables stays in L2, every dependent load is a trip to HBM
    // — with the row's entries fetched one batch after the other a stretch of 256 steps took 3 ms)
    const uint4* fm = D.sl_fmap + ((size_t)q * C + c) * 3;
    const uint4 f0 = fm[0], f1 = fm[1], f2v = fm[2];
    const uint32_t nq = f0.x & 0xFFFFu;
    if (nq == 0xFFFFu) { atomicMin(&flags->fail_pos, (unsigned long long)t); return 2; }
    const uint32_t r = f0.y;
    R[t - a] = r;
    const uint32_t nnl = f0.x >> 16;
    uint32_t v = 0xFFu; bool same = true;
    const uint32_t par[8] = {f1.x, f1.y, f1.z, f1.w, f2v.x, f2v.y, f2v.z, f2v.w};
#pragma unroll
    for (uint32_t l = 0; l < DF_SL_LEAVES; ++l) {
      const uint32_t pl = (par[l >> 2] >> (8 * (l & 3u))) & 0xFFu;
      const uint32_t x = l >= nnl || pl == 0xFFu ? 0xFFu : M[pl];
      if (l < nnl) M2[l] = (uint8_t)x;
      if (x != 0xFFu) { if (v == 0xFFu) v = x; else same = same && x == v; }
    }
    { uint8_t* tmp = M; M = M2; M2 = tmp; }
    q = nq; nl = nnl; ++t;
    if ((!same || v == 0xFFu) && ((t - a) & 63u) == 0 && t + PIECE <= end && D.start_of_state[q] != 0xFFFFu && agree_at(t, nl)) {
      qb[(t - a) >> 6] = (uint16_t)q;
      mode = 1; e_out = t;
      break;
    }
    if (!same || v == 0xFFu) continue;
    anchor_known(v);
    const uint64_t decided = anchor;   // every step before it is decided, and the leaf there is known
    prev = anchor; anchor = t;
    for (uint32_t l = 0; l < DF_SL_LEAVES; ++l) M[l] = (uint8_t)l;
    const uint64_t e = decided & ~63ull;
    if (e > a && e + PIECE <= end && D.start_of_state[qb[(e - a) >> 6]] != 0xFFFFu) { mode = 1; e_out = e; break; }
    if (!last && decided + K >= end) { mode = 2; e_out = end; break; }
  }
  (void)nl;
  uint32_t h_next = h0;
  if (mode == 1) h_next = D.start_of_state[qb[(e_out - a) >> 6]];
  if (mode == 3) {
    // (the shard ends here: its end state has nothing pending and nothing due — the host's tail adds nothing)
    if (D.start_of_state[q] == 0xFFFFu) return 1;
    h_next = D.start_of_state[q];
  }
  if (mode == 2) {
    // the steps end - K .. end - 1 are written by the next lane's first K symbols; and of the constants before them, the ones
    // that lane's state at `end` still has due are written there too: they are the LAST constants of this stretch
    for (uint64_t u = end - K; u < end; ++u) if (u >= a) R[u - a] = NONE; else E[nd + K - (a - u)] = NONE;
    const uint32_t ix = (io.h_behind - 256u) / (C * 8u);
    uint32_t due = D.sl_defoff[ix + 1] - D.sl_defoff[ix];
    for (uint32_t idx = nd + K + (uint32_t)(end - K - a); due && idx-- > 0;) {
      const uint32_t pc = (E[idx] >> 1) & 0x3FFFFFFFu;
      if (pc < D.sl_npc && D.sl_pcoff[pc + 1] > D.sl_pcoff[pc]) { E[idx] = (E[idx] & 0x80000001u) | NONE; --due; }
    }
    if (due) return 1;
  }
  io.base = base; io.nd = nd; io.h_next = h_next; io.e_out = e_out;
  return 0;
}

// Piece records are staged per lane, DF_STAGE of them, and leave as whole 128-byte lines.  BT lanes per block, MINW waves per SIMD.
// What bounds this kernel is the memory side of its access pattern (every lane streams its own segment), as it bounds k_forward:
// blocks of 256 lanes with 4 staged records at 5 / 6 waves per SIMD 3.55 -> 4.31 / 8.20 ms (35 / 97 spilled registers); the lines of
// the next step touched ahead by one more dword load per line 3.40 -> 4.06 ms (profiles/r05_experiments.md §6)
// SLOW: the instance that carries the exact slow path.  Its call and its stack cost the trips a few registers (3.03 -> 3.15 ms on a log
// without a single undecided context): a stage runs the plain instance until a shard meets such a context, redoes that shard's forward
// pass on this one and stays on it (Stage::df_slow_armed).
template <int BT, uint32_t DF_STAGE, int MINW, bool SLOW>
__global__ __launch_bounds__(BT, MINW) void k_dforward(const uint8_t* __restrict__ in, uint64_t n, uint64_t seg, uint32_t nseg, int first_known,
                           const uint64_t* __restrict__ seg_pos, const uint16_t* __restrict__ seg_state,
                           DfRec* __restrict__ rec, uint32_t* __restrict__ wbase, uint32_t* __restrict__ own, uint32_t* __restrict__ spill, Flags* flags,
                           uint32_t* __restrict__ side, uint32_t side_cap, int is_last, DfDev D) {
  static_assert(DF_STAGE == 8 || DF_STAGE == 16, "a group of staged records is one or half a 128-byte line, and at least the slow path's 64-byte map");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  DfLds L = df_stage(D, smem);
  // per-lane staging of DF_STAGE piece records: they leave as whole lines (scattered 8-byte stores of lanes that are a
  // segment apart are read-modify-writes in L2)
  uint2* lrec = reinterpret_cast<uint2*>(smem + ((D.words + 3) & ~3u)) + (size_t)threadIdx.x * DF_STAGE;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t B = k < nseg ? df_own_start(k, n, seg, first_known, seg_pos, seg_state, D) : UNSYNC;
  bool alive = B != UNSYNC;   // (a lane without a part of its own still helps loading: the trips are wave-uniform)
  const uint32_t dead = D.deadh, esc = D.esch;
  // A lane's warm-up: from its synchronisation point in (state, nothing pending, nothing due) to its own start (what these steps write
  // belongs to the lane before; the bytes arrive 8 at a time — a load per byte would put ~100 dependent memory round trips in front of
  // every lane's first piece).  A warm-up that runs into a symbol without a transition or into an undecided context makes no part:
  // the lane before runs through and meets the same bytes with its own state (and reports, or resolves, what it finds) — which is
  // why every lane also walks the warm-up of the lane BEHIND it: both must agree on where the part ends (round 6; before, an
  // undecided context inside a warm-up sent the shard to the general engine).
  auto warm = [&](uint32_t jj, uint64_t Bj) -> uint32_t {
    if (jj == 0 && first_known) return D.starth;
    uint32_t hw = D.start_of_state[(((uint32_t)seg_state[jj] << D.hshift) - OFF_FWD) / D.orig_c4];
    for (uint64_t pw = seg_pos[jj]; pw < Bj;) {
      const uint2 v = *reinterpret_cast<const uint2*>(in + (pw & ~7ull));
      const uint64_t x = (uint64_t)v.x | ((uint64_t)v.y << 32);
      for (uint32_t b = (uint32_t)pw & 7u; b < 8u && pw < Bj; ++b, ++pw) hw = L.ent(hw + L.c8((uint32_t)(x >> (8 * b)) & 0xFFu)).x & 0xFFFFu;
    }
    if (hw == esc && jj == k) atomicAdd(&flags->warm_esc, 1u);
    return hw == esc || hw == dead ? 0xFFFFFFFFu : hw;
  };
  uint32_t h = dead, h_behind = 0;   // h_behind: the state the lane behind starts its own part in (the slow path's hand-over needs what it has due)
  if (alive) { h = warm(k, B); if (h == 0xFFFFFFFFu) { alive = false; h = dead; } }
  uint32_t j = k + 1;
  uint64_t end = n;
  if (alive) for (; j < nseg; ++j) {
    const uint64_t b = df_own_start(j, n, seg, first_known, seg_pos, seg_state, D);
    if (b == UNSYNC) continue;
    h_behind = warm(j, b);
    if (h_behind != 0xFFFFFFFFu) { end = b; break; }
  }
  const bool last = alive && j >= nseg;
  uint64_t pos = alive ? B : 0;
  if (alive) atomicMin(&flags->df_first_own, (unsigned long long)B);
  bool failed = !alive;
  if (!alive) { end = 0; pos = 0; }
  uint32_t m = (uint32_t)(pos / seg), cum = 0, flag = DFREC_OWN;
  uint64_t block_end = ((uint64_t)m + 1) * seg;
  // the run died or escaped inside the piece at p0: which symbol?  1: a symbol without a transition (reported), 2: an undecided context
  auto fail_in = [&](uint32_t h0, uint64_t p0, uint32_t plen) -> int {
    uint32_t hh = h0;
    for (uint32_t t = 0; t < plen; ++t) {
      const uint32_t nh = L.ent(hh + L.c8(in[p0 + t])).x & 0xFFFFu;
      if (nh == dead) { atomicMin(&flags->fail_pos, (unsigned long long)(p0 + t)); failed = true; return 1; }
      if (nh == esc) return 2;
      hh = nh;
    }
    failed = true;
    return 1;
  };
  // records are staged in the slot (piece & (DF_STAGE - 1)) and leave when their group of DF_STAGE is complete (or the lane's part ends)
  uint32_t nst = 0; uint64_t gfirst = 0;
  auto flush_group = [&]() {
    // (as one 8-byte vector store each: stored field by field through the record type, this loop cost the ARMED instance's trips 38
    //  scratch operations per step — 114 spilled registers instead of 70, its forward pass 4.2 -> 5.4 ms on a log with escaped quotes)
    uint2* dst = reinterpret_cast<uint2*>(rec + gfirst);
    for (uint32_t i = 0; i < nst; ++i) dst[i] = lrec[(gfirst + i) & (DF_STAGE - 1)];
    nst = 0;
  };
  const bool coop = !(D.debug & 256u);   // (kx_config::debug_flags & 256: every lane flushes its own records — the A/B of profiles/r06_experiments.md)
  bool in_trip = false;   // inside a trip the complete groups leave together, cooperatively (coop_flush); elsewhere a lane flushes its own
  auto stage_rec = [&](uint64_t pc, DfRec r) {
    if (nst == 0) gfirst = pc;
    if ((pc & (DF_WBASE_PIECES - 1)) == 0) wbase[pc / DF_WBASE_PIECES] = cum | flag;   // (cum: still without this piece)
    lrec[pc & (DF_STAGE - 1)] = make_uint2(r.x, r.y); ++nst;
    if (!in_trip && (pc & (DF_STAGE - 1)) == DF_STAGE - 1) flush_group();
  };
  // a trip of eight pieces may start where the staged group is an aligned one: it then completes at the end of a trip (of every second
  // trip with 16 staged records: the group survives the trip boundary in between) and leaves cooperatively
  auto group_aligned = [&]() { return ((uint32_t)(pos >> 6) & (DF_STAGE - 1)) == nst; };
  // Round 6: the complete record groups of a wave leave as WHOLE LINES written by adjacent lanes (teams of eight lanes; step i: the team
  // writes the group of its lane i, every lane DF_STAGE / 8 records of it — with 16 staged records 16 bytes per lane, one 128-byte line
  // per team and instruction; with 8, half a line), instead of DF_STAGE 8-byte stores per lane that each touch 64 different lines:
  // a sixteenth of the write requests, and half of what the 16-byte records took per piece (the groups' positions travel by two
  // shuffles per step).  Only lanes whose group is complete take part as sources (a lane that died in mid-trip keeps its partial
  // group for its own flush).
  uint2* const lrec_wave = reinterpret_cast<uint2*>(smem + ((D.words + 3) & ~3u)) + (size_t)(threadIdx.x & ~63u) * DF_STAGE;
  auto coop_flush = [&]() {
    const bool full = nst == DF_STAGE && (gfirst & (DF_STAGE - 1)) == 0;
    if (!__any(full)) return;
    const uint32_t glo = (uint32_t)gfirst, ghi = (uint32_t)(gfirst >> 32) | (full ? 0u : 0x80000000u);
    constexpr uint32_t RPL = DF_STAGE / 8;   // records per lane and store
    const uint32_t team = lane & ~7u, r = (lane & 7u) * RPL;
    static_for<0, 8>([&](auto ic) {
      constexpr uint32_t i = decltype(ic)::value;
      const uint32_t slo = (uint32_t)__shfl((int)glo, (int)(team + i)), shi = (uint32_t)__shfl((int)ghi, (int)(team + i));
      if (!(shi & 0x80000000u)) {
        const uint64_t g = ((uint64_t)shi << 32) | slo;
        const uint2* src = lrec_wave + (size_t)(team + i) * DF_STAGE + r;
        if constexpr (RPL == 2) *reinterpret_cast<uint4*>(rec + g + r) = *reinterpret_cast<const uint4*>(src);
        else *reinterpret_cast<uint2*>(rec + g + r) = *src;
      }
    });
    if (full) nst = 0;
  };
  auto cross = [&]() { if (pos == block_end) { (flag ? own : spill)[m] = cum; cum = 0; flag = 0; ++m; block_end += seg; } };
  uint32_t kc_sum = 0, kc_max = 0, kc_n = 0;   // constants per piece: what k_demit's planner dimensions the job slots by
  // ---- THE EXACT SLOW PATH (round 6).  The piece at `a` holds a context that K symbols do not decide (a backslash before a quote in
  // apache_log's quoted fields).  Round 5 gave the whole shard to the general engine for it; here the lane resolves the stretch itself,
  // on the path form: it walks on from the piece's start (product state h0: SST state, K pending steps, constants due), composing the
  // parent maps of the steps since the last ANCHOR; when every live leaf of the current state descends from ONE leaf at the anchor,
  // that leaf is known — the pending steps (first anchor = a) or the steps between the previous anchor and this one (walked BACKWARD
  // over their recorded rows) are decided, and the current position becomes the next anchor: every step is walked once forward and
  // once backward.  It stops at the first piece boundary e behind a decided anchor that leaves the table K + J symbols before the
  // lane's part ends — the table takes over there in (state, nothing pending, nothing due) — or hands its part over at its end:
  // everything up to the steps the next lane's first K symbols write, minus the constants that lane's state still has due — or, on
  // the input's last lane, runs to the end of the input, where the final state's leaf decides.  What the steps write goes to the SIDE
  // ENTRIES, the pieces' records name them (DFREC_HOLE), k_demit's lanes replay them.  Returns 0 resolved, 1 not resolvable here
  // (more than 16 leaves, a stretch beyond DF_HOLE_MAX steps, the end of a shard that is not the last, no room): the shard falls
  // back as before; 2 the input fails inside (reported).
  auto slow = [&](const uint64_t a, const uint32_t h0) -> int {
    // (most stretches end within a few hundred steps — the rest of a log line: room for DF_HOLE_FIRST first, for DF_HOLE_MAX if that was short)
    flush_group();   // (the lane's staged records leave first: they precede the stretch's in the record array, and their LDS slot is the slow path's map)
    DfSlowIO io{in, n, a, end, h0, last ? 1u : 0u, (uint32_t)is_last, h_behind, side, side_cap, flags, L.base, D.wide ? 0u : 3u, reinterpret_cast<uint8_t*>(lrec), DF_HOLE_FIRST, 0, 0, 0, 0};
    {
      int rc = df_slow_resolve(io, D);
      if (rc == 3) { io.max_steps = DF_HOLE_MAX; rc = df_slow_resolve(io, D); }
      if (rc) return rc == 3 ? 1 : rc;
    }
    const uint32_t base = io.base, nd = io.nd, K = D.K;
    const uint64_t e_out = io.e_out;
    const uint32_t* const E = side + base;
    // the pieces' records: lengths from the entries
    const uint64_t pend = (e_out + 63) & ~63ull;
    uint32_t idx = 0;
    for (uint64_t pp = a; pp < pend; pp += PIECE) {
      cross();
      const bool first = pp == a;
      const uint32_t steps = (uint32_t)((e_out - pp) < PIECE ? e_out - pp : PIECE);
      const uint32_t cnt = first ? nd + K + steps : steps;
      uint32_t len = 0;
      for (uint32_t x = 0; x < cnt; ++x) {
        const uint32_t ee = E[idx + x], pc = (ee >> 1) & 0x3FFFFFFFu;
        len += (ee & 1u) + (pc < D.sl_npc ? D.sl_pcoff[pc + 1] - D.sl_pcoff[pc] : 0u);
      }
      if (len > DF_HOLE_LEN_MAX || cnt > DF_HOLE_CNT_MAX) return 1;
      if (((pp >> 6) & (DF_WBASE_PIECES - 1)) == 0) wbase[(pp >> 6) / DF_WBASE_PIECES] = cum | flag;
      rec[pp >> 6] = dfrec_pack_hole(base + idx, cnt, first, len);
      idx += cnt; cum += len; pos = pp + steps;
    }
    h = io.h_next;
    atomicAdd(&flags->slow_steps, (uint32_t)(e_out - a));
    return 0;
  };
  // one whole piece from registers; false: the run ended in it
  bool need_slow = false;   // the piece at `pos` (entered in state h) holds an undecided context
  auto run_slow = [&]() {
    need_slow = false;
    int r = 1;
    if constexpr (SLOW) r = slow(pos, h);
    if (r) { if (r == 1) atomicAdd(&flags->df_esc, 1u); failed = true; }
  };
  auto do_piece = [&](const uint32_t (&w)[16]) -> bool {
    cross();   // (a block may be as short as one piece)
    const uint32_t h0 = h;
    uint32_t mid, sumA, sum = 0;
    if (D.wide) piece_dfrun1w(w, h, mid, sumA, sum); else piece_dfrun1(w, h, mid, sumA, sum);   // sums: bytes appended << 8 | 4 x constants (of the first half; of the second half + bytes of both)
    if (h == dead || h == esc) {
      // (an undecided context: the slow path runs OUTSIDE the trip — behind it, from the outer loop — so that its call and what lives
      //  across it cost the trips' code no registers: the lane sits out the rest of its trip)
      if (fail_in(h0, pos, PIECE) == 2) { need_slow = true; h = h0; }
      return false;
    }
    const uint32_t kA = (sumA & 0xFFu) >> 2, kB = (sum & 0xFFu) >> 2;
    kc_sum += kA + kB; kc_max = kA + kB > kc_max ? kA + kB : kc_max; ++kc_n;
    stage_rec(pos >> 6, dfrec_pack(h0, mid, sumA >> 8, sum >> 8, kA, kB));
    cum += sum >> 8; pos += PIECE;
    return true;
  };
  auto single_piece = [&]() {
    uint32_t w[16];
    load_piece(in, n, pos, w);
    do_piece(w);
  };
  for (;;) {   // (a lane that left a trip for the slow path stands on a piece boundary that is no trip boundary: resolve, align, go again)
  if (need_slow) run_slow();
  while (!failed && !need_slow && pos + PIECE <= end && ((pos & (8 * PIECE - 1)) || !group_aligned())) single_piece();   // up to the next 512-byte boundary with an aligned group
  // trips of eight pieces with cooperative loads (k_forward's scheme): every 8 lanes fetch one 128-byte line of one lane's
  // segment per instruction, an 8 x 8 register transpose hands each lane its own line
  for (;;) {
    const bool can = !failed && !need_slow && pos + 8 * PIECE <= end && !(pos & (8 * PIECE - 1)) && group_aligned();
    // (a lane that waits for the slow path leaves the trips with its whole wave: it would otherwise sit out every remaining trip of
    //  the others and then run its own alone — twice the wave's time for one undecided context, measured)
    if (!__any(can) || __any(need_slow)) break;
    uint32_t line[8];
    {
      const uint32_t mine = can ? (uint32_t)(pos >> 7) : 0xFFFFFFFFu;
      static_for<0, 8>([&](auto ic) { constexpr int i = decltype(ic)::value; line[i] = __shfl(mine, (int)((lane & ~7u) + i)); });
    }
    // the lines of step k2 + 1 are requested between the two pieces of step k2: the second piece's 64 dependent steps hide their way
    // from HBM (unconditional loads: a lane without a trip reads line 0, which exists — some lane of the wave has 512 bytes left)
    auto issue = [&](uint32_t k2, uint4 (&dst)[8]) {
      static_for<0, 8>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const uint64_t ln = line[i] != 0xFFFFFFFFu ? line[i] : 0u;
        dst[i] = *reinterpret_cast<const uint4*>(in + ((ln + k2) << 7) + (lane & 7u) * 16);
      });
    };
    uint4 v[8];
    issue(0, v);
    bool died = false;
    in_trip = coop;
#pragma nounroll
    for (uint32_t k2 = 0; k2 < 4; ++k2) {
      transpose8(v, lane);
      uint32_t wa[16], wb[16];
      static_for<0, 8>([&](auto ic) {
        constexpr int w = decltype(ic)::value;
        uint32_t (&dst)[16] = w < 4 ? wa : wb;
        dst[4 * (w & 3)] = v[w].x; dst[4 * (w & 3) + 1] = v[w].y; dst[4 * (w & 3) + 2] = v[w].z; dst[4 * (w & 3) + 3] = v[w].w;
      });
      bool go = can && !died;
      if (go && !do_piece(wa)) { died = true; go = false; }
      if (k2 < 3) issue(k2 + 1, v);
      if (go && !do_piece(wb)) died = true;
    }
    if (coop) coop_flush();   // (wave-uniform; the lanes whose group of 8 or 16 is complete: with 16, the lanes in the second trip of their group)
    in_trip = false;
  }
  if (!__any(!failed && (need_slow || pos + 8 * PIECE <= end))) break;
  }
  if (!alive) return;
  for (;;) {
  if (need_slow) run_slow();
  while (!failed && !need_slow && pos + PIECE <= end) single_piece();
  if (need_slow) continue;
  if (!failed && pos < end) {   // the input's last, partial piece
    cross();
    const uint32_t plen = (uint32_t)(end - pos), h0 = h;
    uint32_t mid = h, lenA = 0, len = 0, kA = 0, kc = 0;
    for (uint32_t t = 0; t < plen; ++t) {
      if (t == HALF) { mid = h; lenA = len; kA = kc; }
      const uint2 e = L.ent(h + L.c8(in[pos + t]));
      h = e.x & 0xFFFFu; len += e.y >> 24; kc += (e.y >> 23) & 1u;
    }
    if (plen <= HALF) { mid = h; lenA = len; kA = kc; }
    if (h == dead || h == esc) {
      if (fail_in(h0, pos, plen) == 2) { h = h0; need_slow = true; continue; }
    }
    else { stage_rec(pos >> 6, dfrec_pack(h0, mid, lenA, len, kA, kc - kA)); cum += len; pos = end; }
  }
  break;
  }
  flush_group();
  if (failed) return;
  (flag ? own : spill)[m] = cum;
  if (last) flags->end_state = h;
  if (kc_n) { if ((k & 15u) == 0) { atomicAdd(&flags->emit_ksum, kc_sum); atomicAdd(&flags->emit_kn, kc_n); } atomicMax(&flags->emit_kmax, kc_max); }
}

// sharded runs: the bytes before the first lane's own part, from the state the previous shard ends in (one lane)
__global__ void k_dhead(const uint8_t* __restrict__ in, uint64_t n, uint64_t seg, uint64_t head_len, uint32_t h,
                        DfRec* __restrict__ rec, uint32_t* __restrict__ wbase, uint32_t* __restrict__ own, uint32_t* __restrict__ spill, Flags* flags, DfDev D) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  DfLds L = df_stage(D, smem);
  if (blockIdx.x || threadIdx.x) return;
  const uint32_t dead = D.deadh, esc = D.esch;
  uint32_t m = 0, cum = 0;
  uint64_t block_end = seg;
  for (uint64_t pos = 0; pos < head_len;) {
    if (pos == block_end) { spill[m] = cum; cum = 0; ++m; block_end += seg; }
    const uint32_t plen = (uint32_t)(head_len - pos < PIECE ? head_len - pos : PIECE);
    const uint32_t h0 = h;
    uint32_t mid = h, lenA = 0, len = 0, kA = 0, kc = 0;
    for (uint32_t t = 0; t < plen; ++t) {
      if (t == HALF) { mid = h; lenA = len; kA = kc; }
      const uint2 e = L.ent(h + L.c8(in[pos + t]));
      const uint32_t nh = e.x & 0xFFFFu;
      if (nh == dead) { atomicMin(&flags->fail_pos, (unsigned long long)(pos + t)); return; }
      if (nh == esc) { flags->df_esc = 1; return; }
      h = nh; len += e.y >> 24; kc += (e.y >> 23) & 1u;
    }
    if (plen <= HALF) { mid = h; lenA = len; kA = kc; }
    if (kc > 0) atomicMax(&flags->emit_kmax, kc);
    if (((pos >> 6) & (DF_WBASE_PIECES - 1)) == 0) wbase[(pos >> 6) / DF_WBASE_PIECES] = cum;   // (a spill part: no own flag)
    rec[pos >> 6] = dfrec_pack(h0, mid, lenA, len, kA, kc - kA);
    cum += len; pos += plen;
  }
  spill[m] = cum;
  if (head_len == n) flags->end_state = h;
}

__global__ void k_dlen(uint32_t nblk, const uint32_t* __restrict__ own, const uint32_t* __restrict__ spill, uint32_t* __restrict__ len,
                       unsigned long long* __restrict__ wsum) {
  __shared__ unsigned long long red[1024];
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t mylen = 0;
  if (m < nblk) { mylen = own[m] + spill[m]; len[m] = mylen; }
  red[threadIdx.x] = mylen;
  __syncthreads();
  for (uint32_t s = blockDim.x >> 1; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) wsum[blockIdx.x] = red[0];
}

// sharded runs: the shard's start leaf as a function of its end leaf, by composing the path form's parent maps FORWARD from
// the shard's first byte until the map is constant (one lane; the path form's tables staged in LDS as the general kernels have them,
// the input 8 bytes at a time: a few hundred steps of three dependent LDS reads on the BASELINE inputs).
// map[l] = leaf at position 0 that leaf l of the current state descends from.  status: 1 constant, 2 end of shard reached
// (map complete, not constant), 0 gave up (cap): the shard falls back to the general engine.
template <bool GENERAL>
__global__ void k_dmap(const uint8_t* __restrict__ in, uint64_t n, uint32_t q_in, uint64_t cap, uint8_t* __restrict__ map_out,
                       uint32_t* __restrict__ status, DevTables T) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Lds L = stage_tables<GENERAL>(T, smem);   // (the path form's tables from LDS: a step is three dependent reads)
  if (blockIdx.x || threadIdx.x) return;
  __shared__ uint8_t M[2][256];
  const uint32_t C = T.nclasses;
  uint32_t h = (OFF_FWD + q_in * C * 4) >> T.hshift, cur = 0;
  uint32_t nl = T.nleaves[q_in];
  for (uint32_t l = 0; l < nl; ++l) M[0][l] = (uint8_t)l;
  uint64_t pos = 0;
  bool constant = nl == 1, dead = false;
  while (pos < n && pos < cap && !constant && !dead) {
    const uint64_t a8 = pos & ~7ull;
    uint64_t x = 0;
    if (a8 + 8 <= n) { const uint2 v = *reinterpret_cast<const uint2*>(in + a8); x = (uint64_t)v.x | ((uint64_t)v.y << 32); }
    else for (uint64_t i = a8; i < n; ++i) x |= (uint64_t)in[i] << (8 * (i - a8));   // (the shard's last bytes: nothing is read behind them)
    for (uint32_t b = (uint32_t)pos & 7u; b < 8u && pos < n && pos < cap && !constant; ++b, ++pos) {
      const uint32_t e = L.next(h, (uint32_t)(x >> (8 * b)) & 0xFFu);
      const uint32_t nh = e & 0xFFFFu;
      if (nh == T.deadh) { dead = true; break; }
      const uint32_t row = L.ra(e >> 16);
      const uint32_t nq = ((nh << T.hshift) - OFF_FWD) / (C * 4);
      const uint32_t nnl = T.nleaves[nq];
      constant = true;
      for (uint32_t l = 0; l < nnl; ++l) {
        const uint32_t p = (L.w(row + l * 4) >> 2) & 0xFFu;
        M[cur ^ 1][l] = M[cur][p < nl ? p : 0];
        constant = constant && M[cur ^ 1][l] == M[cur ^ 1][0];
      }
      cur ^= 1; h = nh; nl = nnl;
    }
  }
  for (uint32_t l = 0; l < 256; ++l) map_out[l] = constant ? M[cur][0] : l < nl ? M[cur][l] : 0;
  *status = constant ? 1u : pos >= n ? 2u : 0u;
}

// the byte a step copies: input byte S of the piece, or (S < 0) one of the last bytes of the piece before it
template <int S>
__device__ __forceinline__ uint32_t df_byte_src(const uint32_t (&w)[16], uint32_t wp) {
  if constexpr (S >= 0) return w[S >> 2] >> ((S & 3) * 8);
  else return wp >> ((4 + S) * 8);
}

// bytes 0..min(r,3)-1 of v to LDS address d, d+1, d+2 and dwords 0..min(m,4)-1 of w to the 4-byte-aligned LDS address d, d+4, …: straight
// sequences in which v_cmpx narrows the lanes still to be served (put_bytes16's scheme)
__device__ __forceinline__ void put_bytes3(uint32_t r, uint32_t d, uint32_t v) {
  uint32_t t; unsigned long long sv;
  asm volatile("s_mov_b64 %[sv], exec\n"
               "v_cmpx_lt_u32_e32 vcc, 0, %[r]\n"
               "ds_write_b8 %[d], %[v]\n"
               "v_cmpx_lt_u32_e32 vcc, 1, %[r]\n"
               "v_lshrrev_b32 %[t], 8, %[v]\n"
               "ds_write_b8 %[d], %[t] offset:1\n"
               "v_cmpx_lt_u32_e32 vcc, 2, %[r]\n"
               "ds_write_b8_d16_hi %[d], %[v] offset:2\n"
               "s_mov_b64 exec, %[sv]\n"
               : [t] "=&v"(t), [sv] "=&s"(sv) : [r] "v"(r), [d] "v"(d), [v] "v"(v) : "vcc", "memory");
}
__device__ __forceinline__ void put_dwords4(uint32_t m, uint32_t d, const uint32_t (&w)[4]) {
  unsigned long long sv;
  asm volatile("s_mov_b64 %[sv], exec\n"
               "v_cmpx_lt_u32_e32 vcc, 0, %[m]\n"
               "ds_write_b32 %[d], %[w0]\n"
               "v_cmpx_lt_u32_e32 vcc, 1, %[m]\n"
               "ds_write_b32 %[d], %[w1] offset:4\n"
               "v_cmpx_lt_u32_e32 vcc, 2, %[m]\n"
               "ds_write_b32 %[d], %[w2] offset:8\n"
               "v_cmpx_lt_u32_e32 vcc, 3, %[m]\n"
               "ds_write_b32 %[d], %[w3] offset:12\n"
               "s_mov_b64 exec, %[sv]\n"
               : [sv] "=&s"(sv) : [m] "v"(m), [d] "v"(d), [w0] "v"(w[0]), [w1] "v"(w[1]), [w2] "v"(w[2]), [w3] "v"(w[3]) : "vcc", "memory");
}

// Issue priorities of a k_demit wave's phases (the walk itself runs at 3, set inside its sequence; everything else at 0): a wave that
// has walked should finish — its constants and its flush are short dependent chains that, at priority 0, wait for the issue slots the
// walking waves of the SIMD leave over (profiles/r05_experiments.md §11)
#ifndef KX_PRIO_CONSTANTS
#define KX_PRIO_CONSTANTS 2
#endif
#ifndef KX_PRIO_FLUSH
#define KX_PRIO_FLUSH 1
#endif
constexpr int HALF_BYTES = HALF;   // (k_demit's template parameter HALF shadows the engine's constant)

// one step of the fused walk in plain C++ (general path of k_demit: oversize pieces, the input's partial last piece, a round
// whose constants overflowed the job slots): CONSTS 0 = to global memory (o is a global offset), 1 = into staging with the
// constants copied in place
template <int CONSTS>
__device__ __forceinline__ void df_step_gen(uint32_t& h, uint32_t byte_now, uint32_t byte_out, uint64_t& o, uint8_t* __restrict__ dst,
                                            const DfLds& L, const DfDev& D) {
  const uint2 e = L.ent(h + L.c8(byte_now));
  h = e.x & 0xFFFFu;
  const uint32_t cp = E_COPY(e.y), dl = e.y >> 24;
  if (cp) dst[o] = (uint8_t)byte_out;
  if (dl > cp) { const uint32_t src = D.off_pool + (E_AID(e.y) << 4); for (uint32_t i = 0; i < dl - cp; ++i) dst[o + cp + i] = L.base[src + i]; }
  o += dl;
}

// HALF: a lane owns HALF a piece (32 input bytes, one chain): for programs whose pieces are too large for 64 of them to share a wave's
// staging area — instead of several rounds per wave-iteration, each running the whole walk for a part of the lanes, one walk with every
// lane at work over half the input (iso_datetime_to_json: 265 output bytes per piece, three rounds of 22 lanes before)
template <int WAVES, int K, bool HALF = false>
__global__ __launch_bounds__(WAVES * 64) void k_demit(const uint8_t* __restrict__ in, uint64_t n, uint64_t blk, uint64_t blk_inv,
                                                      uint64_t npieces_total, const DfRec* __restrict__ rec, const uint32_t* __restrict__ wbase,
                                                      const uint32_t* __restrict__ spill, const unsigned long long* __restrict__ off,
                                                      Flags* __restrict__ flags, uint32_t stgb, uint32_t jbytes, uint32_t maxcnt,
                                                      uint8_t* __restrict__ out, const uint32_t* __restrict__ side, DfDev D) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  DfLds L = df_stage(D, smem);
  if ((uint32_t)(uintptr_t)smem != 0u) __builtin_trap();   // the walk addresses LDS absolutely
  constexpr int NB = HALF ? HALF_BYTES : PIECE, NW = NB / 4;   // input bytes / dwords per lane
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t stga = ((D.words + 3) & ~3u) * 4 + wave * (stgb + 16 + jbytes);
  uint8_t* stg = (uint8_t*)smem + stga;
  const uint32_t jarea = stga + stgb + 16;
  const uint64_t nunits = HALF ? npieces_total * 2 : npieces_total;   // lanes' units: pieces, or half pieces
  const uint64_t nwi = (nunits + 63) / 64;
  const uint64_t oend_all = flags->total_len;
  const uint64_t one_piece_blocks = (uint64_t)__builtin_amdgcn_readfirstlane(blk == (uint64_t)PIECE ? 1 : 0);
  // everything a unit needs is requested ONE ITERATION AHEAD (the walk needs the output offset at its first step)
  // (the unit's own: its input words, the four bytes before them and its record; the wave's: where the output of the iteration's first
  //  unit starts — base word, block offset and spill length of that unit's block, one address each for the whole wave)
  struct Operands { uint32_t w[NW]; uint32_t wp; uint2 r; uint32_t wb; uint64_t off0; uint32_t sp0; };
  auto request = [&](uint64_t it_, Operands& o) {
    if (it_ >= nwi) return;
    {
      const uint64_t itu = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(it_ >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)it_);
      const uint64_t pf = itu * (HALF ? 32u : 64u);   // the iteration's first piece (it exists: it_ < nwi)
      const uint64_t mf = __umul64hi(pf, blk_inv) + pf * one_piece_blocks;
      // (the indices go through a vector register on purpose: from scalar ones these would be SCALAR loads, which share their counter
      //  with the LDS operations — the walk's first wait for an LDS read would then wait for these trips to memory as well)
      uint32_t vw, vm;
      asm("v_mov_b32 %0, %1" : "=v"(vw) : "s"((uint32_t)(pf / DF_WBASE_PIECES)));
      asm("v_mov_b32 %0, %1" : "=v"(vm) : "s"((uint32_t)mf));
      o.wb = wbase[vw]; o.off0 = off[vm]; o.sp0 = spill[vm];
    }
    const uint64_t u = it_ * 64 + lane;
    const bool ok = u < nunits;
    const uint64_t pc = HALF ? u >> 1 : u;
    const uint64_t ustart = ok ? (HALF ? pc * PIECE + (u & 1) * HALF_BYTES : pc * PIECE) : n;
    if constexpr (HALF) {
      if (ustart + HALF_BYTES <= n) {
        const uint4* p = reinterpret_cast<const uint4*>(in + ustart);
        const uint4 v0 = p[0], v1 = p[1];
        o.w[0] = v0.x; o.w[1] = v0.y; o.w[2] = v0.z; o.w[3] = v0.w; o.w[4] = v1.x; o.w[5] = v1.y; o.w[6] = v1.z; o.w[7] = v1.w;
      } else {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
          uint32_t x = 0;
#pragma unroll
          for (int bb = 0; bb < 4; ++bb) { const uint64_t a = ustart + 4 * i + bb; if (a < n) x |= (uint32_t)in[a] << (8 * bb); }
          o.w[i] = x;
        }
      }
    } else load_piece(in, n, ustart, o.w);
    // the four bytes before the unit (the copied bytes of its first K steps); the first unit's pending steps copy nothing, so it may
    // read anything.  Like the record's, an unconditional load from a clamped address that is always valid: a register that is written
    // both by a load under a branch and by a plain move makes the compiler wait, right here, for loads that are still in flight (it
    // cannot count the memory operations of the flush loop) — i.e. for this very prefetch
    o.wp = *reinterpret_cast<const uint32_t*>(ok && ustart >= 4 ? in + ustart - 4 : reinterpret_cast<const uint8_t*>(D.img));
    o.r = *reinterpret_cast<const uint2*>(rec + (ok ? pc : 0));
  };
  // `cur` = the operands of the iteration at work, `nx` = those of the next one, in flight since the top of this one.  `cur = nx` is
  // done BEFORE the iteration's flush: at that point the only memory operations in flight are the prefetch loads themselves, long
  // arrived; at the top of the next iteration the same wait would also cover the flush's stores, just issued (≈ a fifth of a wave's
  // time in the first version of this kernel: profiles/r05_experiments.md)
  Operands nx, cur;
  request((uint64_t)blockIdx.x * WAVES + wave, nx);
  cur = nx;
  // timeline of the phases (KX_DEBUG_FLAGS & 64; diagnostic: the stamps wait for everything in flight)
  unsigned long long tk[6] = {0, 0, 0, 0, 0, 0};
  auto stamp = [&]() -> unsigned long long {
    if (!(D.debug & 64u)) return 0ull;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    return __builtin_amdgcn_s_memtime();
  };
  for (uint64_t it = (uint64_t)blockIdx.x * WAVES + wave; it < nwi; it += (uint64_t)gridDim.x * WAVES) {
    const unsigned long long t0 = stamp();
    const uint64_t unit = it * 64 + lane;
    const bool valid = unit < nunits;
    const uint64_t piece = HALF ? unit >> 1 : unit;
    const uint32_t half = HALF ? (uint32_t)unit & 1u : 0u;
    const uint64_t ustart = piece * PIECE + half * HALF_BYTES;
    const int plen = valid ? (int)(n <= ustart ? 0 : n - ustart < (uint64_t)NB ? n - ustart : NB) : 0;   // the unit's input bytes
    uint32_t w[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = cur.w[i];
    const uint32_t wp = cur.wp;
    const DfRec rc{cur.r.x, cur.r.y};
    const bool hole = valid && dfrec_hole(rc);   // (a piece the forward pass resolved on the slow path: its lane replays the side entries)
    const uint32_t len = hole ? dfrec_hole_len(rc) : dfrec_len(rc), lenA = hole ? len : dfrec_lenA(rc);   // (a hole's first half-unit replays the whole piece)
    const uint32_t kA = HALF ? (half ? dfrec_kB(rc) : dfrec_kA(rc)) : dfrec_kA(rc), kB = HALF ? 0u : dfrec_kB(rc);
    const uint32_t hA = HALF ? (half ? dfrec_middle(rc) : dfrec_start(rc)) : dfrec_start(rc), hB = dfrec_middle(rc);
    // the output is contiguous: a unit's starts where the iteration's first unit's does (the wave's base) + what the units before it
    // in the wave write; it ends its own length behind
    const uint32_t ulen = valid ? (HALF ? (half ? len - lenA : lenA) : len) : 0u;
    const uint32_t before = wave_scan_incl(ulen) - ulen;
    const uint64_t obase = cur.off0 + (cur.wb & ~DFREC_OWN) + ((cur.wb & DFREC_OWN) ? cur.sp0 : 0u);
    const uint64_t ostart = valid ? obase + before : oend_all, oend = valid ? ostart + ulen : oend_all;
    const unsigned long long vmask = __ballot(valid);
    const uint32_t nvalid = (uint32_t)__popcll(vmask);
    uint32_t first = 0;
    bool taken = false;
    unsigned long long t2 = stamp();
    tk[0] += t2 - t0;
    // pieces the forward pass resolved on its slow path: what their steps write is in the side entries (entry = copy | constant << 1,
    // bit 31: no input byte); their lanes replay them straight into the output, all of an iteration's at once (a stretch is a run of
    // neighbouring pieces: one after the other they cost a wave a millisecond)
    if (hole && half == 0) {
      const uint32_t cntE = dfrec_hole_entries(rc), e0 = dfrec_hole_side(rc);
      uint64_t u = dfrec_hole_first(rc) ? piece * PIECE - K : piece * PIECE, o = ostart;   // (the first piece of a stretch also writes the K pending steps)
      for (uint32_t x = 0; x < cntE; ++x) {
        const uint32_t ee = side[e0 + x], pc = (ee >> 1) & 0x3FFFFFFFu;
        if (ee & 1u) out[o++] = in[u];
        if (pc < D.sl_npc) for (uint32_t b = D.sl_pcoff[pc]; b < D.sl_pcoff[pc + 1]; ++b) out[o++] = D.sl_pcpool[b];
        if (!(ee >> 31)) ++u;
      }
    }
    while (first < nvalid) {
      // the next iteration's operands are requested from INSIDE the round loop: a loop that holds stores, no loads, and a use of a
      // register loaded before it makes the compiler drain every memory operation in front of the loop (its "flush in the preheader"
      // rule) — which here would be this prefetch, just issued
      if (first == 0) request(it + (uint64_t)gridDim.x * WAVES, nx);
      const uint64_t gs = wave_read64(ostart, first);
      const uint64_t abase = gs & ~15ull;
      const bool fits = valid && lane >= first && (oend - abase) <= (uint64_t)stgb && plen == NB && !hole;
      const unsigned long long fm = __ballot(fits) >> first;
      uint32_t cnt = fm == ~0ull ? 64u - first : (uint32_t)__builtin_ctzll(~fm);
      if (cnt > maxcnt) cnt = maxcnt;
      if (cnt == 0) {
        // a unit larger than the staging area, or the input's partial last piece: its lane writes straight to global memory
        if (lane == first && hole) {
          // (replayed in front of the rounds, with every other such piece of the iteration)
        } else
        if (lane == first) {
          uint32_t h = hA;
          uint64_t o = ostart;
          for (int t = 0; t < plen; ++t) {
            const int ts = t - K;
            const uint32_t bn = (w[t >> 2] >> ((t & 3) * 8)) & 0xFFu;
            const uint32_t bo_ = ts >= 0 ? (w[ts >> 2] >> ((ts & 3) * 8)) & 0xFFu : (wp >> ((4 + ts) * 8)) & 0xFFu;
            df_step_gen<0>(h, bn, bo_, o, out, L, D);
          }
        }
        first += 1;
        continue;
      }
      const uint32_t lastl = first + cnt - 1;
      const bool active = lane >= first && lane <= lastl;
      const uint32_t o0 = stga + (uint32_t)(ostart - abase);   // LDS address of the piece's first output byte
      // job slots: the records say how many constants each half of a piece appends, so every lane owns its slots beforehand
      // (an exclusive prefix over the round's lanes); jbytes = 0: constants are copied in place by the walking lane
      const bool inplace = jbytes == 0;
      const uint32_t need = active ? (kA + kB) * 4u : 0u;
      const uint32_t incl = wave_scan_incl(need);
      const uint32_t jtotal = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      const bool jfit = !inplace && jtotal <= jbytes;
      const unsigned long long t3 = stamp();
      tk[2] += t3 - t2;
      if (active && jfit) {
        // the fused walk: chain A = steps 0..31 from (start state, o0), chain B = steps 32..63 from (middle state, o0 + lenA);
        // HALF: the lane's one chain
        uint32_t oA = o0, pA = jarea + incl - need;
        if constexpr (HALF) {
          if (D.wide) { if constexpr (K == 1) piece_dfwalk1cw_k1(w, wp, hA, oA, pA); else piece_dfwalk1cw_k2(w, wp, hA, oA, pA); }
          else { if constexpr (K == 1) piece_dfwalk1c_k1(w, wp, hA, oA, pA); else piece_dfwalk1c_k2(w, wp, hA, oA, pA); }
        } else {
          uint32_t oB = o0 + lenA, pB = pA + 4u * kA;
          if (D.wide) {   // (more than 31 byte classes: one more shift per step)
            if constexpr (K == 1) piece_dfwalk2cw_k1(w, wp, hA, oA, hB, oB, pA, pB);
            else piece_dfwalk2cw_k2(w, wp, hA, oA, hB, oB, pA, pB);
          } else {
            if constexpr (K == 1) piece_dfwalk2c_k1(w, wp, hA, oA, hB, oB, pA, pB);
            else piece_dfwalk2c_k2(w, wp, hA, oA, hB, oB, pA, pB);
          }
        }
      }
      uint32_t njobs = jfit ? jtotal >> 2 : 0u;
      if (!jfit) {
        // more constants than slots: the walking lanes copy them in place
        if (!inplace && lane == first) atomicAdd(&flags->emit_ovf, cnt);
        if (active) {
          for (int ch = 0; ch < (HALF ? 1 : 2); ++ch) {
            uint32_t h = ch ? hB : hA;
            uint64_t o = (uint64_t)(o0 - stga) + (ch ? lenA : 0u);
            for (int t = ch * HALF_BYTES; t < (ch + 1) * HALF_BYTES; ++t) {
              const int ts = t - K;
              const uint32_t bn = (w[t >> 2] >> ((t & 3) * 8)) & 0xFFu;
              const uint32_t bo_ = ts >= 0 ? (w[ts >> 2] >> ((ts & 3) * 8)) & 0xFFu : (wp >> ((4 + ts) * 8)) & 0xFFu;
              df_step_gen<1>(h, bn, bo_, o, stg, L, D);
            }
          }
        }
      }
      wave_lds_fence();
      const unsigned long long t4 = stamp();
      tk[3] += t4 - t3;
      // constants: one lane per job.  A constant lands at an arbitrary staging address d: its bytes up to the next 4-byte boundary
      // leave as byte stores, everything behind as ALIGNED DWORD stores — the pool holds every constant four times, copy s starting
      // at its byte s, so the dwords are one aligned 16-byte read of copy (bytes before the boundary) — and the last 0-3 bytes as
      // byte stores again: at most 3 + 4 + 3 store instructions per 16 bytes where bytewise copying takes 16 (an unaligned dword
      // store would cost a wave ~64 cycles: profiles/r03_lds_cost_table.txt)
      __builtin_amdgcn_s_setprio(KX_PRIO_CONSTANTS);
      for (uint32_t j0 = 0; j0 < njobs; j0 += 64) {
        const uint32_t j = j0 + lane;
        uint32_t l = 0, d = 0, off0 = 0;
        if (j < njobs) {
          const uint32_t jw = *reinterpret_cast<const uint32_t*>((const uint8_t*)smem + jarea + 4 * j);
          const uint32_t e = *reinterpret_cast<const uint32_t*>(L.base + (jw & 0xFFFFu) + 4);   // (the job names the entry; what it writes is its hi word)
          const uint32_t cp = E_COPY(e);
          l = (e >> 24) - cp;
          d = stga + (((jw >> 16) - stga) & 0xFFFFu) + cp;
          off0 = D.off_pool + (E_AID(e) << 4);
        }
        const uint32_t tob = (0u - d) & 3u, nh = l < tob ? l : tob, rem = l - nh;
        const uint32_t src = off0 + nh * ((l + 15u) & ~15u), d1 = d + nh;
        const uint32_t v0 = *reinterpret_cast<const uint32_t*>(L.base + off0);
        uint4 wv = *reinterpret_cast<const uint4*>(L.base + src);
        put_bytes3(nh, d, v0);
        for (uint32_t base = 0;; base += 16) {
          const uint32_t left = rem > base ? rem - base : 0u, m = left >> 2 < 4u ? left >> 2 : 4u;
          const uint32_t w4[4] = {wv.x, wv.y, wv.z, wv.w};
          put_dwords4(m, d1 + base, w4);
          const uint32_t nt = left < 16u ? left & 3u : 0u;
          const uint32_t tw = m == 0 ? wv.x : m == 1 ? wv.y : m == 2 ? wv.z : wv.w;
          put_bytes3(nt, d1 + base + 4u * m, tw);
          if (!__any(rem > base + 16u)) break;
          wv = *reinterpret_cast<const uint4*>(L.base + src + base + 16u);
        }
      }
      wave_lds_fence();
      __builtin_amdgcn_s_setprio(KX_PRIO_FLUSH);
      const unsigned long long t5 = stamp();
      tk[4] += t5 - t4;
      if (lastl + 1 >= nvalid) { cur = nx; taken = true; }   // (the iteration's last round: the next iteration's operands leave the load registers before the stores go out)
      // flush [gs, ge): partial head and tail windows bytewise, everything between as aligned 16 B
      const uint64_t ge = wave_read64(oend, lastl);
      const uint64_t fs = (gs + 15) & ~15ull, fe = ge & ~15ull;
      if (fs >= fe) {
        for (uint64_t x = gs + lane; x < ge; x += 64) out[x] = stg[x - abase];
      } else {
        if (gs + lane < fs) out[gs + lane] = stg[gs + lane - abase];
        if (fe + lane < ge) out[fe + lane] = stg[fe + lane - abase];
        for (uint64_t x = fs + (uint64_t)lane * 16; x < fe; x += 1024)
          *reinterpret_cast<uint4*>(out + x) = *reinterpret_cast<const uint4*>(stg + (x - abase));
      }
      wave_lds_fence();
      __builtin_amdgcn_s_setprio(0);
      t2 = stamp();
      tk[5] += t2 - t5;
      first = lastl + 1;
    }
    if (!taken) cur = nx;   // (the iteration ended in a lane that wrote its piece directly)
  }
  if ((D.debug & 64u) && lane == 0)
    for (int i = 0; i < 6; ++i) atomicAdd(&flags->dbg[i], tk[i]);
}
