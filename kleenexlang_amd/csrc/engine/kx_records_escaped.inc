// kx_records_escaped.inc — device side of escape-aware record mode (include/kxhip.h: kx_split_records_escaped,
// kx_run_records_fd_escaped): cut a buffer into records after every separator byte that is not escaped and, with a quote byte,
// lies outside quotes.  Included by kx_engine.hip behind kx_records_quoted.inc, whose masks, parity pass (rq_valid) and tile shape
// it reuses; the host side is in kx_records_host.inc.
//
// An unescaped escape byte E escapes the next byte; an escaped byte is only data (never a separator, a quote or an escape).  The
// escape state entering a 16-byte granule is one bit c; its escaped mask is simdjson's find_escaped_branchless restated for 16 bits
// (re_esc).  A granule of 16 E passes c through; any other granule's carry-out is independent of c.  So the carry into a granule
// is the carry-out of the nearest granule before it that is not all E (the "copy-or-set" monoid), or the tile's carry-in T if
// there is none; the same holds for tiles, a tile being transparent only if it is 64 KiB of E.  Within a tile the nearest such
// granule comes from a ballot of "not all E" with the carry-outs ballotted beside it, then the 64 (step, wave) groups through LDS
// (re_carries); only then does the quote parity run, over the unescaped quotes (rq_valid).
//
// A tile's counts depend on T only through its first granule F that is not all E, and there only through F's first byte that is
// not E (its escaped bit flips with T; every byte before it in the tile is E).  If that byte is a quote, T flips the parity of every
// separator of the tile; if it is a separator, it counts or not.  So one count pass gives the counts for T = 0 plus F's delta:
//   k_recount  workgroup = tile: unescaped quotes, unescaped separators, and those at even parity from an even tile start, all for
//              T = 0; the tile's flag word (transparent, carry-out, F's quote / separator delta, the last byte's state for T = 0, 1)
//   k_rescan   one workgroup: each tile's T by the copy-or-set scan of the flag words; the quote counts become those for T
//   k_scan_groups over the quote counts: each tile's start parity (^ parity_in); Flags::total_len = all unescaped quotes
//   k_reselect per tile: the count of valid separators for (T, parity); the last tile also writes *info (is the last byte a valid
//              separator, the state after the buffer) for the host's single read
//   k_scan_groups over those: the tiles' first ranks; Flags::total_len = all valid separators
//   k_rewrite  workgroup = tile: the masks again, the escaped masks for the real T, rq_valid for the real parity; ranks as k_rqwrite
// The first granule's bytes before the buffer are cleared; state_in's escape bit enters as an E just before the buffer's first byte
// (re_masks), and tile 0 then starts at T = 0.  Bytes read: 2 n; bytes written: 8 per record.

// flag word of a tile (k_recount; bit RE_T by k_rescan)
constexpr uint32_t RE_TRANSPARENT = 1u, RE_CO = 2u;            // all E; carry-out (any T) if not transparent
constexpr uint32_t RE_DQ = 4u, RE_DQNEG = 8u;                  // T = 1 adds (RE_DQNEG: removes) one unescaped quote
constexpr uint32_t RE_DS = 16u, RE_DSNEG = 32u;                // ... one unescaped separator
constexpr uint32_t RE_LASTS = 64u, RE_LASTE = 256u;            // (last tile) the last byte is an unescaped separator / E: bit << T
constexpr uint32_t RE_T = 1u << 16;                            // the tile's escape carry-in

// the escaped bytes of a granule with escape mask e (16 bits) and carry-in c (0, 1); *co = the carry-out (its byte 16 is escaped)
__device__ __forceinline__ uint32_t re_esc(uint32_t e, uint32_t c, uint32_t* co) {
  const uint32_t EVEN = 0x5555u;
  const uint32_t b = e & ~c;                 // (a first byte that is escaped escapes nothing)
  const uint32_t fe = b << 1 | c;            // bytes that follow an escape
  const uint32_t odd = b & ~EVEN & ~fe;      // runs of E that start on an odd bit
  const uint32_t sum = odd + b;              // bit 16: the carry-out
  *co = sum >> 16;
  return (EVEN ^ (sum << 1)) & fe & 0xFFFFu;
}

// granule g of a0: *sq = separator bits 0-15, quote bits 16-31 (qkeep = 0: no quote byte); *e = escape bits 0-15; bytes outside
// [lo, hi) cleared, and in the granule that holds lo, byte lo - 1 set as an E iff x (state_in's escape bit)
__device__ __forceinline__ void re_masks(const uint8_t* __restrict__ a0, unsigned long long g, unsigned long long lo, unsigned long long hi,
                                         uint32_t spat, uint32_t qpat, uint32_t qkeep, uint32_t epat, uint32_t x, uint32_t* sq,
                                         uint32_t* e) {
  const uint4 v = *reinterpret_cast<const uint4*>(a0 + 16ull * g);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t s = 0, q = 0, es = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t ms = w[k] ^ spat, mq = w[k] ^ qpat, me = w[k] ^ epat;   // the exact zero-byte test of rec_match
    ms = ~(((ms & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | ms | 0x7F7F7F7Fu);
    mq = ~(((mq & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | mq | 0x7F7F7F7Fu);
    me = ~(((me & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | me | 0x7F7F7F7Fu);
    s |= rq_pack4(ms) << (4 * k);
    q |= rq_pack4(mq) << (4 * k);
    es |= rq_pack4(me) << (4 * k);
  }
  const unsigned long long o = 16ull * g;
  const uint32_t a = o < lo ? (uint32_t)(lo - o) : 0u, b = o + 16 > hi ? (uint32_t)(hi - o) : 16u;
  const uint32_t keep = (0xFFFFu >> (16u - b)) & (0xFFFFu << a);
  *sq = (s & keep) | ((q & keep) << 16 & qkeep);
  *e = (es & keep) | (a ? x << (a - 1) : 0u);
}

// the tile's masks into sq[], e[]; a full tile loads without a bounds test so that all REC_G loads are in flight together
__device__ __forceinline__ void re_load_tile(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo,
                                             unsigned long long hi, uint32_t spat, uint32_t qpat, uint32_t qkeep, uint32_t epat, uint32_t x,
                                             uint32_t (&sq)[REC_G], uint32_t (&e)[REC_G]) {
  const unsigned long long g0 = (unsigned long long)blockIdx.x * REC_TILE + threadIdx.x;
  if ((unsigned long long)(blockIdx.x + 1) * REC_TILE <= ng) {
#pragma unroll
    for (uint32_t j = 0; j < REC_G; ++j) re_masks(a0, g0 + j * REC_BT, lo, hi, spat, qpat, qkeep, epat, x, &sq[j], &e[j]);
  } else {
#pragma unroll
    for (uint32_t j = 0; j < REC_G; ++j) {
      const unsigned long long g = g0 + j * REC_BT;
      if (g < ng) re_masks(a0, g, lo, hi, spat, qpat, qkeep, epat, x, &sq[j], &e[j]);
      else sq[j] = e[j] = 0u;
    }
  }
}

__device__ __forceinline__ uint32_t re_high(unsigned long long v) { return 63u - (uint32_t)__clzll((long long)v); }   // v != 0

// The escape carry into each granule of this lane: bit j of *cin for granule j, and bit j of *dep set where the carry is the tile's
// carry-in T (no granule before it in the tile is not all E; *cin's bit is 0 there).  *tile = the tile's flag bits RE_TRANSPARENT,
// RE_CO (the same in every thread).  Ends with a barrier; wp[] is 64 words of LDS.
__device__ __forceinline__ void re_carries(const uint32_t (&e)[REC_G], uint32_t* wp, uint32_t* cin, uint32_t* dep, uint32_t* tile) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t ci = 0, known = 0;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {
    uint32_t co;
    (void)re_esc(e[j], 0u, &co);
    const unsigned long long bn = __ballot(e[j] != 0xFFFFu), bc = __ballot(co);
    const unsigned long long b = bn & below;
    if (b) { known |= 1u << j; ci |= (uint32_t)((bc >> re_high(b)) & 1ull) << j; }
    if (lane == 0) wp[j * (REC_BT / 64) + w] = bn ? 1u | (uint32_t)((bc >> re_high(bn)) & 1ull) << 1 : 0u;
  }
  __syncthreads();
  const uint32_t v = wp[lane];   // (step, wave) group k = 4 j + w at bit k; every wave the same
  const unsigned long long gh = __ballot(v & 1u), gc = __ballot(v >> 1);
  uint32_t dp = 0;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {
    if ((known >> j) & 1u) continue;
    const unsigned long long b = gh & ((1ull << (j * (REC_BT / 64) + w)) - 1ull);
    if (b) ci |= (uint32_t)((gc >> re_high(b)) & 1ull) << j;
    else dp |= 1u << j;
  }
  *cin = ci;
  *dep = dp;
  *tile = gh ? (uint32_t)((gc >> re_high(gh)) & 1ull) * RE_CO : RE_TRANSPARENT;
  __syncthreads();   // (wp is free again)
}

// per tile, for T = 0: tq = unescaped quotes, tsep = unescaped separators, teven = those at even parity from an even tile start;
// tflag = the flag word
__global__ __launch_bounds__(REC_BT) void k_recount(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo,
                                                    unsigned long long hi, uint32_t spat, uint32_t qpat, uint32_t qkeep, uint32_t epat,
                                                    uint32_t x, unsigned long long* __restrict__ tq, unsigned long long* __restrict__ tsep,
                                                    unsigned long long* __restrict__ teven, uint32_t* __restrict__ tflag) {
  __shared__ uint32_t wp[REC_G * (REC_BT / 64)];
  __shared__ uint32_t red[3][REC_BT / 64];
  __shared__ uint32_t flag;
  uint32_t m[REC_G], e[REC_G];
  re_load_tile(a0, ng, lo, hi, spat, qpat, qkeep, epat, x, m, e);
  if (threadIdx.x == 0) flag = 0;
  uint32_t cin, dep, tile;
  re_carries(e, wp, &cin, &dep, &tile);
  const unsigned long long g0 = (unsigned long long)blockIdx.x * REC_TILE + threadIdx.x;
  uint32_t cq = 0, cs = 0;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {
    uint32_t co;
    const uint32_t esc = re_esc(e[j], (cin >> j) & 1u, &co), raw = m[j];
    m[j] &= ~(esc | esc << 16);
    cq += __popc(m[j] >> 16);
    cs += __popc(m[j] & 0xFFFFu);
    const bool first = ((dep >> j) & 1u) && e[j] != 0xFFFFu;   // F, the tile's first granule that is not all E
    const bool last = g0 + j * REC_BT == ng - 1;                 // the granule of the buffer's last byte
    if (first || last) {
      const uint32_t d = (dep >> j) & 1u;
      const uint32_t esc1 = d ? re_esc(e[j], 1u, &co) : esc;     // the escaped mask for T = 1
      uint32_t f = 0;
      if (first) {
        const int dq = __popc((raw >> 16) & ~esc1) - __popc(m[j] >> 16), ds = __popc(raw & 0xFFFFu & ~esc1) - __popc(m[j] & 0xFFFFu);
        f |= dq ? RE_DQ | (dq < 0 ? RE_DQNEG : 0u) : 0u;
        f |= ds ? RE_DS | (ds < 0 ? RE_DSNEG : 0u) : 0u;
      }
      if (last) {
        const uint32_t bl = (uint32_t)(hi - 1 - 16ull * (ng - 1));
        f |= ((raw & ~esc) >> bl & 1u) * RE_LASTS | ((raw & ~esc1) >> bl & 1u) * (RE_LASTS << 1);
        f |= ((e[j] & ~esc) >> bl & 1u) * RE_LASTE | ((e[j] & ~esc1) >> bl & 1u) * (RE_LASTE << 1);
      }
      atomicOr(&flag, f);
    }
  }
  rq_valid(m, 0u, wp);
  uint32_t ce = 0;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) ce += __popc(m[j]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    cq += __shfl_xor(cq, d);
    cs += __shfl_xor(cs, d);
    ce += __shfl_xor(ce, d);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = cq;
    red[1][threadIdx.x >> 6] = cs;
    red[2][threadIdx.x >> 6] = ce;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long s = 0;
    for (uint32_t w = 0; w < REC_BT / 64; ++w) s += red[threadIdx.x][w];
    (threadIdx.x == 0 ? tq : threadIdx.x == 1 ? tsep : teven)[blockIdx.x] = s;
  } else if (threadIdx.x == 64) {
    tflag[blockIdx.x] = flag | tile;
  }
}

// One workgroup of 1024: each tile's escape carry-in T (RE_T in tflag) by the copy-or-set scan over the tiles in chunks of 1024,
// from t0 before tile 0; tq[t] becomes the tile's unescaped quotes for T.
__global__ __launch_bounds__(1024) void k_rescan(uint32_t ntiles, uint32_t t0, uint32_t* __restrict__ tflag,
                                                 unsigned long long* __restrict__ tq) {
  __shared__ uint32_t ws[16];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t carry = t0;
  for (uint32_t base = 0; base < ntiles; base += 1024) {
    const uint32_t t = base + threadIdx.x;
    const uint32_t f = t < ntiles ? tflag[t] : RE_TRANSPARENT;
    const unsigned long long bh = __ballot(!(f & RE_TRANSPARENT)), bc = __ballot(f & RE_CO);
    if (lane == 0) ws[w] = bh ? 1u | (uint32_t)((bc >> re_high(bh)) & 1ull) << 1 : 0u;
    __syncthreads();
    uint32_t c = carry;
    const unsigned long long b = bh & ((1ull << lane) - 1ull);
    if (b) c = (uint32_t)((bc >> re_high(b)) & 1ull);
    else for (uint32_t k = 0; k < w; ++k) if (ws[k] & 1u) c = ws[k] >> 1;   // (the last wave below with a carry-out)
    for (uint32_t k = 0; k < 16; ++k) if (ws[k] & 1u) carry = ws[k] >> 1;
    if (t < ntiles) {
      tflag[t] = f | c * RE_T;
      if (c && (f & RE_DQ)) tq[t] = (f & RE_DQNEG) ? tq[t] - 1 : tq[t] + 1;
    }
    __syncthreads();   // (ws is free again)
  }
}

// per tile: its count of valid separators for its T and start parity (the exclusive scan of the quote counts, ^ parity_in).  The
// last tile writes *info: bit 0 the last byte is a valid separator, bit 1 the quote parity after the buffer, bit 2 its escape state.
__global__ void k_reselect(uint32_t ntiles, const uint32_t* __restrict__ tflag, const unsigned long long* __restrict__ tq,
                           const unsigned long long* __restrict__ tqoff, const unsigned long long* __restrict__ tsep,
                           const unsigned long long* __restrict__ teven, uint32_t parity_in, unsigned long long* __restrict__ tcount,
                           uint32_t* __restrict__ info) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntiles) return;
  const uint32_t f = tflag[t], T = (f & RE_T) ? 1u : 0u;
  unsigned long long cs = tsep[t], ce = teven[t];
  if (T && (f & RE_DQ)) ce = cs - ce;   // (the flipped quote precedes every separator of the tile)
  if (T && (f & RE_DS)) {               // (the separator at the flipped byte has no quote before it in the tile)
    cs = (f & RE_DSNEG) ? cs - 1 : cs + 1;
    ce = (f & RE_DSNEG) ? ce - 1 : ce + 1;
  }
  tcount[t] = ((tqoff[t] ^ parity_in) & 1u) ? cs - ce : ce;
  if (t == ntiles - 1) {
    const uint32_t pout = (uint32_t)((tqoff[t] + tq[t] + parity_in) & 1u);
    const uint32_t lasts = (f >> T) & RE_LASTS, laste = (f >> T) & RE_LASTE;
    *info = (lasts && !pout ? 1u : 0u) | pout << 1 | (laste ? 4u : 0u);
  }
}

// tail: the buffer does not end in a valid separator — off[nsep + 1] = base + n closes the last record
__global__ __launch_bounds__(REC_BT) void k_rewrite(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo,
                                                    unsigned long long hi, uint32_t spat, uint32_t qpat, uint32_t qkeep, uint32_t epat,
                                                    uint32_t x, const uint32_t* __restrict__ tflag,
                                                    const unsigned long long* __restrict__ tqoff, uint32_t parity_in,
                                                    const unsigned long long* __restrict__ toff, unsigned long long base,
                                                    unsigned long long nsep, int tail, unsigned long long* __restrict__ off) {
  __shared__ uint32_t wt[REC_G * (REC_BT / 64)], wb[REC_G * (REC_BT / 64)];
  static_assert(REC_G * (REC_BT / 64) == 64, "one wave scans the (step, wave) totals");
  uint32_t m[REC_G], e[REC_G];
  re_load_tile(a0, ng, lo, hi, spat, qpat, qkeep, epat, x, m, e);
  uint32_t cin, dep, tile;
  re_carries(e, wt, &cin, &dep, &tile);
  cin |= (tflag[blockIdx.x] & RE_T) ? dep : 0u;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {
    uint32_t co;
    const uint32_t esc = re_esc(e[j], (cin >> j) & 1u, &co);
    m[j] &= ~(esc | esc << 16);
  }
  rq_valid(m, (uint32_t)((tqoff[blockIdx.x] ^ parity_in) & 1u), wt);
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t pre[REC_G];
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {   // in-wave exclusive prefix of the granule counts, five bits at a time (as k_rwrite)
    const uint32_t c = __popc(m[j]);
    uint32_t p = 0, t = 0;
#pragma unroll
    for (int b = 0; b < 5; ++b) {
      const unsigned long long bal = __ballot((c >> b) & 1u);
      p += rq_lane_prefix(bal) << b;
      t += (uint32_t)__popcll(bal) << b;
    }
    pre[j] = p;
    if (lane == 0) wt[j * (REC_BT / 64) + w] = t;
  }
  __syncthreads();
  if (w == 0) {   // granule order is step-major, then wave: exclusive scan of the 64 totals in that order
    const uint32_t v = wt[lane];
    uint32_t s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(s, d); if (lane >= (uint32_t)d) s += y; }
    wb[lane] = s - v;
  }
  __syncthreads();
  const unsigned long long tb = toff[blockIdx.x];
  const unsigned long long g0 = (unsigned long long)blockIdx.x * REC_TILE + threadIdx.x;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {
    if (!m[j]) continue;
    unsigned long long r = tb + wb[j * (REC_BT / 64) + w] + pre[j];
    const unsigned long long rel = 16ull * (g0 + j * REC_BT) - lo;   // (relative offset of the granule's byte 0; lo ≤ its first match)
    for (uint32_t y = m[j]; y && r < nsep; y &= y - 1) off[1 + r++] = base + rel + __builtin_ctz(y) + 1;   // (never past the count)
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    off[0] = base;
    if (tail) off[nsep + 1] = base + (hi - lo);
  }
}
