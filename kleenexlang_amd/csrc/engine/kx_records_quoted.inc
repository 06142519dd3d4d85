// kx_records_quoted.inc — device side of quote-aware record mode (include/kxhip.h: kx_split_records_quoted,
// kx_run_records_fd_quoted): cut a buffer into records after every separator byte that lies outside quotes.  Included by
// kx_engine.hip behind kx_records.inc, whose tile shape, granule rule and byte test it reuses; the host side is in
// kx_records_host.inc.
//
// The quote state at a byte is the parity of the quote bytes before it, counted from the stream's start (parity_in carries it
// into the buffer).  A separator ends a record iff that parity is even; since quote != sep, the parity "before" and "at" a
// separator are the same.  Per granule a lane packs the separator and the quote masks to 16 bits each (bit i = byte i).  The
// parity at each granule start inside a tile comes from three parts: the in-wave prefix (mbcnt of a ballot of each granule's
// quote parity), the (step, wave) totals (one bit each, 64 entries in LDS, every wave ballots them) and the tile's start parity.
//   k_rqcount   workgroup = tile: quotes, separators, and the separators outside quotes if the tile starts at even parity
//   k_scan_groups over the quote counts: each tile's start parity (^ parity_in); Flags::total_len = all quotes
//   k_rqselect  per tile: the count of separators outside quotes for the tile's real start parity (even, or total − even)
//   k_scan_groups over those: the tiles' first ranks; Flags::total_len = all separators outside quotes
//   k_rqwrite   workgroup = tile: the masks again; ranks as k_rwrite (five ballots + mbcnt, then the (step, wave) totals);
//               each valid separator at relative byte r writes off[1 + rank] = base + r + 1
// Bytes read: 2 n; bytes written: 8 per record.

// high bits 7, 15, 23, 31 of a match word → bits 0-3: (m >> 7) has them at 0, 8, 16, 24, and the product's partial terms
// (8 i + 7 k, i, k < 4) never collide, so bits 28-31 of it are exactly those four
__device__ __forceinline__ uint32_t rq_pack4(uint32_t m) { return ((m >> 7) * 0x10204080u) >> 28; }

// granule g of a0: bits 0-15 the separator bytes, bits 16-31 the quote bytes, bytes outside [lo, hi) — offsets from a0 — cleared
__device__ __forceinline__ uint32_t rq_masks(const uint8_t* __restrict__ a0, unsigned long long g, unsigned long long lo,
                                             unsigned long long hi, uint32_t spat, uint32_t qpat) {
  const uint4 v = *reinterpret_cast<const uint4*>(a0 + 16ull * g);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t s = 0, q = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t ms = w[k] ^ spat, mq = w[k] ^ qpat;   // the exact zero-byte test of rec_match
    ms = ~(((ms & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | ms | 0x7F7F7F7Fu);
    mq = ~(((mq & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | mq | 0x7F7F7F7Fu);
    s |= rq_pack4(ms) << (4 * k);
    q |= rq_pack4(mq) << (4 * k);
  }
  // keep bytes [lo - o, hi - o) (all 16 but in the first and the last granule); selects, not a branch, so that the loads of a
  // tile stay in flight together
  const unsigned long long o = 16ull * g;
  const uint32_t a = o < lo ? (uint32_t)(lo - o) : 0u, b = o + 16 > hi ? (uint32_t)(hi - o) : 16u;
  const uint32_t keep = (0xFFFFu >> (16u - b)) & (0xFFFFu << a);
  return (s & keep) | (q & keep) << 16;
}

// the tile's packed masks into m[]; a full tile loads without a bounds test so that all REC_G loads are in flight together
__device__ __forceinline__ void rq_load_tile(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo,
                                             unsigned long long hi, uint32_t spat, uint32_t qpat, uint32_t (&m)[REC_G]) {
  const unsigned long long g0 = (unsigned long long)blockIdx.x * REC_TILE + threadIdx.x;
  if ((unsigned long long)(blockIdx.x + 1) * REC_TILE <= ng) {
#pragma unroll
    for (uint32_t j = 0; j < REC_G; ++j) m[j] = rq_masks(a0, g0 + j * REC_BT, lo, hi, spat, qpat);
  } else {
#pragma unroll
    for (uint32_t j = 0; j < REC_G; ++j) {
      const unsigned long long g = g0 + j * REC_BT;
      m[j] = g < ng ? rq_masks(a0, g, lo, hi, spat, qpat) : 0u;
    }
  }
}

__device__ __forceinline__ uint32_t rq_lane_prefix(unsigned long long bal) {   // set bits of bal in the lanes below this one
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
}

// The separators outside quotes of each granule, for tile start parity tpar, in place of m[] (16 bits each).  Ends with a barrier;
// wp[] is 64 words of LDS.
__device__ __forceinline__ void rq_valid(uint32_t (&m)[REC_G], uint32_t tpar, uint32_t* wp) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t gp = 0;   // bit j: parity of the quotes before granule j of this lane, inside its (step, wave) group
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {
    const unsigned long long bal = __ballot(__popc(m[j] >> 16) & 1u);
    gp |= (rq_lane_prefix(bal) & 1u) << j;
    if (lane == 0) wp[j * (REC_BT / 64) + w] = (uint32_t)__popcll(bal) & 1u;
  }
  __syncthreads();
  const unsigned long long tot = __ballot(wp[lane] != 0);   // (step, wave) group k = 4 j + w at bit k; every wave the same
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {
    const uint32_t k = j * (REC_BT / 64) + w;
    const uint32_t par = tpar ^ ((gp >> j) & 1u) ^ ((uint32_t)__popcll(tot & ((1ull << k) - 1ull)) & 1u);
    uint32_t p = m[j] >> 16;   // inclusive prefix parity of the quotes inside the granule
    p ^= p << 1;
    p ^= p << 2;
    p ^= p << 4;
    p ^= p << 8;
    m[j] &= (par ? p : ~p) & 0xFFFFu;
  }
  __syncthreads();   // (wp is free again)
}

// per tile: tq = quotes, tsep = separators, teven = separators outside quotes if the tile starts at even parity
__global__ __launch_bounds__(REC_BT) void k_rqcount(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo,
                                                    unsigned long long hi, uint32_t spat, uint32_t qpat, unsigned long long* __restrict__ tq,
                                                    unsigned long long* __restrict__ tsep, unsigned long long* __restrict__ teven) {
  __shared__ uint32_t wp[REC_G * (REC_BT / 64)];
  __shared__ uint32_t red[3][REC_BT / 64];
  uint32_t m[REC_G];
  rq_load_tile(a0, ng, lo, hi, spat, qpat, m);
  uint32_t cq = 0, cs = 0;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {
    cq += __popc(m[j] >> 16);
    cs += __popc(m[j] & 0xFFFFu);
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
  }
}

// per tile: its count of separators outside quotes, from its start parity (the exclusive scan of the quote counts, ^ parity_in)
__global__ void k_rqselect(uint32_t ntiles, const unsigned long long* __restrict__ tqoff, const unsigned long long* __restrict__ tsep,
                           const unsigned long long* __restrict__ teven, uint32_t parity_in, unsigned long long* __restrict__ tcount) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntiles) return;
  tcount[t] = ((tqoff[t] ^ parity_in) & 1u) ? tsep[t] - teven[t] : teven[t];
}

// tail: the buffer does not end in a separator outside quotes — off[nsep + 1] = base + n closes the last record
__global__ __launch_bounds__(REC_BT) void k_rqwrite(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo,
                                                    unsigned long long hi, uint32_t spat, uint32_t qpat,
                                                    const unsigned long long* __restrict__ tqoff, uint32_t parity_in,
                                                    const unsigned long long* __restrict__ toff, unsigned long long base,
                                                    unsigned long long nsep, int tail, unsigned long long* __restrict__ off) {
  __shared__ uint32_t wt[REC_G * (REC_BT / 64)], wb[REC_G * (REC_BT / 64)];
  static_assert(REC_G * (REC_BT / 64) == 64, "one wave scans the (step, wave) totals");
  uint32_t m[REC_G];
  rq_load_tile(a0, ng, lo, hi, spat, qpat, m);
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
    for (int d = 1; d < 64; d <<= 1) { const uint32_t x = __shfl_up(s, d); if (lane >= (uint32_t)d) s += x; }
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
    for (uint32_t x = m[j]; x; x &= x - 1) off[1 + r++] = base + rel + __builtin_ctz(x) + 1;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    off[0] = base;
    if (tail) off[nsep + 1] = base + (hi - lo);
  }
}
