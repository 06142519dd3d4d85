// kx_records_rs.inc — device side of record mode with a multi-byte separator (include/kxhip.h: kx_split_records_rs,
// kx_run_records_fd_rs): cut a buffer into records after the leftmost, non-overlapping copies of a separator rs of m = 1-8 bytes,
// as bytes.split(rs) finds them.  Included by kx_engine.hip behind kx_records_escaped.inc; the tile shape, the granule rule and the
// byte test are those of kx_records.inc, the packing and the ranks those of kx_records_quoted.inc; the host side is in
// kx_records_host.inc.
//
// Candidates.  Bit i of a granule's candidate mask is set when a copy of rs ENDS at its byte i.  A lane holds its granule and the
// last 8 bytes of the granule before it (24 bytes, positions -8 .. 15); per separator byte b the exact byte test gives 24 equality
// bits, and the mask is the AND over b of (eq_b << (m - 1 - b)), bits 8-23.  The k context bytes (k < m) stand for the bytes
// [lo - k, lo) right before the buffer: they replace what memory holds there (rs_window; only granules 0 and 1 can see them), and a
// copy must start at or after lo - k and end before hi, so ends outside [lo - k + m - 1, hi) are cleared.  The granule before the
// first one is never read: granule 0 takes its own first 8 bytes in its place, all of which lie before lo - k.
//
// Border-free separators (no proper prefix of rs is a suffix) cannot overlap themselves: every candidate is selected.
//   k_rbcount  workgroup = tile: the candidates of the tile
//   k_scan_groups over the counts; k_rbwrite: the masks again, ranks as k_rqwrite
//
// Self-overlapping separators.  A candidate ending at e is selected iff e - (the last selected end) >= m.  The state entering a
// granule is t in [0, m - 1]: its end positions < t are blocked.  Inside a granule the selection from t is a short greedy loop
// (rs_select); the state it leaves is max(0, last selected bit + m - 16), and 0 if it selects nothing.  A granule is therefore a map
// t -> t' of eight 3-bit entries (rs_map), and maps compose: in the wave (rs_wave_scan, Hillis-Steele over shuffles, skipped when
// every map of the wave is constant — then each map is its own inclusive prefix), across the 64 (step, wave) groups through LDS,
// and across tiles in k_rsscan.  Beside its map a granule keeps the count of its selection for each t (4 bits each); with the
// prefix map P of a granule inside its tile the tile's count for the entering state T is the sum of count[P[T]], kept for all m T.
//   k_rocount  workgroup = tile: the tile's map, its m counts, and (last tile) whether the buffer's last byte is selected, per T
//   k_rsscan   one workgroup: each tile's entering state by the scan of the maps from 0; tcount[t] = its count for that state
//   k_scan_groups over those; k_rowrite: masks and maps again, the selection for the real state, ranks as k_rqwrite
// Bytes read: 2 n (+ 8 bytes per granule that hit the cache line of the lane before); bytes written: 8 per record.

constexpr uint32_t RS_ID = 0xFAC688u;        // the identity map: entry t (bits 3 t .. 3 t + 2) = t
constexpr uint32_t RS_ONES = 0x249249u;      // bit 0 of each entry

__device__ __forceinline__ unsigned long long rs_shift_bytes(unsigned long long x, int s) {   // x moved up by s bytes (down: s < 0)
  return s >= 8 || s <= -8 ? 0ull : s >= 0 ? x << (8 * s) : x >> (-8 * s);
}

// The 24 bytes of granule g: w[0, 1] = the 8 bytes before it, w[2 .. 5] = the granule; the context bytes (ctx8, k of them, the
// first in the low byte) in place of [lo - k, lo).
__device__ __forceinline__ void rs_window(const uint8_t* __restrict__ a0, unsigned long long g, unsigned long long lo, unsigned long long ctx8,
                                          uint32_t k, uint32_t (&w)[6]) {
  const uint4 v = *reinterpret_cast<const uint4*>(a0 + 16ull * g);
  const uint2 p = *reinterpret_cast<const uint2*>(a0 + (g ? 16ull * g - 8ull : 0ull));
  w[0] = p.x; w[1] = p.y; w[2] = v.x; w[3] = v.y; w[4] = v.z; w[5] = v.w;
  if (g <= 1 && k) {
    const unsigned long long km = ~0ull >> (64u - 8u * k);
    const int s = (int)lo - (int)k - (16 * (int)g - 8);   // byte of the window that holds the first context byte (may be < 0, > 23)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      unsigned long long x = (unsigned long long)w[2 * i] | (unsigned long long)w[2 * i + 1] << 32;
      x = (x & ~rs_shift_bytes(km, s - 8 * i)) | rs_shift_bytes(ctx8, s - 8 * i);
      w[2 * i] = (uint32_t)x;
      w[2 * i + 1] = (uint32_t)(x >> 32);
    }
  }
}

// candidate mask of granule g (16 bits); rs8 = the separator's bytes, the first in the low byte
__device__ __forceinline__ uint32_t rs_cand(const uint8_t* __restrict__ a0, unsigned long long g, unsigned long long lo, unsigned long long hi,
                                            unsigned long long rs8, uint32_t m, unsigned long long ctx8, uint32_t k) {
  uint32_t w[6];
  rs_window(a0, g, lo, ctx8, k, w);
  uint32_t c = 0xFFFFFFu;
#pragma unroll
  for (uint32_t b = 0; b < 8; ++b) {
    if (b < m) {
      const uint32_t pat = 0x01010101u * (uint32_t)((rs8 >> (8 * b)) & 0xFFu);
      uint32_t eq = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        uint32_t x = w[i] ^ pat;   // the exact zero-byte test of rec_match
        x = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
        eq |= rq_pack4(x) << (4 * i);
      }
      c &= eq << (m - 1 - b);
    }
  }
  const unsigned long long o = 16ull * g, first = lo - k + m - 1;   // (lo - k + m - 1 >= lo: k < m)
  const uint32_t a = o < first ? (uint32_t)(first - o) : 0u, e = o + 16 > hi ? (uint32_t)(hi - o) : 16u;
  const uint32_t keep = (0xFFFFu >> (16u - e)) & (0xFFFFu << (a > 16u ? 16u : a));
  return (c >> 8) & keep;
}

// the tile's candidate masks into c[]; a full tile loads without a bounds test so that all loads are in flight together
__device__ __forceinline__ void rs_load_tile(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo, unsigned long long hi,
                                             unsigned long long rs8, uint32_t m, unsigned long long ctx8, uint32_t k, uint32_t (&c)[REC_G]) {
  const unsigned long long g0 = (unsigned long long)blockIdx.x * REC_TILE + threadIdx.x;
  if ((unsigned long long)(blockIdx.x + 1) * REC_TILE <= ng) {
#pragma unroll
    for (uint32_t j = 0; j < REC_G; ++j) c[j] = rs_cand(a0, g0 + j * REC_BT, lo, hi, rs8, m, ctx8, k);
  } else {
#pragma unroll
    for (uint32_t j = 0; j < REC_G; ++j) {
      const unsigned long long g = g0 + j * REC_BT;
      c[j] = g < ng ? rs_cand(a0, g, lo, hi, rs8, m, ctx8, k) : 0u;
    }
  }
}

// Ranks of the selected ends m[] inside the tile and their offsets (the second half of k_rqwrite).  Starts with a barrier-free
// use of wt[], so the caller leaves wt[] unused behind a barrier.
__device__ __forceinline__ void rs_rank_write(const uint32_t (&m)[REC_G], uint32_t* wt, uint32_t* wb, unsigned long long tb, unsigned long long lo,
                                              unsigned long long hi, unsigned long long base, unsigned long long nsep, int tail,
                                              unsigned long long* __restrict__ off) {
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
  const unsigned long long g0 = (unsigned long long)blockIdx.x * REC_TILE + threadIdx.x;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {
    if (!m[j]) continue;
    unsigned long long r = tb + wb[j * (REC_BT / 64) + w] + pre[j];
    const unsigned long long rel = 16ull * (g0 + j * REC_BT) - lo;   // (relative offset of the granule's byte 0; lo ≤ its first end)
    for (uint32_t y = m[j]; y && r < nsep; y &= y - 1) off[1 + r++] = base + rel + __builtin_ctz(y) + 1;   // (never past the count)
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    off[0] = base;
    if (tail) off[nsep + 1] = base + (hi - lo);
  }
}

// ------------------------------------------------------------------------------------------------------------------ border-free
__global__ __launch_bounds__(REC_BT) void k_rbcount(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo,
                                                    unsigned long long hi, unsigned long long rs8, uint32_t m, unsigned long long ctx8, uint32_t k,
                                                    unsigned long long* __restrict__ tcount) {
  __shared__ uint32_t red[REC_BT / 64];
  uint32_t c[REC_G];
  rs_load_tile(a0, ng, lo, hi, rs8, m, ctx8, k, c);
  uint32_t s = 0;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) s += __popc(c[j]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (uint32_t w = 0; w < REC_BT / 64; ++w) t += red[w];
    tcount[blockIdx.x] = t;
  }
}

// tail: the buffer does not end in a selected separator — off[nsep + 1] = base + n closes the last record
__global__ __launch_bounds__(REC_BT) void k_rbwrite(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo,
                                                    unsigned long long hi, unsigned long long rs8, uint32_t m, unsigned long long ctx8, uint32_t k,
                                                    const unsigned long long* __restrict__ toff, unsigned long long base,
                                                    unsigned long long nsep, int tail, unsigned long long* __restrict__ off) {
  __shared__ uint32_t wt[REC_G * (REC_BT / 64)], wb[REC_G * (REC_BT / 64)];
  static_assert(REC_G * (REC_BT / 64) == 64, "one wave scans the (step, wave) totals");
  uint32_t c[REC_G];
  rs_load_tile(a0, ng, lo, hi, rs8, m, ctx8, k, c);
  rs_rank_write(c, wt, wb, toff[blockIdx.x], lo, hi, base, nsep, tail, off);
}

// ------------------------------------------------------------------------------------------------------------ self-overlapping
// the ends selected from the candidates c (16 bits) entering in state t; *tout = the state the granule leaves
__device__ __forceinline__ uint32_t rs_select(uint32_t c, uint32_t t, uint32_t m, uint32_t* tout) {
  const uint32_t span = (1u << m) - 1u;
  uint32_t x = c & (0xFFFFu << t), sel = 0;
  while (x) {
    const uint32_t b = x & (0u - x);
    sel |= b;
    x &= ~(b * span);   // (the m - 1 ends behind a selected one are blocked)
  }
  const int over = sel ? 31 - __clz((int)sel) + (int)m - 16 : 0;
  *tout = over > 0 ? (uint32_t)over : 0u;
  return sel;
}

// a granule's map (entry t = the state it leaves when entered in t, t < m; the other entries 0) and *cnt = the size of its
// selection for each t, 4 bits each.  The selection from t is the one from t - 1 unless bit t - 1 is a candidate.
__device__ __forceinline__ uint32_t rs_map(uint32_t c, uint32_t m, uint32_t* cnt) {
  uint32_t f = 0, n = 0, to = 0, pc = 0;
  if (c) {
#pragma nounroll
    for (uint32_t t = 0; t < m; ++t) {
      if (t == 0 || ((c >> (t - 1)) & 1u)) pc = (uint32_t)__popc(rs_select(c, t, m, &to));
      f |= to << (3 * t);
      n |= pc << (4 * t);
    }
  }
  *cnt = n;
  return f;
}

__device__ __forceinline__ uint32_t rs_apply(uint32_t f, uint32_t t) { return (f >> (3 * t)) & 7u; }

// a, then b: entry t = b[a[t]], t < m
__device__ __forceinline__ uint32_t rs_comp(uint32_t a, uint32_t b, uint32_t m) {
  uint32_t r = 0;
#pragma unroll
  for (uint32_t t = 0; t < 8; ++t) if (t < m) r |= rs_apply(b, rs_apply(a, t)) << (3 * t);
  return r;
}

// inclusive scan of the maps of a wave in lane order
__device__ __forceinline__ uint32_t rs_wave_scan(uint32_t f, uint32_t m) {
  const uint32_t lane = threadIdx.x & 63, em = (1u << (3 * m)) - 1u;
  uint32_t inc = f;
  if (__ballot(((f ^ (f & 7u) * RS_ONES) & em) != 0u)) {   // (a constant map behind any map is itself)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(inc, d);
      if (lane >= (uint32_t)d) inc = rs_comp(y, inc, m);
    }
  }
  return inc;
}

// The prefix maps inside the tile: e[j] = the composition of the lane's granules before granule j in its (step, wave) group, *gex
// = in lane k the composition of the groups before group k = 4 j + w (every wave the same), *tile = the tile's map.  Ends with a
// barrier; wp[] is 64 words of LDS.
__device__ __forceinline__ void rs_prefixes(const uint32_t (&f)[REC_G], uint32_t m, uint32_t* wp, uint32_t (&e)[REC_G], uint32_t* gex,
                                            uint32_t* tile) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {
    const uint32_t inc = rs_wave_scan(f[j], m), up = __shfl_up(inc, 1);
    e[j] = lane ? up : RS_ID;
    if (lane == 63) wp[j * (REC_BT / 64) + w] = inc;
  }
  __syncthreads();
  const uint32_t ginc = rs_wave_scan(wp[lane], m), gup = __shfl_up(ginc, 1);
  *gex = lane ? gup : RS_ID;
  *tile = __shfl(ginc, 63);
  __syncthreads();   // (wp is free again)
}

// per tile: tmap = its map (bits 0-23) and, in the last tile, bit 24 + T: the buffer's last byte is a selected end when the tile is
// entered in state T; tcnt[8 tile + T] = its selected ends when entered in T
__global__ __launch_bounds__(REC_BT) void k_rocount(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo,
                                                    unsigned long long hi, unsigned long long rs8, uint32_t m, unsigned long long ctx8, uint32_t k,
                                                    uint32_t* __restrict__ tmap, uint32_t* __restrict__ tcnt) {
  __shared__ uint32_t wp[REC_G * (REC_BT / 64)];
  __shared__ uint32_t red[4][REC_BT / 64];
  __shared__ uint32_t lastbits;
  uint32_t c[REC_G], f[REC_G], cg[REC_G], e[REC_G];
  rs_load_tile(a0, ng, lo, hi, rs8, m, ctx8, k, c);
  if (threadIdx.x == 0) lastbits = 0;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) f[j] = rs_map(c[j], m, &cg[j]);
  uint32_t gex, tile;
  rs_prefixes(f, m, wp, e, &gex, &tile);   // (its first barrier also orders lastbits = 0)
  const uint32_t w = threadIdx.x >> 6;
  const unsigned long long g0 = (unsigned long long)blockIdx.x * REC_TILE + threadIdx.x;
  uint32_t cnt[4] = {0, 0, 0, 0};   // counts for T = 2 i (bits 0-15) and 2 i + 1 (bits 16-31); a wave's sum is at most 8192
  uint32_t lc = 0, lg = RS_ID, le = RS_ID;
  bool has_last = false;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {
    const uint32_t G = __shfl(gex, j * (REC_BT / 64) + w);
    if (g0 + j * REC_BT == ng - 1) { has_last = true; lc = c[j]; lg = G; le = e[j]; }   // the granule of the buffer's last byte
    if (!c[j]) continue;
#pragma unroll
    for (uint32_t T = 0; T < 8; ++T) {
      if (T < m) cnt[T >> 1] += ((cg[j] >> (4 * rs_apply(e[j], rs_apply(G, T)))) & 15u) << (16 * (T & 1u));
    }
  }
  if (has_last) {   // (one thread of the grid)
    uint32_t lb = 0;
    for (uint32_t T = 0; T < m; ++T) {
      uint32_t to;
      lb |= ((rs_select(lc, rs_apply(le, rs_apply(lg, T)), m, &to) >> (uint32_t)(hi - 1 - 16ull * (ng - 1))) & 1u) << T;
    }
    lastbits = lb;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt[i] += __shfl_xor(cnt[i], d);
    if ((threadIdx.x & 63) == 0) red[i][w] = cnt[i];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    uint32_t s = 0;
    for (uint32_t v = 0; v < REC_BT / 64; ++v) s += (red[threadIdx.x >> 1][v] >> (16 * (threadIdx.x & 1u))) & 0xFFFFu;
    tcnt[8ull * blockIdx.x + threadIdx.x] = s;
  } else if (threadIdx.x == 64) {
    tmap[blockIdx.x] = (tile & 0xFFFFFFu) | lastbits << 24;
  }
}

// One workgroup of 1024: each tile's entering state (tmap[t], in place of its map) by the scan of the maps over the tiles in
// chunks of 1024, from state 0 before tile 0; tcount[t] = the tile's count for that state; *info = the buffer's last byte is a
// selected end.
__global__ __launch_bounds__(1024) void k_rsscan(uint32_t ntiles, uint32_t m, uint32_t* __restrict__ tmap, const uint32_t* __restrict__ tcnt,
                                                 unsigned long long* __restrict__ tcount, uint32_t* __restrict__ info) {
  __shared__ uint32_t ws[16];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < ntiles; base += 1024) {
    const uint32_t t = base + threadIdx.x;
    const uint32_t raw = t < ntiles ? tmap[t] : RS_ID;
    const uint32_t inc = rs_wave_scan(raw & 0xFFFFFFu, m), up = __shfl_up(inc, 1);
    if (lane == 63) ws[w] = inc;
    __syncthreads();
    uint32_t s = carry;
    for (uint32_t v = 0; v < w; ++v) s = rs_apply(ws[v], s);
    const uint32_t T = lane ? rs_apply(up, s) : s;
    for (uint32_t v = 0; v < 16; ++v) carry = rs_apply(ws[v], carry);
    if (t < ntiles) {
      tmap[t] = T;
      tcount[t] = tcnt[8ull * t + T];
      if (t == ntiles - 1) *info = (raw >> (24 + T)) & 1u;
    }
    __syncthreads();   // (ws is free again)
  }
}

// tail: the buffer does not end in a selected separator — off[nsep + 1] = base + n closes the last record
__global__ __launch_bounds__(REC_BT) void k_rowrite(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo,
                                                    unsigned long long hi, unsigned long long rs8, uint32_t m, unsigned long long ctx8, uint32_t k,
                                                    const uint32_t* __restrict__ tstate, const unsigned long long* __restrict__ toff,
                                                    unsigned long long base, unsigned long long nsep, int tail,
                                                    unsigned long long* __restrict__ off) {
  __shared__ uint32_t wt[REC_G * (REC_BT / 64)], wb[REC_G * (REC_BT / 64)];
  static_assert(REC_G * (REC_BT / 64) == 64, "one wave scans the (step, wave) totals");
  uint32_t c[REC_G], f[REC_G], e[REC_G];
  rs_load_tile(a0, ng, lo, hi, rs8, m, ctx8, k, c);
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) { uint32_t cg; f[j] = rs_map(c[j], m, &cg); }
  uint32_t gex, tile;
  rs_prefixes(f, m, wt, e, &gex, &tile);
  const uint32_t T = tstate[blockIdx.x], w = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {
    const uint32_t G = __shfl(gex, j * (REC_BT / 64) + w);
    uint32_t to;
    c[j] = c[j] ? rs_select(c[j], rs_apply(e[j], rs_apply(G, T)), m, &to) : 0u;
  }
  rs_rank_write(c, wt, wb, toff[blockIdx.x], lo, hi, base, nsep, tail, off);
}
