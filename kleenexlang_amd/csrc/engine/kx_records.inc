// kx_records.inc — device side of record mode (include/kxhip.h: kx_split_records, kx_run_records_fd): cut a buffer into
// records after every separator byte.  Included by kx_engine.hip behind kx_batch.inc; the host side is kx_records_host.inc.
//
// A stream compaction over the aligned 16-byte granules that hold a byte of the buffer [in, in + n) — the granules of
// a0 = in & ~15 up to the one holding in[n - 1]; no other byte is read (the rule of bload_piece).  A tile is REC_G granules per
// thread of one workgroup, thread t of step j taking granule j * REC_BT + t, so every load instruction is 1 KiB contiguous per wave.
//   k_rcount  workgroup = tile: separators of the tile (exact zero-byte test of x ^ sep·0x01010101, popcount)
//   k_scan_groups (kx_engine.hip): exclusive scan of the tile counts; Flags::total_len = all separators
//   k_rwrite  workgroup = tile: the same test again; the rank of each granule's first separator inside the tile is the in-wave
//             prefix (bit-sliced: five ballots + mbcnt, counts are ≤ 16) plus the prefix of the (step, wave) totals (LDS, one wave
//             scans 64 entries); each separator at relative byte r writes off[1 + rank] = base + r + 1
// Bytes read: 2 n; bytes written: 8 per record.

constexpr uint32_t REC_BT = 256;                          // threads per workgroup
constexpr uint32_t REC_G = 16;                            // granules per thread and tile
constexpr uint32_t REC_TILE = REC_BT * REC_G;             // granules per tile (64 KiB)

// bytes [a, b) of a dword (0 ≤ a, b ≤ 4) as their high bits
__device__ __forceinline__ uint32_t rec_byte_span(long long a, long long b) {
  a = a < 0 ? 0 : a > 4 ? 4 : a;
  b = b < 0 ? 0 : b > 4 ? 4 : b;
  if (b <= a) return 0u;
  const uint32_t hi = b == 4 ? 0xFFFFFFFFu : (1u << (8 * b)) - 1u;
  return 0x80808080u & hi & ~((1u << (8 * a)) - 1u);
}

// Granule g of a0: the high bit of every byte equal to the separator (pat = sep · 0x01010101), bytes outside [lo, hi) — offsets
// from a0 — cleared.  The exact test: ((x & 0x7F..) + 0x7F..) sets a byte's high bit iff its low seven bits are not all zero; or-ing
// x adds the byte's own high bit; what stays clear is a zero byte, with no borrow from its neighbours (the haszero trick has one).
__device__ __forceinline__ uint4 rec_match(const uint8_t* __restrict__ a0, unsigned long long g, unsigned long long lo,
                                           unsigned long long hi, uint32_t pat) {
  const uint4 v = *reinterpret_cast<const uint4*>(a0 + 16ull * g);
  uint32_t m[4] = {v.x ^ pat, v.y ^ pat, v.z ^ pat, v.w ^ pat};
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = ~(((m[k] & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | m[k] | 0x7F7F7F7Fu);
  const unsigned long long o = 16ull * g;
  if (o < lo || o + 16 > hi) {   // (the first and the last granule only)
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] &= rec_byte_span((long long)lo - (long long)(o + 4 * k), (long long)hi - (long long)(o + 4 * k));
  }
  return make_uint4(m[0], m[1], m[2], m[3]);
}

__device__ __forceinline__ uint32_t rec_popc(const uint4 m) {
  return (uint32_t)(__popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w));
}

// the tile's matches into m[]; a full tile loads without a bounds test so that all REC_G loads are in flight together
__device__ __forceinline__ void rec_load_tile(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo,
                                              unsigned long long hi, uint32_t pat, uint4 (&m)[REC_G]) {
  const unsigned long long g0 = (unsigned long long)blockIdx.x * REC_TILE + threadIdx.x;
  if ((unsigned long long)(blockIdx.x + 1) * REC_TILE <= ng) {
#pragma unroll
    for (uint32_t j = 0; j < REC_G; ++j) m[j] = rec_match(a0, g0 + j * REC_BT, lo, hi, pat);
  } else {
#pragma unroll
    for (uint32_t j = 0; j < REC_G; ++j) {
      const unsigned long long g = g0 + j * REC_BT;
      m[j] = g < ng ? rec_match(a0, g, lo, hi, pat) : make_uint4(0, 0, 0, 0);
    }
  }
}

__global__ __launch_bounds__(REC_BT) void k_rcount(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo,
                                                   unsigned long long hi, uint32_t pat, unsigned long long* __restrict__ tcount) {
  __shared__ uint32_t red[REC_BT / 64];
  uint4 m[REC_G];
  rec_load_tile(a0, ng, lo, hi, pat, m);
  uint32_t c = 0;
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) c += rec_popc(m[j]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (uint32_t w = 0; w < REC_BT / 64; ++w) s += red[w];
    tcount[blockIdx.x] = s;
  }
}

// tail: the buffer does not end in a separator — off[nsep + 1] = base + n closes the last record
__global__ __launch_bounds__(REC_BT) void k_rwrite(const uint8_t* __restrict__ a0, unsigned long long ng, unsigned long long lo,
                                                   unsigned long long hi, uint32_t pat, const unsigned long long* __restrict__ toff,
                                                   unsigned long long base, unsigned long long nsep, int tail,
                                                   unsigned long long* __restrict__ off) {
  __shared__ uint32_t wt[REC_G * (REC_BT / 64)], wb[REC_G * (REC_BT / 64)];
  static_assert(REC_G * (REC_BT / 64) == 64, "one wave scans the (step, wave) totals");
  uint4 m[REC_G];
  rec_load_tile(a0, ng, lo, hi, pat, m);
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t pre[REC_G];
#pragma unroll
  for (uint32_t j = 0; j < REC_G; ++j) {   // in-wave exclusive prefix of the granule counts, five bits at a time
    const uint32_t c = rec_popc(m[j]);
    uint32_t p = 0, t = 0;
#pragma unroll
    for (int b = 0; b < 5; ++b) {
      const unsigned long long bal = __ballot((c >> b) & 1u);
      p += __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u)) << b;
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
    const uint32_t mk[4] = {m[j].x, m[j].y, m[j].z, m[j].w};
    if (!(mk[0] | mk[1] | mk[2] | mk[3])) continue;
    unsigned long long r = tb + wb[j * (REC_BT / 64) + w] + pre[j];
    const unsigned long long rel = 16ull * (g0 + j * REC_BT) - lo;   // (relative offset of the granule's byte 0; lo ≤ its first match)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      for (uint32_t x = mk[k]; x; x &= x - 1) off[1 + r++] = base + rel + 4 * k + (__builtin_ctz(x) >> 3) + 1;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    off[0] = base;
    if (tail) off[nsep + 1] = base + (hi - lo);
  }
}

// longest record of offsets off[0 .. n]: atomicMax into *best
__global__ void k_rlongest(const unsigned long long* __restrict__ off, unsigned long long n, unsigned long long* __restrict__ best) {
  unsigned long long mx = 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long l = off[i + 1] - off[i];
    mx = l > mx ? l : mx;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) { const unsigned long long x = __shfl_xor(mx, d); mx = x > mx ? x : mx; }
  if ((threadIdx.x & 63) == 0 && mx) atomicMax(best, mx);
}
