// kx_batch.inc — device side of batched runs (kx_run_batch, include/kxhip.h): many independent documents in one call.
// Included by kx_engine.hip behind the general engine's kernels; the host driver is kx_batch_host.inc.
//
// A document is a whole input: it starts in the initial state, must end in a final state, and its output begins with the
// initial closure's constant.  The kernels run the stage's PATH FORM (DevTables — the general engine's image; it exists for
// every stage, never escapes, and covers lookahead, symbol-table and regex-coder stages), with the compiler-scheduled piece
// forms of kx_engine.hip (piece_forward, walk_len) so that BIG stages (image in global memory) go through the same code.
//
//   k_bcheck    lane = document: offsets non-decreasing (else the call fails with KX_E_ARG before any other kernel runs);
//               the caller's result records are cleared
//   k_bforward  lane = document: state sequence from the start state, one checkpoint per 32 symbols, first dead step or a
//               non-final end state as fail_pos.  Documents longer than batch_doc_max, and every document of a stage with
//               register actions, are listed for the single-document route instead.
//   k_bback     lane = document: from fin_leaf of the end state, backward over its 64-symbol pieces (back rows re-derived
//               from the checkpoints, as k_backlen does): one record per piece {document, leaf at the piece's end, output
//               bytes behind the piece} and the document's length including the initial closure's constant
//   k_bscan_*   exclusive scan of the 64-bit document lengths (k_scan_groups in the middle)
//   k_binit     lane = document: the initial closure's constant
//   k_bemit     lane = piece: re-derive the piece, walk it backward from its recorded leaf and store its bytes straight to
//               global memory at their final, arbitrarily aligned place
//   k_bplace    workgroup = routed document: its output from the route's scratch to its place
//
// Per-document workspace needs no scan: document i (relative start r = off[i] - off[0]) owns checkpoint slots
// [r/32 + i, r/32 + i + n_i/32] and piece slots [r/64 + i, (r + n_i)/64 + i + 1) — floor(a) + floor(b) <= floor(a + b) keeps the
// ranges of consecutive documents apart.  Every slot of a document's piece range is written by k_bback (unused ones marked), so
// k_bemit can take the slots as its lanes without a memset.
//
// Framed batches (kx_run_batch_framed): k_bcheck / k_bforward / k_bback end in a parameter pack FR that is empty or one BFrame,
// and k_bemit has a twin, k_bemit_fr, that takes one.  The framed instances take document i of stage 0 as
// in[off[i], off[i+1] - trim) (one document may be left whole); the instances without a frame are the kernels of kx_run_batch.
// The slot bases above still come from the UNTRIMMED starts, so the ranges stay apart; a trimmed document may need one slot fewer
// than its range holds, which k_bback marks unused like any other.  bload_piece gets the trimmed end, so a lane still loads only
// the granules of its own (trimmed) document.  A suffix is no business of these kernels: BDoc::len stays the document's own
// output length, the scan adds the suffix to the length of every accepted document (k_bscan_*'s sfx), and k_bsuffix writes its
// bytes at the end of the document's output range.

constexpr uint32_t BATCH_BT = 512;     // threads per workgroup of the per-document kernels
constexpr uint32_t BATCH_NO_DOC = 0xFFFFFFFFu;
enum { BC_ROUTED = 0, BC_REJECTED = 1, BC_BADOFF = 2, BC_SHORT = 3, BC_N = 4 };

struct __attribute__((aligned(16))) BDoc { unsigned long long len; uint32_t endh; uint16_t mode; uint16_t l0; };   // mode: BM_*
enum { BM_RUN = 0, BM_SKIP = 1, BM_ROUTED = 2 };
struct __attribute__((aligned(8))) BRoute { unsigned long long start, len; uint32_t doc, rejected; unsigned long long fail; };
struct __attribute__((aligned(16))) BRec { uint32_t doc, leaf4; unsigned long long cum; };   // cum: output bytes of the steps behind the piece

// the frame of a stage's input: the last `trim` bytes of every document's range are not the document's, except for document `whole`
struct BFrame { unsigned long long trim, whole; };
constexpr unsigned long long BATCH_NO_WHOLE = ~0ull;
// the length of document i, whose range holds n bytes; fr: nothing, or the stage's BFrame
template <typename... FR>
__device__ __forceinline__ unsigned long long bdoc_len(unsigned long long n, unsigned long long i, const FR&... fr) {
  static_assert(sizeof...(FR) <= 1, "at most one frame");
  if constexpr (sizeof...(FR) != 0) {
    const BFrame& f = (fr, ...);
    return n - (i == f.whole ? 0ull : f.trim);
  } else return n;
}

__device__ __forceinline__ unsigned long long bchk_base(unsigned long long rel, unsigned long long i) { return (rel >> 5) + i; }
__device__ __forceinline__ unsigned long long bpiece_base(unsigned long long rel, unsigned long long i) { return (rel >> 6) + i; }
__device__ __forceinline__ uint32_t bstate_of(uint32_t h, const DevTables& T) { return ((h << T.hshift) - OFF_FWD) / (T.nclasses * 4); }

// The 64 bytes from p (any alignment) into w, read as aligned 16-byte words: a word is loaded only where it holds a byte
// below `end`, so nothing outside the document's own 16-byte granules is touched.  Bytes at or beyond `end` are garbage (the
// callers mask those steps).  Five words cover any misalignment; the byte shift is a word select plus v_alignbyte.
__device__ __forceinline__ void bload_piece(const uint8_t* p, const uint8_t* end, uint32_t (&w)[16]) {
  const uintptr_t a = (uintptr_t)p, a0 = a & ~(uintptr_t)15, e = (uintptr_t)end;
  uint32_t d[20];
#pragma unroll
  for (int g = 0; g < 5; ++g) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (a0 + 16u * g < e) v = *reinterpret_cast<const uint4*>(a0 + 16u * g);
    d[4 * g] = v.x; d[4 * g + 1] = v.y; d[4 * g + 2] = v.z; d[4 * g + 3] = v.w;
  }
  const uint32_t q = (uint32_t)(a >> 2) & 3u, r = (uint32_t)a & 3u;
  uint32_t x[17];
#pragma unroll
  for (int j = 0; j < 17; ++j) x[j] = q == 0 ? d[j] : q == 1 ? d[j + 1] : q == 2 ? d[j + 2] : d[j + 3];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = __builtin_amdgcn_alignbyte(x[i + 1], x[i], r);
}

template <typename... FR>
__global__ void k_bcheck(const unsigned long long* __restrict__ off, unsigned long long ndocs, kx_batch_doc* __restrict__ rec,
                         unsigned long long* __restrict__ ctr, FR... fr) {
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ndocs) return;
  if (off[i + 1] < off[i]) atomicOr(&ctr[BC_BADOFF], 1ull);
  else if constexpr (sizeof...(FR) != 0) {   // a range shorter than what is cut from it
    const BFrame& f = (fr, ...);
    if (i != f.whole && off[i + 1] - off[i] < f.trim) atomicOr(&ctr[BC_SHORT], 1ull);
  }
  rec[i] = kx_batch_doc{0, 0, 0};
}

template <bool WIDE, typename... FR>
__global__ __launch_bounds__(BATCH_BT) void k_bforward(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                       unsigned long long ndocs, unsigned long long doc_max, int route_all, uint32_t stage,
                                                       BDoc* __restrict__ docs, kx_batch_doc* __restrict__ rec, uint16_t* __restrict__ chk,
                                                       BRoute* __restrict__ routes, unsigned long long* __restrict__ ctr, DevTables T, FR... fr) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Lds L = stage_tables<WIDE>(T, smem);
  const unsigned long long o0 = off[0];
  const uint32_t dead = T.deadh;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < ndocs; i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long s = off[i], n = bdoc_len(off[i + 1] - s, i, fr...);
    BDoc d{0, 0, BM_RUN, 0};
    if (rec[i].status) { d.mode = BM_SKIP; docs[i] = d; continue; }   // rejected by an earlier stage: not run (not even as an empty document)
    if (route_all || n > doc_max) {
      d.mode = BM_ROUTED; docs[i] = d;
      const unsigned long long k = atomicAdd(&ctr[BC_ROUTED], 1ull);
      routes[k] = BRoute{s, n, (uint32_t)i, 0, 0};
      continue;
    }
    uint16_t* ck = chk + bchk_base(s - o0, i);
    const uint8_t* p = in + s;
    const uint8_t* e = p + n;
    uint32_t h = T.q0h;
    unsigned long long fail = NOFAIL;
    for (unsigned long long ps = 0; ps < n; ps += PIECE) {
      uint32_t w[16];
      bload_piece(p + ps, e, w);
      const uint32_t plen = n - ps < PIECE ? (uint32_t)(n - ps) : (uint32_t)PIECE;
      const uint32_t h0 = h;
      ck[ps >> 5] = (uint16_t)h;
      static_for<0, PIECE>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        if constexpr (t == HALF) { if (plen >= (uint32_t)HALF) ck[(ps >> 5) + 1] = (uint16_t)h; }
        const uint32_t nh = L.next(h, BYTE_AT_DEP(w, t, h)) & 0xFFFFu;
        h = (uint32_t)t < plen ? nh : h;
      });
      if (h == dead) {   // (the dead handle absorbs): find the first symbol without a transition
        h = h0;
        uint32_t k = 0;
        bool alive = true;
        static_for<0, PIECE>([&](auto tc) {
          constexpr int t = decltype(tc)::value;
          if (alive && (uint32_t)t < plen) {
            const uint32_t nh = L.next(h, BYTE_AT_DEP(w, t, h)) & 0xFFFFu;
            if (nh == dead) alive = false; else { h = nh; ++k; }
          }
        });
        fail = ps + k;
        break;
      }
    }
    if (fail == NOFAIL && T.fin_leaf[bstate_of(h, T)] == KXP_NO_LEAF) fail = n;   // ends in a state that is not final
    if (fail != NOFAIL) {
      rec[i] = kx_batch_doc{fail, 1u, stage};
      atomicAdd(&ctr[BC_REJECTED], 1ull);
      d.mode = BM_SKIP;
    } else d.endh = h;
    docs[i] = d;
  }
}

template <bool WIDE, typename... FR>
__global__ __launch_bounds__(BATCH_BT) void k_bback(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                    unsigned long long ndocs, BDoc* __restrict__ docs, const uint16_t* __restrict__ chk,
                                                    BRec* __restrict__ brec, DevTables T, FR... fr) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Lds L = stage_tables<WIDE>(T, smem);
  const unsigned long long o0 = off[0];
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < ndocs; i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long s = off[i], n = bdoc_len(off[i + 1] - s, i, fr...), rel = s - o0;
    const unsigned long long pb = bpiece_base(rel, i), pe = bpiece_base(off[i + 1] - o0, i + 1);
    BDoc d = docs[i];
    unsigned long long np = 0;
    if (d.mode == BM_RUN) {
      np = (n + PIECE - 1) / PIECE;
      const uint16_t* ck = chk + bchk_base(rel, i);
      const uint8_t* p = in + s;
      uint32_t leaf = (uint32_t)T.fin_leaf[bstate_of(d.endh, T)] * 4u;
      unsigned long long cum = 0;
      for (unsigned long long k = np; k-- > 0;) {
        const unsigned long long ps = k * PIECE;
        const int plen = n - ps < PIECE ? (int)(n - ps) : PIECE;
        uint32_t w[16], bo[BOW];
        bload_piece(p + ps, p + n, w);
        piece_forward(w, ck[2 * k], L, bo);
        mask_tail(bo, plen, T.nullrow);
        brec[pb + k] = BRec{(uint32_t)i, leaf, cum};
        cum += walk_len<WIDE>(bo, leaf, L, T);
      }
      d.l0 = (uint16_t)(leaf >> 2);
      d.len = cum + T.init_len[leaf >> 2];
      docs[i] = d;
    }
    for (unsigned long long k = pb + np; k < pe; ++k) brec[k].doc = BATCH_NO_DOC;   // (pe from the untrimmed end: a trimmed document's spare slot too)
  }
}

// the routed documents' results (host): length, or the rejection
__global__ void k_broute_set(uint32_t nr, const BRoute* __restrict__ res, uint32_t stage, BDoc* __restrict__ docs,
                             kx_batch_doc* __restrict__ rec, unsigned long long* __restrict__ ctr) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nr) return;
  const BRoute r = res[k];
  if (r.rejected) {
    rec[r.doc] = kx_batch_doc{r.fail, 1u, stage};
    docs[r.doc].len = 0;
    atomicAdd(&ctr[BC_REJECTED], 1ull);
  } else docs[r.doc].len = r.len;
}

// exclusive scan of the document lengths: per-workgroup sums, k_scan_groups, then inside each workgroup.  ooff[ndocs] = total.
// sfx != 0 (the last stage of a framed batch): every accepted document's length counts sfx more bytes, its suffix (BDoc::len itself stays)
__device__ __forceinline__ unsigned long long bscan_len(unsigned long long i, unsigned long long ndocs, const BDoc* __restrict__ docs,
                                                        const kx_batch_doc* __restrict__ rec, unsigned long long sfx) {
  if (i >= ndocs) return 0;
  unsigned long long v = docs[i].len;
  if (sfx && rec[i].status == 0) v += sfx;
  return v;
}

__global__ __launch_bounds__(1024) void k_bscan_reduce(unsigned long long ndocs, const BDoc* __restrict__ docs, unsigned long long* __restrict__ wsum,
                                                       const kx_batch_doc* __restrict__ rec, unsigned long long sfx) {
  __shared__ unsigned long long red[1024];
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  red[threadIdx.x] = bscan_len(i, ndocs, docs, rec, sfx);
  __syncthreads();
  for (uint32_t s = blockDim.x >> 1; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) wsum[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(1024) void k_bscan_down(unsigned long long ndocs, const BDoc* __restrict__ docs, const unsigned long long* __restrict__ woff,
                                                     const Flags* __restrict__ flags, unsigned long long* __restrict__ ooff,
                                                     const kx_batch_doc* __restrict__ rec, unsigned long long sfx) {
  __shared__ unsigned long long buf[1024];
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long v = bscan_len(i, ndocs, docs, rec, sfx);
  buf[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t d = 1; d < blockDim.x; d <<= 1) {
    const unsigned long long x = threadIdx.x >= d ? buf[threadIdx.x - d] : 0;
    __syncthreads();
    buf[threadIdx.x] += x;
    __syncthreads();
  }
  if (i < ndocs) ooff[i] = woff[blockIdx.x] + buf[threadIdx.x] - v;
  else if (i == ndocs) ooff[i] = flags->total_len;
}

__global__ void k_binit(unsigned long long ndocs, const BDoc* __restrict__ docs, const unsigned long long* __restrict__ ooff,
                        uint8_t* __restrict__ out, DevTables T) {
  const uint8_t* pool = reinterpret_cast<const uint8_t*>(T.packed) + T.off_pool;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < ndocs; i += (unsigned long long)gridDim.x * blockDim.x) {
    const BDoc d = docs[i];
    if (d.mode != BM_RUN) continue;
    const uint32_t nb = T.init_len[d.l0], src = T.init_off[d.l0];
    uint8_t* o = out + ooff[i];
    for (uint32_t j = 0; j < nb; ++j) o[j] = pool[src + j];
  }
}

// One step of the placing walk, straight to global memory: the step's bytes are [copied symbol][constant] and end at o.
template <int T_, bool WIDE>
__device__ __forceinline__ void bemit_step(const uint32_t (&bo)[BOW], const uint32_t (&w)[16], uint32_t& leaf, uint8_t*& o,
                                           const Lds& L, const DevTables& T) {
  const uint32_t a = L.ra(BO_GET_DEP(bo, T_, leaf)) + leaf;
  const uint32_t e = L.w(a);
  leaf = E_LEAF4(e);
  const uint32_t dl = ent_dlen<WIDE>(e, a, L, T);
  if (dl == 0) return;
  o -= dl;
  const uint32_t cp = E_COPY(e), cl = dl - cp;
  if (cp) o[0] = (uint8_t)ent_sym<WIDE>(e, BYTE_AT_DEP(w, T_, e), L, T);
  if (cl == 0) return;
  if (!WIDE && T.inl && !(e & 0x8000u)) { o[cp] = (uint8_t)(e >> 16); return; }   // inline-constant layout: the byte rides in the entry
  uint32_t src;
  if (WIDE) src = ent_off<true>(e, a, L, T);
  else if (T.jl) src = ent_off<false, false, true>(e, a, L, T);
  else if (T.inl) src = ent_off<false, true>(e, a, L, T);
  else src = ent_off<false>(e, a, L, T);
  for (uint32_t j = 0; j < cl; ++j) o[cp + j] = L.pb(src + j);
}

template <bool WIDE>
__global__ __launch_bounds__(BATCH_BT) void k_bemit(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                    unsigned long long nslots, const BDoc* __restrict__ docs, const uint16_t* __restrict__ chk,
                                                    const BRec* __restrict__ brec, const unsigned long long* __restrict__ ooff,
                                                    uint8_t* __restrict__ out, DevTables T) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Lds L = stage_tables<WIDE>(T, smem);
  const unsigned long long o0 = off[0];
  for (unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; j < nslots; j += (unsigned long long)gridDim.x * blockDim.x) {
    const BRec r = brec[j];
    if (r.doc == BATCH_NO_DOC) continue;
    const unsigned long long i = r.doc, s = off[i], n = off[i + 1] - s, rel = s - o0;
    const unsigned long long k = j - bpiece_base(rel, i), ps = k * PIECE;
    const int plen = n - ps < PIECE ? (int)(n - ps) : PIECE;
    uint32_t w[16], bo[BOW];
    bload_piece(in + s + ps, in + s + n, w);
    piece_forward(w, chk[bchk_base(rel, i) + 2 * k], L, bo);
    mask_tail(bo, plen, T.nullrow);
    if (T.xlat) xlat_piece(w, L.base + T.xlat);   // one symbol table on every copying entry: translate the piece once
    uint8_t* o = out + ooff[i] + docs[i].len - r.cum;
    uint32_t leaf = r.leaf4;
    static_for<0, PIECE>([&](auto tc) { bemit_step<PIECE - 1 - decltype(tc)::value, WIDE>(bo, w, leaf, o, L, T); });
  }
}

// k_bemit for stage 0 of a framed batch: k_bemit's body with the trimmed length — KEEP THE TWO IN STEP, a change to one is a
// change to both.  Two kernels and not one shared inline body: with a shared body the register allocation of k_bemit<true>
// differs from the one DESIGN.md §2h records (123 VGPRs / 63 SGPRs, not 121 / 65).
template <bool WIDE, typename... FR>
__global__ __launch_bounds__(BATCH_BT) void k_bemit_fr(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                    unsigned long long nslots, const BDoc* __restrict__ docs, const uint16_t* __restrict__ chk,
                                                    const BRec* __restrict__ brec, const unsigned long long* __restrict__ ooff,
                                                    uint8_t* __restrict__ out, DevTables T, FR... fr) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Lds L = stage_tables<WIDE>(T, smem);
  const unsigned long long o0 = off[0];
  for (unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; j < nslots; j += (unsigned long long)gridDim.x * blockDim.x) {
    const BRec r = brec[j];
    if (r.doc == BATCH_NO_DOC) continue;
    const unsigned long long i = r.doc, s = off[i], n = bdoc_len(off[i + 1] - s, i, fr...), rel = s - o0;
    const unsigned long long k = j - bpiece_base(rel, i), ps = k * PIECE;
    const int plen = n - ps < PIECE ? (int)(n - ps) : PIECE;
    uint32_t w[16], bo[BOW];
    bload_piece(in + s + ps, in + s + n, w);
    piece_forward(w, chk[bchk_base(rel, i) + 2 * k], L, bo);
    mask_tail(bo, plen, T.nullrow);
    if (T.xlat) xlat_piece(w, L.base + T.xlat);   // one symbol table on every copying entry: translate the piece once
    uint8_t* o = out + ooff[i] + docs[i].len - r.cum;
    uint32_t leaf = r.leaf4;
    static_for<0, PIECE>([&](auto tc) { bemit_step<PIECE - 1 - decltype(tc)::value, WIDE>(bo, w, leaf, o, L, T); });
  }
}

// workgroup = routed document: its output (at src in the route's scratch) to its place
__global__ void k_bplace(const BRoute* __restrict__ res, const uint8_t* __restrict__ scratch, const unsigned long long* __restrict__ ooff,
                         uint8_t* __restrict__ out) {
  const BRoute r = res[blockIdx.x];
  if (r.rejected || r.len == 0) return;
  uint8_t* d = out + ooff[r.doc];
  const uint8_t* sp = scratch + r.start;
  for (unsigned long long k = threadIdx.x; k < r.len; k += blockDim.x) d[k] = sp[k];
}

// lane = document: the suffix of an accepted document, the last `len` (1 to 8) bytes of its output range (any alignment).  The scan
// gave every accepted document those bytes, so the stores stay inside the document's own range.  Every kernel that places
// output (k_bemit, k_bplace, the batch replay) stops where the document's own bytes end, so its order against them is free.
__global__ void k_bsuffix(unsigned long long ndocs, const kx_batch_doc* __restrict__ rec, const unsigned long long* __restrict__ ooff,
                          uint8_t* __restrict__ out, unsigned long long sfx8, uint32_t len) {
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ndocs || rec[i].status) return;
  const unsigned long long b = ooff[i], e = ooff[i + 1];
  if (e - b < len) return;   // (never: the scan counted the suffix)
  uint8_t* o = out + e - len;
  for (uint32_t j = 0; j < len; ++j) o[j] = (uint8_t)(sfx8 >> (8 * j));
}

// ---------------------------------------------------------------------------- host-side workspace of kx_run_batch
// grow-only device buffers of one program's batched runs (kx_program::batch; freed by kx_free)
struct BatchWs {
  struct Buf { void* p = nullptr; size_t cap = 0; };
  Buf chk, brec, docs, routes, ctr, flags, wsum, woff, vals[2], offs[2], rin, rout, tok, tokout, rres;
  Buf actr, atok, atoff, atab, awlist, adeep, aretry, astates, ascr, aheap;   // the batch replay of action stages (kx_batch_actions.inc)
  hipEvent_t ev[10] = {};
  bool have_events = false, lds_set = false;
  static int ensure(Buf& b, size_t bytes) {   // contents are not kept
    if (b.cap >= bytes) return 0;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
    const size_t want = bytes + bytes / 8 + 4096;
    HIPCHECK(hipMalloc(&b.p, want));
    b.cap = want;
    return 0;
  }
  static int grow(Buf& b, size_t used, size_t bytes, hipStream_t sm) {   // contents [0, used) are kept
    if (b.cap >= bytes) return 0;
    const size_t want = bytes > 2 * b.cap ? bytes + 4096 : 2 * b.cap;
    void* nb = nullptr;
    HIPCHECK(hipMalloc(&nb, want));
    if (used) { HIPCHECK(hipMemcpyAsync(nb, b.p, used, hipMemcpyDeviceToDevice, sm)); HIPCHECK(hipStreamSynchronize(sm)); }
    if (b.p) (void)hipFree(b.p);
    b.p = nb; b.cap = want;
    return 0;
  }
  ~BatchWs() {
    for (Buf* b : {&chk, &brec, &docs, &routes, &ctr, &flags, &wsum, &woff, &vals[0], &vals[1], &offs[0], &offs[1], &rin, &rout, &tok, &tokout, &rres,
                   &actr, &atok, &atoff, &atab, &awlist, &adeep, &aretry, &astates, &ascr, &aheap})
      if (b->p) (void)hipFree(b->p);
    if (have_events) for (auto& e : ev) (void)hipEventDestroy(e);
  }
};
