// kx_batch_actions.inc — batched runs, stages with register actions: the token streams of a whole batch replayed on the device,
// one document per lane or per wave (kx_config::batch_actions = 2; DESIGN.md §2h "batch replay").  Included by kx_engine.hip
// behind kx_batch.inc; the host side is in kx_batch_host.inc.
//
// Such a stage first runs like any other (k_bforward … k_bemit) into a workspace batch that holds every document's TOKEN STREAM
// (kxp_format.h).  Every document starts from the empty state by contract, so the document boundaries are the safe points the
// single-stream post-pass has to search for, and a document's replayed output is never longer than its token stream:
//
//   k_bact_measure  lane = document: the replay with numbers only — the length of the bottom buffer, of the open frames and of
//                   every register; no byte is moved.  The length goes into the document's BDoc (the ordinary scan then gives
//                   the stage's real out_off), and the document is classed: LANE (registers below LANE_REGS, depth at most
//                   LANE_DEPTH, at most BACT_LANE_MAX bytes of tokens), WAVE (the rest, listed through an atomic counter), or
//                   DEEP (a Push at depth 64: the single-document route reports that error, and so it is left to it)
//   k_bact_lanes    lane = document of class LANE: act_lane_replay (the interpreter of k_actions_lanes), the bottom buffer
//                   straight to dst + out_off[i]
//   k_bact_waves    wave = document of class WAVE: actions_body on a fresh ActState, a persistent grid over the list
//
// Frames and registers that leave the VGPRs / LDS live in the document's own stretch of two arenas, addressed from the token
// stream's offsets as k_actions_lanes addresses its chunks (t + 64 i and 2 t + 1024 i for document i at token offset t): no scan.
// A document whose registers outgrow that stretch (the bump allocation never frees) is listed for the single-document route
// after all (BA_RETRY); its measured length stays valid, so nothing else moves.
//
// End of a document = end of the single-document replay (ActionRunner::run_seq, which decides wherever this text and it
// disagree): the output is the bottom buffer; registers still full and frames still open are dropped; a token cut by the end
// ends the replay; Pop at depth 0 and registers >= act_regs are ignored.

enum { BM_ACT_LANE = 3, BM_ACT_WAVE = 4 };                     // BDoc::mode of a measured document (behind BM_*)
enum { BA_WAVES = 0, BA_WNEXT = 1, BA_RETRY = 2, BA_DEEP = 3, BA_REPLAY = 4, BA_N = 8 };   // the replay's counters (BatchWs::actr)
constexpr uint32_t BACT_MT = 256;            // threads per workgroup of k_bact_measure / k_bact_lanes
constexpr uint32_t BACT_LANE_MAX = 4096;     // token bytes up to which a document is replayed by a lane (a wave lasts as long as its longest lane)
constexpr uint32_t BACT_TAB_FRAMES = 64 - LANE_DEPTH;   // k_bact_measure's per-thread table: frames 8..63, then registers 8..nregs-1

__device__ __forceinline__ uint8_t* bact_scratch(uint8_t* scratch, unsigned long long t, unsigned long long i) { return scratch + t + 64ull * i; }
__device__ __forceinline__ uint8_t* bact_heap(uint8_t* heap, unsigned long long t, unsigned long long i) { return heap + 2 * t + 1024ull * i; }

// `list[k] = v` for the lanes with `take`, k from one atomic per wave (all lanes of the wave that are still in the loop call it)
__device__ __forceinline__ void bact_append(bool take, unsigned long long* counter, uint32_t* list, uint32_t v) {
  const unsigned long long m = __ballot(take);
  if (!m) return;
  const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__builtin_ctzll(m);
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(counter, (unsigned long long)__builtin_popcountll(m));
  base = __shfl(base, (int)leader);
  if (take) list[base + (unsigned long long)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = v;
}

// lane_mode: kx_config::act_lanes (0 auto, 1 no lanes, 2 lanes wherever the interpreter's limits allow)
__global__ __launch_bounds__(BACT_MT) void k_bact_measure(const uint8_t* __restrict__ tok, const unsigned long long* __restrict__ toff,
                                                          unsigned long long ndocs, uint32_t nregs, uint32_t lane_mode, BDoc* __restrict__ docs,
                                                          uint32_t* __restrict__ tab, uint32_t* __restrict__ wlist, uint32_t* __restrict__ deep,
                                                          unsigned long long* __restrict__ ctr) {
  const unsigned long long nth = (unsigned long long)gridDim.x * blockDim.x, tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t* ftab = tab + tid;                                        // frame k (k >= LANE_DEPTH): ftab[(k - LANE_DEPTH) * nth]
  uint32_t* rtab = tab + (unsigned long long)BACT_TAB_FRAMES * nth + tid;   // register r (r >= LANE_REGS): rtab[(r - LANE_REGS) * nth]
  for (unsigned long long i = tid; i < ndocs; i += nth) {
    BDoc d = docs[i];
    bool is_wave = false, is_deep = false;
    if (d.mode == BM_RUN) {
      const unsigned long long t0 = toff[i], n = toff[i + 1] - t0;
      const uint8_t* src = tok + t0;
      // st[k]: the length of the buffer BELOW frame k + 1 while that frame is open (st[0]: the bottom buffer); cur: the top buffer
      uint32_t st[LANE_DEPTH], rl[LANE_REGS];
#pragma unroll
      for (uint32_t q = 0; q < LANE_DEPTH; ++q) st[q] = 0;
#pragma unroll
      for (uint32_t q = 0; q < LANE_REGS; ++q) rl[q] = 0;
      for (uint32_t r = LANE_REGS; r < nregs; ++r) rtab[(unsigned long long)(r - LANE_REGS) * nth] = 0;
      uint32_t cur = 0, depth = 0, maxdepth = 0;
      bool bigreg = false;
      is_deep = (n >> 32) != 0;   // (lengths are 32-bit numbers here; such a stream is not a batch document)
      unsigned long long pos = 0;
      Win8 W;
      while (pos < n && !is_deep) {
        uint32_t r = 0, run = 0; unsigned long long w;
        const uint32_t k = act_token_w(W, src, n, pos, r, run, w);
        if (k == 0) { cur += run; continue; }
        if (k == 4) break;
        if (k == 1) {
          if (depth >= 64) { is_deep = true; break; }
          if (depth < LANE_DEPTH) {
#pragma unroll
            for (uint32_t q = 0; q < LANE_DEPTH; ++q) if (q == depth) st[q] = cur;
          } else ftab[(unsigned long long)(depth - LANE_DEPTH) * nth] = cur;
          cur = 0; depth += 1;
          maxdepth = depth > maxdepth ? depth : maxdepth;
          continue;
        }
        if (r >= nregs) continue;
        bigreg |= r >= LANE_REGS;
        if (k == 2) {   // Pop: the top buffer becomes the register, the buffer below is the top again
          if (depth == 0) continue;
          if (r < LANE_REGS) {
#pragma unroll
            for (uint32_t q = 0; q < LANE_REGS; ++q) if (q == r) rl[q] = cur;
          } else rtab[(unsigned long long)(r - LANE_REGS) * nth] = cur;
          depth -= 1;
          if (depth < LANE_DEPTH) {
#pragma unroll
            for (uint32_t q = 0; q < LANE_DEPTH; ++q) if (q == depth) cur = st[q];
          } else cur = ftab[(unsigned long long)(depth - LANE_DEPTH) * nth];
        } else {        // Write: the register onto the top buffer; it is empty afterwards
          if (r < LANE_REGS) {
#pragma unroll
            for (uint32_t q = 0; q < LANE_REGS; ++q) if (q == r) { cur += rl[q]; rl[q] = 0; }
          } else { cur += rtab[(unsigned long long)(r - LANE_REGS) * nth]; rtab[(unsigned long long)(r - LANE_REGS) * nth] = 0; }
        }
      }
      d.len = depth == 0 ? cur : st[0];   // frames still open are dropped
      if (is_deep) { d.len = 0; d.mode = BM_ROUTED; }
      else {
        const bool lane_ok = !bigreg && maxdepth <= LANE_DEPTH && lane_mode != 1 && (lane_mode == 2 || n <= BACT_LANE_MAX);
        d.mode = lane_ok ? BM_ACT_LANE : BM_ACT_WAVE;
        is_wave = !lane_ok;
      }
      docs[i] = d;
    }
    const unsigned long long measured = __ballot(is_wave || d.mode == BM_ACT_LANE);
    if (measured && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(measured)) atomicAdd(&ctr[BA_REPLAY], (unsigned long long)__builtin_popcountll(measured));
    bact_append(is_wave, &ctr[BA_WAVES], wlist, (uint32_t)i);
    bact_append(is_deep, &ctr[BA_DEEP], deep, (uint32_t)i);
  }
}

__global__ __launch_bounds__(BACT_MT) void k_bact_lanes(const uint8_t* __restrict__ tok, const unsigned long long* __restrict__ toff,
                                                        unsigned long long ndocs, uint32_t nregs, const BDoc* __restrict__ docs,
                                                        const unsigned long long* __restrict__ ooff, uint8_t* scratch, uint8_t* heap,
                                                        uint8_t* __restrict__ out, uint32_t* __restrict__ retry, unsigned long long* __restrict__ ctr) {
  const unsigned long long nth = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < ndocs; i += nth) {
    const BDoc d = docs[i];
    bool failed = false;
    if (d.mode == BM_ACT_LANE) {
      const unsigned long long t0 = toff[i];
      uint32_t olen, depth;
      const uint32_t status = act_lane_replay<true>(tok + t0, (uint32_t)(toff[i + 1] - t0), bact_scratch(scratch, t0, i), bact_heap(heap, t0, i),
                                                    out + ooff[i], (uint32_t)d.len, nregs, olen, depth);
      // (4: a token cut by the document's end ends the replay; frames still open are dropped)
      failed = (status != 0 && status != 4) || olen != (uint32_t)d.len;
    }
    bact_append(failed, &ctr[BA_RETRY], retry, (uint32_t)i);
  }
}

template <uint32_t BUF, uint32_t NR>
__global__ __launch_bounds__(64) void k_bact_waves(const uint8_t* __restrict__ tok, const unsigned long long* __restrict__ toff, uint32_t nregs,
                                                   const BDoc* __restrict__ docs, const unsigned long long* __restrict__ ooff,
                                                   const uint32_t* __restrict__ wlist, ActState* states, uint8_t* scratch, uint8_t* heap,
                                                   uint8_t* out, uint32_t* __restrict__ retry, unsigned long long* __restrict__ ctr) {
  ActState* st = states + blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const unsigned long long nw = ctr[BA_WAVES];
  for (;;) {
    unsigned long long k = 0;
    if (lane == 0) k = atomicAdd(&ctr[BA_WNEXT], 1ull);
    k = __shfl(k, 0);
    if (k >= nw) break;
    const unsigned long long i = wlist[k], t0 = toff[i], n = toff[i + 1] - t0;
    // a fresh state: empty stack, empty registers, the document's own stretch of the arenas
    st->frame_start[lane] = 0;
    for (uint32_t r = lane; r < NR; r += 64) st->reg[r] = ActReg{0, 0, 0};
    if (lane == 0) {
      st->scratch_len = 0; st->scratch_cap = n + 64; st->heap_len = 0; st->heap_cap = 2 * n + 1024;
      st->consumed = 0; st->out_len = 0; st->depth = 0; st->status = 0; st->carry_n = 0;
    }
    __threadfence();
    __syncthreads();
    actions_body<BUF, NR>(tok + t0, n, st, bact_scratch(scratch, t0, i), bact_heap(heap, t0, i), out + ooff[i], nregs);
    __threadfence();
    __syncthreads();
    // (a token cut by the end stays in the carry and is dropped; so are open frames and full registers)
    if (lane == 0 && (st->status != 0 || st->out_len != docs[i].len)) retry[atomicAdd(&ctr[BA_RETRY], 1ull)] = (uint32_t)i;
    __syncthreads();
  }
}
