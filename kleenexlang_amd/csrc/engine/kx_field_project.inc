// kx_field_project.inc — device side of the projection of field mode (include/kxhip.h: kx_run_batch_field_project,
// kx_run_records_fd_field_project; `--only`): an accepted record writes the outputs of its selected fields, item by item as the
// list was written and joined by OFS, and no other byte of its body.  Included by kx_engine.hip behind kx_field_list.inc and the
// two files that share its driver; the host side is kx_field_project_host.inc.
//
// Everything up to the outputs is the list's (kx_field_list.inc): the documents of S, the union of the items, the inner batch and
// with a codec the spellings, whose field separator is then OFS.  The projection is another last step over the same arrays:
//   k_fpsplen   lane = record: status, fail_field and the rejected-record counter as k_flsplen (fl_status); an accepted record's
//               length = its items' (two scanned offsets each) + OFS between them + the kept separator + the suffix
//   the scan, into the caller's output offsets
//   k_fpsplice  lane = aligned 16-byte granule of the OUTPUT: the record by a search in the output offsets, the item by a walk of
//               the at most 16 items, the output inside the item by a search; from there a cursor
// The two lane bodies are kx_field_lanes.h's fp_splen_lane and fp_splice_lane, which a host program runs as they are; the kernels
// are the grid-stride loops around them.  No byte of `in` is read but a kept separator's; every output byte is written exactly
// once, nothing at or behind the total.

__global__ __launch_bounds__(FLD_BT) void k_fpsplen(const unsigned long long* __restrict__ off, unsigned long long n, FPSpec P,
                                                    const unsigned long long* __restrict__ d0, const unsigned long long* __restrict__ nf,
                                                    const unsigned long long* __restrict__ poff, const kx_batch_doc* __restrict__ drec,
                                                    kx_batch_doc* __restrict__ rec, uint32_t* __restrict__ fail_field, BDoc* __restrict__ len,
                                                    unsigned long long* __restrict__ ctr) {
  // (the loop's bound is the workgroup's, so that whole waves take each step and one lane adds a wave's rejected records)
  for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < n; base += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long i = base + threadIdx.x;
    bool rejected = false;
    if (i < n) {
      kx_batch_doc r;
      unsigned long long K;
      BDoc d{fp_splen_lane(P, off, i, d0, nf, poff, drec, &r, &K), 0, BM_RUN, 0};
      rejected = r.status != 0;
      rec[i] = r;
      if (fail_field) fail_field[i] = (uint32_t)K;
      len[i] = d;
    }
    const unsigned long long bal = __ballot(rejected);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&ctr[FC_REJECTED], (unsigned long long)__popcll(bal));
  }
}

__global__ __launch_bounds__(FLD_GT) void k_fpsplice(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off,
                                                     unsigned long long n, FPSpec P, const unsigned long long* __restrict__ d0,
                                                     const uint8_t* __restrict__ pout, const unsigned long long* __restrict__ poff,
                                                     const unsigned long long* __restrict__ ooff, unsigned long long total,
                                                     uint8_t* __restrict__ out) {
  const unsigned long long ng = ((unsigned long long)((uintptr_t)out & 15) + total + 15) >> 4;
  for (unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += (unsigned long long)gridDim.x * blockDim.x)
    fp_splice_lane(P, in, off, n, d0, pout, poff, ooff, total, out, g);
}
