// stage_fuzz.cpp — corrupt and truncated blobs through the whole host-only stage builder (kx_stage.h), as a stand-alone program so
// that it can be built with -fsanitize=address,undefined: a bad index that the checks let through shows as a sanitizer report, not
// as luck.  The mutations are those of tests/test_abi.py::test_corrupt_and_truncated_blobs_are_refused_not_read_out_of_bounds.
//   stage_fuzz BLOB      exit 0 iff every call returned 0 or an error code (and the intact blob returned 0)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <random>

#include "../../kleenexlang_amd/csrc/engine/kx_stage.h"

namespace {

size_t g_calls = 0, g_refused = 0;

// every stage of the blob through buildStage, from a heap copy of exactly `len` bytes (a read past the end is a report)
int build(const uint8_t* blob, size_t len) {
  uint8_t* copy = (uint8_t*)malloc(len ? len : 1);
  memcpy(copy, blob, len);
  std::string err;
  const uint8_t* c = nullptr; uint32_t ns = 0;
  int rc = kxst::readBlobHeader(copy, len, &c, &ns, err);
  for (uint32_t s = 0; s < ns && !rc; ++s) {
    kxst::HostStage S;
    rc = kxst::buildStage(c, copy + len, kx_config{}, kxst::WITH_ALT | kxst::WITH_DELAYED, S, err);
  }
  free(copy);
  ++g_calls; g_refused += rc != 0;
  if (rc != 0 && rc != KX_E_BLOB && rc != KX_E_ARG) { fprintf(stderr, "unexpected return value %d\n", rc); exit(2); }
  return rc;
}
uint32_t u32At(const std::vector<uint8_t>& b, size_t off) { uint32_t v; memcpy(&v, &b[off], 4); return v; }
int withByte(std::vector<uint8_t> b, size_t off, uint8_t v) { b[off] = v; return build(b.data(), b.size()); }
int withWord(std::vector<uint8_t> b, size_t off, uint32_t v) { memcpy(&b[off], &v, 4); return build(b.data(), b.size()); }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: stage_fuzz BLOB\n"); return 2; }
  std::ifstream f(argv[1], std::ios::binary);
  const std::vector<uint8_t> blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (blob.size() < 20 || build(blob.data(), blob.size()) != 0) { fprintf(stderr, "%s: the intact blob is refused\n", argv[1]); return 1; }
  // truncations: every length below 200, then every (len / 400)-th
  const size_t step = blob.size() / 400 ? blob.size() / 400 : 1;
  for (size_t cut = 0; cut + 1 < blob.size(); cut += cut < 200 ? 1 : step)
    if (build(blob.data(), cut) == 0) { fprintf(stderr, "a blob cut to %zu bytes is accepted\n", cut); return 1; }
  // 1500 seeded 32-bit mutations: three in ten in the first stage's header words, the rest anywhere behind the blob header
  const size_t hdr = 20 + kxst::pad4(u32At(blob, 16));
  std::mt19937 r(7);
  for (int i = 0; i < 1500; ++i) {
    const size_t off = hdr + (r() % 10 < 3 ? (r() % 16) * 4 : (r() % (blob.size() - hdr - 4)) & ~(size_t)3);
    const uint32_t values[4] = {0xFFFFFFFFu, 0x7FFFFFFFu, 0x10000u, (uint32_t)r()};
    withWord(blob, off, values[r() % 4]);
  }
  // single bytes the 32-bit mutations do not reach: a byte class beyond the class count, a state without leaves, a final leaf
  // beyond the state's leaves, the table field of a back entry
  kxst::StageView v; std::string err;
  const uint8_t* c = blob.data() + hdr;
  if (kxst::readStage(c, blob.data() + blob.size(), v, err)) return 1;
  auto at = [&](const void* p) { return (size_t)((const uint8_t*)p - blob.data()); };
  if (withByte(blob, at(v.cls) + 'z', (uint8_t)v.C) == 0 && v.C < 256) { fprintf(stderr, "a byte class beyond the class count is accepted\n"); return 1; }
  if (withByte(blob, at(v.nleaves) + v.q0, 0) == 0) { fprintf(stderr, "a state without leaves is accepted\n"); return 1; }
  for (uint32_t q = 0; q < v.nstates; ++q)
    if (v.fin_leaf[q] != KXP_NO_LEAF) {
      if (withByte(blob, at(v.fin_leaf) + q, v.nleaves[q]) == 0) { fprintf(stderr, "a final leaf beyond the state's leaves is accepted\n"); return 1; }
      break;
    }
  for (size_t i = 0; v.has_tbl && i < v.nent(); ++i)
    if (v.back[i] != KXP_DEAD_LEAF && v.tbOf(v.back[i])) {
      if (withWord(blob, at(v.back + i), (v.back[i] & 0xFFFFFFu) | (v.ntables + 1) << 24) == 0) { fprintf(stderr, "a table beyond the tables is accepted\n"); return 1; }
      if (withWord(blob, at(v.back + i), v.back[i] & ~0x100u) == 0) { fprintf(stderr, "a table on an entry that does not copy is accepted\n"); return 1; }
      break;
    }
  if (v.has_tbl && build(blob.data(), blob.size() - 100) == 0) { fprintf(stderr, "truncated symbol tables are accepted\n"); return 1; }
  printf("%zu calls, %zu refused\n", g_calls, g_refused);
  return g_refused > 100 ? 0 : 1;
}
