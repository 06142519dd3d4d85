// project_lanes.cpp — the two lane bodies of the projection (kx_field_lanes.h: fp_splen_lane, fp_splice_lane; the kernels k_fpsplen
// and k_fpsplice are grid-stride loops around them) run one lane at a time on the host and compared with a plain reference written
// here.  Built with -fsanitize=address,undefined by tests/test_records_project.py.  The program is not run: every document draws a
// random output and status.  Every array has exactly the size the kernels may touch (the sanitizer sees a read or a write one
// past it), and the output sits between guard bytes.  The record bodies in `in` are random bytes the projection must not use.
//
//   project_lanes [cases]      exit 0: every case equal and every listed population seen
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <random>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../include/kxhip.h"
#include "../../kleenexlang_amd/csrc/engine/kx_field_lanes.h"

typedef unsigned long long u64;

namespace {

struct Item { u64 lo, hi; };   // hi = FL_OPEN: open

// exactly n elements on the heap (n = 0: one, never touched by a correct lane, since a zero-length new[] has no usable byte)
template <class T> struct Exact {
  T* p; size_t n;
  explicit Exact(size_t k) : p(new T[k ? k : 1]()), n(k) {}
  ~Exact() { delete[] p; }
  Exact(const Exact&) = delete;
  T& operator[](size_t i) { return p[i]; }
};

int fail(const char* what, unsigned seed) { fprintf(stderr, "case %u: %s\n", seed, what); return 1; }

std::set<std::string> seen;

int one_case(unsigned seed) {
  std::mt19937 rnd(seed);
  auto upto = [&](u64 k) { return (u64)(rnd() % (k + 1)); };
  auto pick = [&](std::initializer_list<uint32_t> v) { return v.begin()[rnd() % v.size()]; };
  // the items as written, and S in normal form
  std::vector<Item> items;
  std::vector<std::pair<u64, u64>> norm;
  for (;;) {
    items.clear();
    const uint32_t ni = seed % 7 == 0 ? 16 : seed % 7 == 1 ? 1 : 1 + (uint32_t)upto(15);
    for (uint32_t t = 0; t < ni; ++t) {
      const u64 lo = 1 + upto(11);
      const uint32_t kind = (uint32_t)upto(5);
      if (kind == 0) items.push_back({lo, FL_OPEN});
      else if (kind == 1 && !items.empty()) items.push_back(items[upto(items.size() - 1)]);   // a repeat
      else items.push_back({lo, lo + (kind >= 4 ? upto(3) : 0)});
    }
    if (upto(3) == 0) std::reverse(items.begin(), items.end());
    std::vector<std::pair<u64, u64>> s;
    for (const Item& it : items) s.emplace_back(it.lo, it.hi);
    std::sort(s.begin(), s.end());
    norm.clear();
    for (const auto& r : s) {
      if (!norm.empty() && (norm.back().second == FL_OPEN || r.first <= norm.back().second + 1)) norm.back().second = std::max(norm.back().second, r.second);
      else norm.push_back(r);
    }
    if (norm.size() <= 8) break;
  }
  const bool open = norm.back().second == FL_OPEN;
  const u64 need = open ? norm.back().first : norm.back().second;
  auto member = [&](u64 K) { for (const auto& r : norm) if (K >= r.first && K <= r.second) return true; return false; };
  Exact<u64> rng(16), itm(32);
  for (uint32_t j = 0; j < 8; ++j) {
    rng[j] = j < norm.size() ? norm[j].first : FL_OPEN;
    rng[8 + j] = j < norm.size() ? norm[j].second : FL_OPEN;
  }
  for (uint32_t j = 0; j < 16; ++j) {   // the items' table as the host driver fills it: the members of S below lo, and the size
    itm[j] = itm[16 + j] = 0;
    if (j >= items.size()) continue;
    for (u64 K = 1; K < items[j].lo; ++K) itm[j] += member(K) ? 1 : 0;
    itm[16 + j] = items[j].hi == FL_OPEN ? FL_OPEN : items[j].hi - items[j].lo + 1;
  }
  // the framing
  FPSpec P{};
  P.rng = rng.p; P.itm = itm.p;
  P.n_items = (uint32_t)items.size();
  P.ofs_len = pick({0, 1, 2, 8});
  P.sfx_len = pick({0, 1, 8});
  P.sep_len = pick({0, 1, 2});
  P.keep = (uint32_t)upto(1);
  uint8_t ofs[8], sfx[8];
  for (uint32_t i = 0; i < 8; ++i) { ofs[i] = (uint8_t)('A' + i); sfx[i] = (uint8_t)('s' + i); }
  for (uint32_t i = 0; i < P.ofs_len; ++i) P.ofs8 |= (u64)ofs[i] << (8 * i);
  for (uint32_t i = 0; i < P.sfx_len; ++i) P.sfx8 |= (u64)sfx[i] << (8 * i);
  const u64 n = 1 + upto(seed % 5 == 0 ? 70 : 12);
  const bool last_whole = upto(2) == 0;
  P.whole = last_whole ? n - 1 : ~0ull;
  // the records: fields found, documents, outputs, statuses
  const uint32_t reject_pct = pick({0, 10, 40, 90}), short_pct = pick({0, 10, 50}), empty_pct = pick({0, 30, 80, 100});
  std::vector<u64> fields(n);
  std::vector<std::vector<u64>> doc_field(n);            // the field numbers of a record's documents
  std::vector<std::vector<std::string>> doc_out(n);
  std::vector<std::vector<kx_batch_doc>> doc_rec(n);
  u64 ndocs = 0, obytes = 0;
  for (u64 i = 0; i < n; ++i) {
    const bool too_short = need > 1 ? upto(99) < short_pct : false;
    fields[i] = too_short ? upto(need - 1) : need + upto(seed % 3 == 0 ? 40 : 3);
    if (too_short) continue;
    const bool rejected = upto(99) < reject_pct;
    for (u64 K = 1; K <= fields[i]; ++K) {
      if (!member(K)) continue;
      kx_batch_doc d{0, 0u, 0u};
      if (rejected && upto(2) == 0) d = kx_batch_doc{upto(9), 1u, (uint32_t)upto(2)};
      std::string o;
      if (!d.status && upto(99) >= empty_pct) for (u64 k = 1 + upto(seed % 4 == 0 ? 40 : 4); k; --k) o.push_back((char)('a' + upto(25)));
      doc_field[i].push_back(K); doc_out[i].push_back(o); doc_rec[i].push_back(d);
      obytes += o.size();
    }
    ndocs += doc_field[i].size();
  }
  Exact<u64> off(n + 1), d0(n + 1), nf(n), poff(ndocs + 1);
  Exact<kx_batch_doc> drec(ndocs);
  Exact<uint8_t> pout(obytes);
  std::vector<uint8_t> inb;
  {
    u64 d = 0, ob = 0;
    for (u64 i = 0; i < n; ++i) {
      off[i] = inb.size(); d0[i] = d; nf[i] = fields[i];
      for (u64 k = upto(20); k; --k) inb.push_back((uint8_t)('0' + upto(9)));   // the body: never read
      if (!(last_whole && i == n - 1)) for (u64 k = 0; k < P.sep_len; ++k) inb.push_back((uint8_t)(k ? '\n' : '\r'));
      for (size_t k = 0; k < doc_field[i].size(); ++k, ++d) {
        poff[d] = ob; drec[d] = doc_rec[i][k];
        memcpy(pout.p + ob, doc_out[i][k].data(), doc_out[i][k].size());
        ob += doc_out[i][k].size();
      }
    }
    off[n] = inb.size(); d0[n] = d; poff[ndocs] = ob;
  }
  Exact<uint8_t> in(inb.size());
  if (!inb.empty()) memcpy(in.p, inb.data(), inb.size());
  // the reference: per record its result, K, and its bytes
  std::vector<std::string> want(n);
  std::vector<kx_batch_doc> want_rec(n);
  std::vector<u64> want_k(n);
  for (u64 i = 0; i < n; ++i) {
    want_rec[i] = kx_batch_doc{0, 0u, 0u}; want_k[i] = 0;
    if (doc_field[i].empty()) {
      want_rec[i] = kx_batch_doc{fields[i], 2u, 0u};
      for (u64 K = fields[i] + 1;; ++K) if (member(K)) { want_k[i] = K; break; }
      continue;
    }
    for (size_t k = 0; k < doc_field[i].size(); ++k) if (doc_rec[i][k].status) { want_rec[i] = doc_rec[i][k]; want_k[i] = doc_field[i][k]; break; }
    if (want_rec[i].status) continue;
    std::string o;
    bool first = true;
    for (const Item& it : items)
      for (size_t k = 0; k < doc_field[i].size(); ++k) {
        const u64 K = doc_field[i][k];
        if (K < it.lo || K > it.hi) continue;
        if (!first) o.append((const char*)ofs, P.ofs_len);
        first = false;
        o += doc_out[i][k];
      }
    if (P.keep && !(last_whole && i == n - 1)) o.append((const char*)in.p + off[i + 1] - P.sep_len, P.sep_len);
    o.append((const char*)sfx, P.sfx_len);
    want[i] = o;
  }
  // k_fpsplen's lanes
  Exact<u64> ooff(n + 1);
  u64 total = 0;
  for (u64 i = 0; i < n; ++i) {
    kx_batch_doc r;
    u64 K = 99;
    const u64 len = fp_splen_lane(P, off.p, i, d0.p, nf.p, poff.p, drec.p, &r, &K);
    if (r.status != want_rec[i].status || r.fail_pos != want_rec[i].fail_pos || r.fail_stage != want_rec[i].fail_stage) return fail("k_fpsplen: a record's result differs", seed);
    if (K != want_k[i]) return fail("k_fpsplen: a record's field number differs", seed);
    if (len != want[i].size()) return fail("k_fpsplen: a record's length differs", seed);
    ooff[i] = total;
    total += len;
  }
  ooff[n] = total;
  // k_fpsplice's lanes, at one alignment of the output (the seed's) in the order a grid would not take them
  const uint32_t align = seed & 15;
  std::vector<uint8_t> store(16 + 16 + align + total + 16 + 16);
  uint8_t* base = (uint8_t*)(((uintptr_t)store.data() + 15) & ~(uintptr_t)15);
  uint8_t* out = base + 16 + align;
  memset(store.data(), 0xA5, store.size());
  if (total) {
    const u64 ng = (align + total + 15) >> 4;
    for (u64 g = ng; g-- > 0;) fp_splice_lane(P, in.p, off.p, n, d0.p, pout.p, poff.p, ooff.p, total, out, g);
  }
  std::string all;
  for (u64 i = 0; i < n; ++i) all += want[i];
  if (all.size() != total || memcmp(out, all.data(), total) != 0) return fail("k_fpsplice: the output differs", seed);
  for (uint8_t* q = store.data(); q < store.data() + store.size(); ++q)
    if ((q < out || q >= out + total) && *q != 0xA5) return fail("k_fpsplice: a byte outside the output was written", seed);
  // what this case held
  auto rej = [&](u64 i) { return want_rec[i].status != 0; };
  seen.insert("items " + std::to_string(P.n_items == 1 ? 1 : P.n_items == 16 ? 16 : 2));
  seen.insert(open ? "open" : "closed");
  for (size_t a = 0; a < items.size(); ++a) for (size_t b = a + 1; b < items.size(); ++b) {
    if (items[a].lo == items[b].lo && items[a].hi == items[b].hi) seen.insert("repeat");
    if (items[b].lo < items[a].lo) seen.insert("reversal");
  }
  seen.insert("ofs_len " + std::to_string(P.ofs_len));
  seen.insert("sep_len " + std::to_string(P.sep_len));
  seen.insert(P.keep ? "keep_sep" : "no keep_sep");
  seen.insert("suffix " + std::to_string(P.sfx_len));
  seen.insert("align " + std::to_string(align));
  if (total) {
    if (rej(0)) seen.insert("rejected first");
    if (rej(n - 1)) seen.insert("rejected last");
    for (u64 i = 0; i + 1 < n; ++i) if (rej(i) && rej(i + 1)) seen.insert("rejected adjacent");
    for (u64 i = 0; i < n; ++i) {
      if (want_rec[i].status == 2) seen.insert("short record");
      if (want_rec[i].status == 1) seen.insert("rejected field");
      if (!rej(i) && want[i].empty()) seen.insert("accepted record without a byte");
      if (!rej(i)) for (const Item& it : items) if (it.lo > fields[i]) seen.insert("item without a field");
      size_t run = 0;
      for (const std::string& o : doc_out[i]) { run = o.empty() ? run + 1 : 0; if (run >= 2 && !rej(i)) seen.insert("empty outputs in a row"); }
    }
    for (u64 i = 0; i + 2 < n; ++i) if (!rej(i) && !rej(i + 1) && !rej(i + 2) && (ooff[i] + align) / 16 == (ooff[i + 3] + align - 1) / 16 && ooff[i + 3] > ooff[i + 2] && ooff[i + 1] > ooff[i])
      seen.insert("three records in one granule");
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const unsigned cases = argc > 1 ? (unsigned)atoi(argv[1]) : 20000;
  for (unsigned seed = 0; seed < cases; ++seed) if (one_case(seed)) return 1;
  std::vector<std::string> wanted = {"items 1", "items 2", "items 16", "open", "closed", "repeat", "reversal", "ofs_len 0", "ofs_len 1", "ofs_len 2", "ofs_len 8",
                                     "sep_len 0", "sep_len 1", "sep_len 2", "keep_sep", "no keep_sep", "suffix 0", "suffix 1", "suffix 8", "rejected first",
                                     "rejected last", "rejected adjacent", "short record", "rejected field", "accepted record without a byte",
                                     "empty outputs in a row", "three records in one granule", "item without a field"};
  for (int a = 0; a < 16; ++a) wanted.push_back("align " + std::to_string(a));
  int missing = 0;
  for (const std::string& w : wanted) if (!seen.count(w)) { fprintf(stderr, "never seen: %s\n", w.c_str()); ++missing; }
  if (missing) return 1;
  printf("project_lanes: %u cases, %zu populations\n", cases, wanted.size());
  return 0;
}
