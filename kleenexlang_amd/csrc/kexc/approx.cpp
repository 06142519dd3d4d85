// approx.cpp — approximate matching: the `<k>t` term and --metric / --approxmode / --ite.
//
// The reference implements approximation as a source-to-source rewrite of the desugared program, applied once the whole
// program is desugared (src/KMC/Kleenex/Desugaring.hs:146-149,209-229):
//   core form           src/KMC/Kleenex/Core.hs:49-75          (stdToCore)
//   k-fold rewrite      src/KMC/Kleenex/Approximation.hs:13-26,61-136
//   rewrite tables      src/KMC/Kleenex/ApproximationMetrics.hs:25-195
// Everything after the desugarer (transducer, determinization, tables, engine) sees an ordinary RProg.  Identifiers are
// assigned with the reference's counter arithmetic, and the alternatives of every sum keep the reference's order: the
// greedy leftmost parse, and so the output, depends on that order.
#include "kexc.h"

#include <algorithm>

namespace kexc {

namespace {

using Decls = std::map<int, RTerm>;

RTerm seqT(std::vector<int> ids) { RTerm t; t.kind = RTerm::RSeq; t.ids = std::move(ids); return t; }
RTerm sumT(std::vector<int> ids) { RTerm t; t.kind = RTerm::RSum; t.ids = std::move(ids); return t; }
RTerm readT(const ByteSet& p, bool copy) { RTerm t; t.kind = RTerm::RRead; t.pred = p; t.copy = copy; return t; }
RTerm byteT(int b) { RTerm t; t.kind = RTerm::RConst; t.c = {0, b}; return t; }

// Recursion guard: the rewrites recurse along the program; a grammar whose continuation stacks grow without bound (not
// right-regular) would recurse forever, and a very deep one would exhaust the native stack (8 MiB by default; a level of
// the core rewrite takes a few hundred bytes of it).  An approximated sequence of n reads is about 2n levels deep.
constexpr int kMaxDepth = 4000;

std::string describe(const RTerm& t) {   // names a term in error messages, in the reference's `show` shape
  switch (t.kind) {
    case RTerm::RConst: {
      static const char* acts[] = {"Left ", "Right Push", "Right (Pop ", "Right (Write "};
      if (t.c.kind == 0) return "RConst (Left " + std::to_string(t.c.arg) + ")";
      if (t.c.kind == 1) return "RConst (Right Push)";
      return std::string("RConst (") + acts[t.c.kind] + std::to_string(t.c.arg) + "))";
    }
    case RTerm::RRead: return std::string("RRead <") + std::to_string(t.pred.size()) + " symbols> " + (t.copy ? "True" : "False");
    default: {
      std::string s = t.kind == RTerm::RSeq ? "RSeq [" : "RSum [";
      for (size_t i = 0; i < t.ids.size(); ++i) s += (i ? "," : "") + std::to_string(t.ids[i]);
      return s + "]";
    }
  }
}

// getDecl (Core.hs:37-40): the declaration of `rid`, through chains of one-element sequences
const RTerm& getDecl(int rid, const Decls& decls) {
  for (int guard = 0;; ++guard) {
    auto it = decls.find(rid);
    if (it == decls.end()) throw CompileError("internal error: identifier without declaration: " + std::to_string(rid));
    if (it->second.kind != RTerm::RSeq || it->second.ids.size() != 1) return it->second;
    if (guard > (int)decls.size()) throw CompileError("Approximation: the declaration " + std::to_string(rid) + " is a cycle of one-element sequences");
    rid = it->second.ids[0];
  }
}

// ------------------------------------------------------------------ core form (Core.hs)
// Rewrites the sub-program reached from one identifier so that every sequence has two elements, a read or a constant
// first; sums stay sums; continuation stacks are memoised by their contents.
struct CoreForm {
  const Decls& in;
  Decls out;
  int fresh = 0;
  std::map<std::vector<int>, int> visited;

  explicit CoreForm(const Decls& d) : in(d) {}

  int getFresh(const std::vector<int>& st) { int i = fresh++; visited[st] = i; return i; }   // Core.hs:18-23
  int insertDecl(int i, const RTerm& t) { out[i] = t; return i; }                           // Core.hs:26-28
  int decl(const RTerm& t, const std::vector<int>& st) { return insertDecl(getFresh(st), t); }  // Core.hs:31-34

  int rewrite(const std::vector<int>& stack, int depth) {   // Core.hs:49-67
    if (stack.empty()) throw CompileError("internal error: empty stack during declaration rewrite");
    if (depth > kMaxDepth || (int)stack.size() > kMaxDepth)
      throw CompileError("Approximation: the approximated sub-program is not right-regular or too deep (continuation stack over " +
                         std::to_string(kMaxDepth) + ")");
    // Core.hs:52-53: `vis > 0` — the stack that received id 0 counts as not yet visited, so the first stack can be
    // rewritten a second time; kept, it decides the numbering
    auto v = visited.find(stack);
    if (v != visited.end() && v->second > 0) return v->second;
    const RTerm& t = getDecl(stack[0], in);
    const std::vector<int> rest(stack.begin() + 1, stack.end());
    switch (t.kind) {
      case RTerm::RSum: {
        const int f = getFresh(stack);
        std::vector<int> ids;
        for (int x : t.ids) {
          std::vector<int> st{x};
          st.insert(st.end(), rest.begin(), rest.end());
          ids.push_back(rewrite(st, depth + 1));
        }
        return insertDecl(f, sumT(ids));
      }
      case RTerm::RSeq: {
        if (rest.empty() && t.ids.empty()) return decl(t, stack);
        const int f = getFresh(stack);
        std::vector<int> st(t.ids);
        st.insert(st.end(), rest.begin(), rest.end());
        const int nid = rewrite(st, depth + 1);
        return insertDecl(f, seqT({nid}));
      }
      default: {
        if (rest.empty()) return decl(t, stack);
        const int f = getFresh(stack);
        // Core.hs:64: `decl t stack` takes a second fresh id for the same stack, and the memo entry now names the bare
        // read or constant; followed to the letter
        const int id1 = decl(t, stack);
        const int id2 = rewrite(rest, depth + 1);
        return insertDecl(f, seqT({id1, id2}));
      }
    }
  }
};

// ------------------------------------------------------------------ the k-fold rewrite (Approximation.hs)
struct ApproxState {   // ApproximationMetrics.hs:13-15
  Decls n;                                // newDecls
  std::map<std::pair<int, int>, int> m;   // (old id, errors still allowed) → new id; old id -1 = the ε-end
  int c = 0;                              // counter
};

struct KFold {
  ApproxMetric metric;
  ApproxMode mode;
  const Decls& old;
  ApproxState s;

  KFold(ApproxMetric mt, ApproxMode md, const Decls& d) : metric(mt), mode(md), old(d) {}

  // HM.union newElems n: the new elements win
  void put(int id, const RTerm& t) { s.n[id] = t; }

  int lookupMapping(int rid, int k) const {   // Approximation.hs:33-38
    auto it = s.m.find({rid, k});
    if (it == s.m.end())
      throw CompileError("Internal error: Could not find mapping: (" + std::to_string(rid) + "," + std::to_string(k) + ")");
    return it->second;
  }

  // Approximation.hs:42-49: the list is translated from its end, so a new id goes to the last unmapped element first
  std::vector<int> translatePointers(const std::vector<int>& xs, int k) {
    std::vector<int> r(xs.size());
    for (size_t j = xs.size(); j-- > 0;) {
      auto it = s.m.find({xs[j], k});
      if (it != s.m.end()) r[j] = it->second;
      else { r[j] = s.c; s.m[{xs[j], k}] = s.c; ++s.c; }
    }
    return r;
  }

  void initialize(int rid, int k) {   // Approximation.hs:52-63
    for (int i = 0; i < k; ++i) {     // addStartSums: copy i first, then the sum over the copies with more errors allowed
      put(s.c, sumT({s.c + 1, s.c + 2}));
      s.m[{rid, i}] = s.c + 1;
      s.c += 2;
    }
    s.m[{rid, k}] = s.c++;
    for (int i = 0; i <= k; ++i) addEpsEnds(i);
  }

  void addEpsEnds(int k) {   // Approximation.hs:131-136
    const int rid = translatePointers({-1}, k)[0];
    if (k == 0) { put(rid, seqT({})); return; }
    rewriteEpsilon(rid, lookupMapping(-1, k - 1));
  }

  void rewriteEpsilon(int rid, int frid) {   // ApproximationMetrics.hs:25-52
    const int c = s.c;
    if (metric == ApproxMetric::Hamming) { put(rid, seqT({})); return; }
    if (mode == ApproxMode::Explicit) {
      put(rid, sumT({c + 3, c + 4}));
      put(c, byteT('D'));
      put(c + 1, seqT({c + 2, frid}));
      put(c + 2, readT(ByteSet::universe(), true));
      put(c + 3, seqT({c, c + 1}));
      put(c + 4, sumT({}));
      s.c = c + 5;
      return;
    }
    put(rid, sumT({c + 1, c + 2}));
    put(c, readT(ByteSet::universe(), mode == ApproxMode::Matching));
    put(c + 1, seqT({c, frid}));
    put(c + 2, seqT({}));
    s.c = c + 3;
  }

  void insertConst(int rid1, int rid2, const RTerm& t, int k) {   // Approximation.hs:100-104 (also insertRead at k = 0)
    const std::vector<int> p = translatePointers({rid1, rid2}, k);
    const int c = s.c;
    put(p[0], seqT({c, p[1]}));
    put(c, t);
    s.c = c + 1;
  }

  void insertRead(int rid1, int rid2, const RTerm& rt, int k) {   // Approximation.hs:118-127
    if (k == 0) { insertConst(rid1, rid2, rt, 0); return; }
    const std::vector<int> p = translatePointers({rid1, rid2}, k);
    rewriteRead(p[0], p[1], rid1, rid2, k, rt);
  }

  void rewriteRead(int rid, int rid_, int old1, int old2, int k, const RTerm& rt) {   // ApproximationMetrics.hs:58-195
    // frid / frid' (the same positions with one error fewer allowed) are looked up only by the tables that use them, as
    // the reference's lazy bindings are
    auto frid = [&]() { return lookupMapping(old1, k - 1); };
    auto frid_ = [&]() { return lookupMapping(old2, k - 1); };
    auto findMin = [&]() {   // RS.findMin of the read's range: the byte a deletion writes
      if (rt.pred.empty()) throw CompileError("Approximation: cannot approximate a read of the empty set");
      return byteT(rt.pred.first());
    };
    const ByteSet U = ByteSet::universe();
    const bool keep = mode == ApproxMode::Matching && rt.copy;   // `(mode == Matching) && out`
    const int c = s.c;
    switch (metric) {
      case ApproxMetric::LCS:
        if (mode == ApproxMode::Explicit) {   // :63-79
          put(rid, sumT({c, c + 1}));
          put(c, seqT({c + 11, rid_}));
          put(c + 1, sumT({c + 2, c + 6}));
          put(c + 2, seqT({c + 4, c + 8}));
          put(c + 3, readT(U, true));
          put(c + 4, byteT('I'));
          put(c + 5, byteT('D'));
          put(c + 6, seqT({c + 5, c + 10}));
          put(c + 7, seqT({c + 4, c + 8}));
          put(c + 8, seqT({c + 9, frid_()}));
          put(c + 9, findMin());
          put(c + 10, seqT({c + 3, frid()}));
          put(c + 11, rt);
          s.c = c + 12;
        } else if (mode == ApproxMode::Correction && rt.copy) {   // :80-91
          put(rid, sumT({c, c + 2}));
          put(c, seqT({c + 1, rid_}));
          put(c + 1, rt);
          put(c + 2, sumT({c + 3, c + 5}));
          put(c + 3, seqT({c + 4, frid()}));
          put(c + 4, readT(U, false));
          put(c + 5, seqT({c + 6, frid_()}));
          put(c + 6, findMin());
          s.c = c + 7;
        } else {   // :92-101
          put(rid, sumT({c, c + 2}));
          put(c, seqT({c + 1, rid_}));
          put(c + 1, rt);
          put(c + 2, sumT({c + 3, frid_()}));
          put(c + 3, seqT({c + 4, frid()}));
          put(c + 4, readT(U, keep));
          s.c = c + 5;
        }
        return;
      case ApproxMetric::Hamming:
        if (mode == ApproxMode::Explicit) {   // :105-117
          put(rid, sumT({c, c + 2}));
          put(c, seqT({c + 1, rid_}));
          put(c + 1, rt);
          put(c + 2, seqT({c + 3, c + 4}));
          put(c + 3, readT(U, true));
          put(c + 4, seqT({c + 5, c + 6}));
          put(c + 5, byteT('R'));
          put(c + 6, seqT({c + 7, frid_()}));
          put(c + 7, findMin());
          s.c = c + 8;
        } else if (mode == ApproxMode::Correction && rt.copy) {   // :118-128
          put(rid, sumT({c, c + 2}));
          put(c, seqT({c + 1, rid_}));
          put(c + 1, rt);
          put(c + 2, seqT({c + 3, c + 4}));
          put(c + 3, readT(U, false));
          put(c + 4, seqT({c + 5, frid_()}));
          put(c + 5, findMin());
          s.c = c + 6;
        } else {   // :129-137
          put(rid, sumT({c, c + 2}));
          put(c, seqT({c + 1, rid_}));
          put(c + 1, rt);
          put(c + 2, seqT({c + 3, frid_()}));
          put(c + 3, readT(U, keep));
          s.c = c + 4;
        }
        return;
      case ApproxMetric::Levenshtein:
        if (mode == ApproxMode::Explicit) {   // :141-163
          put(rid, sumT({c, c + 2}));
          put(c, seqT({c + 1, rid_}));
          put(c + 1, rt);
          put(c + 2, sumT({c + 3, c + 9}));
          put(c + 3, seqT({c + 4, c + 5}));
          put(c + 4, readT(U, true));
          put(c + 5, seqT({c + 6, c + 7}));
          put(c + 6, byteT('R'));
          put(c + 7, seqT({c + 8, frid_()}));
          put(c + 8, findMin());
          put(c + 9, sumT({c + 10, c + 14}));
          put(c + 10, seqT({c + 11, c + 12}));
          put(c + 11, byteT('D'));
          put(c + 12, seqT({c + 13, frid()}));
          put(c + 13, readT(U, true));
          put(c + 14, seqT({c + 15, c + 16}));
          put(c + 15, byteT('I'));
          put(c + 16, seqT({c + 17, frid_()}));
          put(c + 17, findMin());
          s.c = c + 18;
        } else if (mode == ApproxMode::Correction && rt.copy) {   // :164-180
          put(rid, sumT({c, c + 2}));
          put(c, seqT({c + 1, rid_}));
          put(c + 1, rt);
          put(c + 2, sumT({c + 3, c + 7}));
          put(c + 3, seqT({c + 4, c + 5}));
          put(c + 4, readT(U, false));
          put(c + 5, seqT({c + 6, frid_()}));
          put(c + 6, findMin());
          put(c + 7, sumT({c + 8, c + 10}));
          put(c + 8, seqT({c + 9, frid()}));
          put(c + 9, readT(U, false));
          put(c + 10, seqT({c + 11, frid_()}));
          put(c + 11, findMin());
          s.c = c + 12;
        } else {   // :181-193
          put(rid, sumT({c, c + 2}));
          put(c, seqT({c + 1, rid_}));
          put(c + 1, rt);
          put(c + 2, sumT({c + 3, c + 5}));
          put(c + 3, seqT({c + 4, frid_()}));
          put(c + 4, readT(U, keep));
          put(c + 5, sumT({c + 6, frid_()}));
          put(c + 6, seqT({c + 7, frid()}));
          put(c + 7, readT(U, keep));
          s.c = c + 8;
        }
        return;
    }
  }

  void insertSum(int rid, const RTerm& t, int k) {   // Approximation.hs:107-111
    const std::vector<int> ids = translatePointers(t.ids, k);
    put(lookupMapping(rid, k), sumT(ids));
  }

  void insertEps(int rid, int k) { put(lookupMapping(rid, k), seqT({lookupMapping(-1, k)})); }   // Approximation.hs:114-115

  void approxStms(int r, int k, int depth) {   // Approximation.hs:70-88
    for (;; ++depth) {   // a sequence continues with its tail: iterate instead of recursing
      if (depth > kMaxDepth)
        throw CompileError("Approximation: the approximated sub-program is too deep (over " + std::to_string(kMaxDepth) + " levels)");
      if (s.n.count(lookupMapping(r, 0))) return;
      const RTerm& t = getDecl(r, old);
      switch (t.kind) {
        case RTerm::RConst: for (int i = 0; i <= k; ++i) insertConst(r, -1, t, i); return;
        case RTerm::RRead: for (int i = 0; i <= k; ++i) insertRead(r, -1, t, i); return;
        case RTerm::RSum:
          for (int i = 0; i <= k; ++i) insertSum(r, t, i);
          for (int id : t.ids) approxStms(id, k, depth + 1);
          return;
        case RTerm::RSeq:
          if (t.ids.empty()) { for (int i = 0; i <= k; ++i) insertEps(r, i); return; }
          if (t.ids.size() == 2) {
            const RTerm& head = getDecl(t.ids[0], old);
            const int rid2 = t.ids[1];
            if (head.kind == RTerm::RRead) { for (int i = 0; i <= k; ++i) insertRead(r, rid2, head, i); r = rid2; continue; }
            if (head.kind == RTerm::RConst) { for (int i = 0; i <= k; ++i) insertConst(r, rid2, head, i); r = rid2; continue; }
            throw CompileError("Approximation: Sequence must start with const or read. Term: " + describe(t) + " not allowed");
          }
          throw CompileError("Cannot Approximation on term like " + describe(t));
      }
    }
  }
};

// calculateReach (Desugaring.hs:221-229), to the letter: a child already on the list resets the result to the list
// the call started with
void calculateReach(int r, const Decls& terms, std::vector<int>& rs, long& budget, int depth) {
  if (--budget < 0 || depth > kMaxDepth)
    throw CompileError("Approximation: the program is too large to check for nested approximation terms");
  auto it = terms.find(r);
  if (it == terms.end() || it->second.kind == RTerm::RConst || it->second.kind == RTerm::RRead) return;
  const std::vector<int> start = rs;
  for (int x : it->second.ids) {
    if (std::find(rs.begin(), rs.end(), x) != rs.end()) rs = start;
    else { rs.insert(rs.begin(), x); calculateReach(x, terms, rs, budget, depth + 1); }
  }
}

}  // namespace

std::map<int, RTerm> stdToCore(const std::map<int, RTerm>& decls, int start) {   // Core.hs:70-75: the result starts at 0
  CoreForm cf(decls);
  cf.rewrite({start}, 0);
  return std::move(cf.out);
}

std::map<int, RTerm> approxProg(const std::map<int, RTerm>& decls, int start, int k, int offset, ApproxMetric m, ApproxMode mode) {
  KFold kf(m, mode, decls);   // Approximation.hs:13-20: the result starts at `offset`
  kf.s.c = offset;
  kf.initialize(start, k);
  kf.approxStms(start, k, 0);
  return std::move(kf.s.n);
}

std::map<int, RTerm> approxProgIt(const std::map<int, RTerm>& decls, int start, int k, int offset, ApproxMetric m, ApproxMode mode) {
  std::map<int, RTerm> d = decls;   // Approximation.hs:24-26: k one-error rewrites, each of the previous result
  for (int i = 0; i < k; ++i) { d = approxProg(d, start, 1, offset, m, mode); start = offset; }
  return d;
}

void applyApproximation(std::map<int, RTerm>& decls, int fresh, const std::vector<ApproxSite>& sites, ApproxMetric m,
                        ApproxMode mode, bool ite) {   // Desugaring.hs:209-219
  std::vector<int> approxIds;
  for (auto& a : sites) approxIds.push_back(a.i2);
  int c = fresh;
  // the reference conses each site onto its list as it desugars it: the last one found is rewritten first
  for (auto a = sites.rbegin(); a != sites.rend(); ++a) {
    if (a->k < 1) continue;   // `<0>t` is `t`
    std::vector<int> reach;
    long budget = 50000000;
    calculateReach(a->i1, decls, reach, budget, 0);
    for (int x : reach)
      if (std::find(approxIds.begin(), approxIds.end(), x) != approxIds.end())
        throw CompileError("Approximated sub-programs cannot contain approximation terms");
    const std::map<int, RTerm> core = stdToCore(decls, a->i1);
    const std::map<int, RTerm> dnew = ite ? approxProgIt(core, 0, a->k, c, m, mode) : approxProg(core, 0, a->k, c, m, mode);
    for (auto& [id, t] : dnew) decls.emplace(id, t);   // M.union dold dnew: the old declarations win
    decls[a->i2] = seqT({c});
    c += (int)dnew.size();
  }
}

}  // namespace kexc
