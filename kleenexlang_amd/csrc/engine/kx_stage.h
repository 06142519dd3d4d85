// kx_stage.h — the STAGE LOADER (host side, no HIP and no device code): from a stage's section of a KXP blob
// (include/kxp_format.h) to the bytes the engine uploads and the structs its kernels take.  The steps, in the order buildStage runs them:
//   readStage         header, section pointers (StageView) and every bounds / index check: a corrupt blob ends here with KX_E_BLOB
//   buildPool         the engine's 16-byte-aligned constant pool
//   chooseLayout      symbol-table mode and entry layout (inline constants, job stride, direct, BIG, GENERAL), decided once
//   packEntries       the back entries in the chosen layout
//   buildGeneral      the two above, then the LDS image, pair table, synchronising automaton, the one-allocation layout and DevTables
//   chooseDelayed     the delayed form's delay and merge window (kx_delayed.h)
//   buildDelayedImage the delayed form's image, DfDev and the slow path's tables
// Every pointer field of DevTables / DfDev is a BYTE OFFSET into its allocation until the engine uploads the bytes and rebases it
// (kx_engine.hip: uploadStage).  kx_stage_describe_cfg (include/kxhip.h) shows all of it to a machine without a device.
#ifndef KX_STAGE_H
#define KX_STAGE_H
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/kxhip.h"
#include "../../../include/kxp_format.h"
#include "kx_delayed.h"

namespace kxst {

#ifdef __HIP__
using Quad = uint4;                            // (the engine's kernels fetch DfDev::sl_fmap as uint4)
#else
struct Quad { uint32_t x, y, z, w; };
#endif

constexpr uint32_t OFF_FWD = 256;         // the table image starts with the 256-byte class table; state rows follow
constexpr uint32_t PAIR_CLS2_AT = 16128;  // k_forward's pair mode keeps a second class table at this LDS address (kx_sweeps.inc: PAIR_CLS2)
constexpr uint32_t DF_STEP_MAX = 126;     // most bytes a step of the delayed form appends (the piece record's widths, kx_dfkernels.inc)

// ------------------------------------------------------------------ device-side program view
// The table image is copied verbatim into LDS (at LDS address 0 of the dynamic segment) and is
// addressed by *byte offsets* that are stored pre-scaled inside the tables themselves, so that a
// lookup is one add + one ds_read:
//   state handle h   = byte offset of the state's row in the image     (h = off_fwd + state·C·4)
//   cls4[byte]       = class·4 (u8 table at LDS address 0; programs with more than 64 byte classes
//                      store the class index and shift: DevTables::cshift)
//   e = fwd[h + cls4[b]] :  low 16 = next handle, high 16 = byte offset of the transition's back row
//   back entry x = ent[row + leaf·4] :
//     bit 0 "no input byte copied" | bit 1 "leaf' is a fixed point of this row that only copies" (k_backlen may
//     then skip the rest of a run of identical transitions) | bits 2-9 leaf' (so x & 0x3FC = leaf'·4) |
//     bits 10-22 action id (index into adesc: which constant) | bit 23 "a constant follows" |
//     bits 24-30 appended bytes (copy included); bit 31 = 0
//     appended = 127 escapes to the wide side table wlen (global memory) for long constants.
//   adesc[aid] = {byte offset of the constant in the pool (multiple of 16), its length}: two u32 per action.
//   The layout serves k_emit's step: the byte count is a whole byte (SDWA operand), bit 0 shifted to
//   bit 31 turns the staging address of a step that copies nothing into an out-of-range LDS address
//   (the hardware drops such stores), and bit 23 is the sign of byte 2 (one SDWA compare).
struct DevTables {
  const uint32_t* packed;     // [cls4 | fwd | ent | pool] image
  uint32_t packed_words;
  uint32_t off_fwd, off_ent, off_pool, off_cls, off_adesc, naid;  // byte offsets inside the image; number of actions
  uint32_t nstates, nclasses, q0h, maxleaves, deadh, nullrow, cshift, debug;
  // BIG programs (image beyond 16-bit byte addressing or the LDS budget; GENERAL instances only): the image stays in
  // global memory (L2), state handles count 4-byte words (hshift = 2) and back rows 16-byte units from off_ent
  // (rshift = 4, rbase = off_ent).  Otherwise hshift = rshift = rbase = 0 and stage_words = packed_words.
  uint32_t big, hshift, rshift, rbase, stage_words;
  // k_forward's two-symbol stride (piece_run_pair): pair[(q*C + c1)*C + c2] = C*C * state after two symbols, u16;
  // pair_words = 0: the program has none (table too large for LDS, GENERAL or BIG program).  pair_magic: e / (C*C) =
  // umulhi(e, pair_magic) for every row index e.
  const uint32_t* pair; uint32_t pair_words, pair_magic;
  const uint32_t* wlen;       // [nent] appended byte count per back entry (wide form)
  const uint8_t* cls;         // global copy for kernels that do not stage the big image
  const uint8_t* nleaves;     // [nstates+1]  by state id
  const uint8_t* fin_leaf;    // [nstates+1]
  const uint16_t* sync16;     // [(nsync+1)*C next | (nsync+1) state]: subsets < sync_multi are undecided
  uint32_t nsync, sync_multi, sync_words;  // sync_words = u32 words of the sync16 image
  const uint32_t* init_off;   // [maxleaves] pool offset / length of the initial closure output
  const uint32_t* init_len;
  // Symbol tables (kxp_format.h: output = table[symbol], AppendTblI): 256 bytes each at image offset off_tbl.
  //   xlat != 0    every copying entry of the program uses the SAME table: k_emit translates the piece's 64 input bytes
  //                once (table at image offset xlat), the entries and the sweeps are the ordinary ones
  //   tblmode != 0 several tables, or plain copies beside table steps (GENERAL instances only): bits 20-22 of an entry hold
  //                table+1 (0 = plain copy) and the action id is 10 bits wide (aid_mask)
  uint32_t off_tbl, xlat, tblmode, aid_mask;
  // INLINE-CONSTANT layout (inl != 0; fast instances, at most 64 leaves): a ONE-BYTE constant rides in its entry — byte 2 =
  // the constant, bits 8-15 zero, byte 3 = appended bytes as ever — and leaves with one more byte store of the sweeping lane
  // (piece_sweep2i) instead of a job.  Every other entry has bit 15 set (sign-extended into the inline store's address it
  // sends that store out of range), its action id in bits 10-14 (low) and 16-22 (high), bit 23 = a constant follows.  A
  // coder's one-byte codes on every step (regex flavour) are the case: no job slots, one round per wave-iteration.
  uint32_t inl;
  // JOB-STRIDE layout (jl != 0; fast instances; round 4): bits 10-15 = the constant's pool offset / 16 (at most 64 pool slots),
  // byte 2 = 4 where a constant follows and 0 elsewhere (bit 18), no adesc lookup.  piece_sweep2j stores a job word on EVERY
  // step at the lane's own list pointer and advances the pointer by byte 2: no vote, no rank, no scalar bookkeeping.
  uint32_t jl;
  // plain fast instances (no wide entries, symbol tables, inline or job-stride layout): the action field of an entry holds the
  // constant's pool offset / 16 itself instead of an index into adesc
  uint32_t direct;
  uint32_t short_consts;   // every path constant fits 16 bytes: k_emit copies them with the straight v_cmpx sequence (put_bytes16)
};

// the delayed form's device view (kx_dfkernels.inc has the kernels, kx_delayed.h the construction)
struct DfDev {
  const uint32_t* img; uint32_t words;
  uint32_t off_pool, deadh, esch, starth, K, C;
  const uint16_t* start_of_state;     // [nstates] handle of (q, nothing pending), 0xFFFF = none
  uint32_t orig_c4, hshift;           // the general tables' row size (C*4) and handle shift: k_sync's handles -> state ids
  uint32_t short_consts, debug;
  uint32_t nstates;                   // SST states: start_of_state's length
  uint32_t J;                         // merge window (kx_delayed.h): a lane's own part starts K + J symbols behind its synchronisation point
  uint32_t wide;                      // more than 31 byte classes: the class table holds class indices, the kernels shift by 3
  // Round 6 — the EXACT SLOW PATH of a context that the delay does not decide (k_dforward: `slow`): the path form as the blob holds
  // it, in global memory (sl_back[row * Lm + leaf] = parent | copy << 8 | constant << 9, 0xFFFFFFFF dead), and what a product state
  // owes: sl_q its SST state, sl_pend[(state * K + j) * Lm + leaf] the kind (copy | constant << 1) of pending step j at that leaf,
  // sl_defpc[sl_defoff[state] ..] the constants that are due.  sl_on = 0: the stage has none (more than 16 leaves): an escape
  // sends the whole shard to the general engine as in round 5.
  const Quad* sl_fmap;   // 3 x uint4 per (state, class): {next state | its leaves << 16, backward row, 0, 0} {parent leaf of leaves 0-15, a byte each, 0xFF dead} {… 16-31}
  const uint32_t* sl_back; const uint8_t* sl_nleaves; const uint8_t* sl_fin_leaf; const uint8_t* sl_cls;   // (nleaves, fin_leaf, cls: the general image's, in ITS allocation)
  const uint32_t* sl_pcoff; const uint8_t* sl_pcpool; const uint32_t* sl_pend; const uint32_t* sl_defoff; const uint32_t* sl_defpc; const uint16_t* sl_q;
  uint32_t sl_Lm, sl_npc, sl_on;
};

// a pointer field as a byte offset into its allocation, and back
template <class P> void setOff(const P*& p, size_t off) { p = reinterpret_cast<const P*>(off); }
template <class P> size_t offOf(const P* p) { return reinterpret_cast<size_t>(p); }
template <class P> void rebase(const P*& p, const void* base) { p = reinterpret_cast<const P*>(reinterpret_cast<uintptr_t>(base) + offOf(p)); }
inline void rebaseTables(DevTables& T, const void* d) {
  rebase(T.packed, d); rebase(T.pair, d); rebase(T.wlen, d); rebase(T.cls, d); rebase(T.nleaves, d); rebase(T.fin_leaf, d);
  rebase(T.sync16, d); rebase(T.init_off, d); rebase(T.init_len, d);
}
inline void rebaseDelayed(DfDev& D, const void* d_df, const void* d_slow, const void* d_all) {
  rebase(D.img, d_df); rebase(D.start_of_state, d_df);
  if (!D.sl_on) return;
  rebase(D.sl_fmap, d_slow); rebase(D.sl_back, d_slow); rebase(D.sl_pcoff, d_slow); rebase(D.sl_pcpool, d_slow); rebase(D.sl_pend, d_slow);
  rebase(D.sl_defoff, d_slow); rebase(D.sl_defpc, d_slow); rebase(D.sl_q, d_slow);
  rebase(D.sl_nleaves, d_all); rebase(D.sl_fin_leaf, d_all); rebase(D.sl_cls, d_all);
}

inline size_t pad4(size_t x) { return (x + 3) & ~(size_t)3; }
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int fail(std::string& err, int code, const char* m) { err = m; return code; }

// does a table image of the delayed form respect the piece record's widths?  (a stage whose image does not has no delayed form)
inline bool dfRecFits(const uint32_t* img, uint32_t nrows, uint32_t C) {
  if (256u + (uint64_t)nrows * C * 8u > 65536u) return false;          // every row handle below 64 KiB (and a multiple of 8 by construction)
  for (size_t i = 0; i < (size_t)nrows * C; ++i) if ((img[64 + 2 * i + 1] >> 24) > DF_STEP_MAX) return false;
  return true;
}

// ------------------------------------------------------------------ readStage: the blob's sections, checked
struct StageView {   // const pointers into the blob
  uint32_t nstates, C, q0, Lm, nback, npc, pcpl, nsync, flags;
  const uint8_t* cls; const uint16_t* delta; const uint32_t* pback; const uint8_t *nleaves, *fin_leaf; const uint32_t* back;
  const uint32_t* pcoff; const uint8_t* pcpool; const uint32_t *init_const, *sync_next, *sync_state;
  bool has_tbl; uint32_t ntables; const uint8_t* tables;
  size_t sc() const { return (size_t)nstates * C; }
  size_t nent() const { return (size_t)nback * Lm; }
  bool act() const { return (flags & 1u) != 0; }
  uint32_t actRegs() const { return flags >> 8; }
  uint32_t pcOf(uint32_t e) const { return has_tbl ? (e >> 9) & 0x7FFFu : e >> 9; }
  uint32_t tbOf(uint32_t e) const { return has_tbl ? e >> 24 : 0u; }   // table+1, 0 = none
  uint32_t clen(uint32_t pc) const { return pcoff[pc + 1] - pcoff[pc]; }
  uint32_t dlen(uint32_t e) const { return clen(pcOf(e)) + ((e >> 8) & 1); }   // bytes a live entry appends, copy included
  // an entry that does not fit the compact form (≥ 127 appended bytes) escapes to the wide side table: GENERAL instances
  bool anywide() const {
    for (size_t i = 0; i < nent(); ++i) if (back[i] != KXP_DEAD_LEAF && dlen(back[i]) >= 127) return true;
    return false;
  }
  uint32_t rowLen(uint32_t b) const {   // ragged back rows: row b keeps entries up to its last live leaf
    uint32_t rl = 1;
    for (uint32_t j = 0; j < Lm; ++j) if (back[(size_t)b * Lm + j] != KXP_DEAD_LEAF) rl = j + 1;
    return rl;
  }
  uint32_t poolBytes() const {          // the engine's pool (buildPool) without its 16 bytes of padding
    uint32_t n = 0;
    for (uint32_t pc = 0; pc < npc; ++pc) n += (clen(pc) + 15) & ~15u;
    return n;
  }
};

inline int readStage(const uint8_t*& c, const uint8_t* end, StageView& v, std::string& err) {
  if (end < c || (size_t)(end - c) < 64) return fail(err, KX_E_BLOB, "truncated stage header");
  uint32_t h[16];
  memcpy(h, c, 64); c += 64;
  if (h[0] != KXP_STAGE_MAGIC) return fail(err, KX_E_BLOB, "bad stage magic");
  const uint32_t nstates = h[1], C = h[2], q0 = h[3], nactions = h[5], nops = h[6], nconsts = h[7], cpl = h[8];
  const uint32_t Lm = h[9], nback = h[10], npc = h[11], pcpl = h[12], nsync = h[13];
  const size_t sc = (size_t)nstates * C;
  {   // total size of the sections that follow, in 64-bit arithmetic, against what is left of the blob
    const unsigned long long need = 256ull + pad4(sc * 2) + sc * 4 + (unsigned long long)nstates * 4 + ((unsigned long long)nactions + 1) * 4 +
                                    (unsigned long long)nops * 8 + ((unsigned long long)nconsts + 1) * 4 + pad4(cpl) + sc * 4 + 2 * pad4(nstates) +
                                    (unsigned long long)nback * Lm * 4 + ((unsigned long long)npc + 1) * 4 + pad4(pcpl) + (unsigned long long)Lm * 4 +
                                    (unsigned long long)nsync * C * 4 + (unsigned long long)nsync * 4;
    if (nstates > 0xFFFFu || C > 256 || Lm > 256 || need > (unsigned long long)(end - c)) return fail(err, KX_E_BLOB, "truncated stage body");
  }
  v.nstates = nstates; v.C = C; v.q0 = q0; v.Lm = Lm; v.nback = nback; v.npc = npc; v.pcpl = pcpl; v.nsync = nsync; v.flags = h[15];
  v.cls = c; c += 256;
  v.delta = (const uint16_t*)c; c += pad4(sc * 2);
  c += sc * 4;                                   // act        (register form: not used by the engine)
  c += (size_t)nstates * 4;                      // final_act
  c += ((size_t)nactions + 1) * 4;               // act_off
  c += (size_t)nops * 8;                         // ops
  c += ((size_t)nconsts + 1) * 4; c += pad4(cpl);  // consts
  v.pback = (const uint32_t*)c; c += sc * 4;
  v.nleaves = c; c += pad4(nstates);
  v.fin_leaf = c; c += pad4(nstates);
  v.back = (const uint32_t*)c; c += (size_t)nback * Lm * 4;
  v.pcoff = (const uint32_t*)c; c += ((size_t)npc + 1) * 4;
  v.pcpool = c; c += pad4(pcpl);
  v.init_const = (const uint32_t*)c; c += (size_t)Lm * 4;
  v.sync_next = (const uint32_t*)c; c += (size_t)nsync * C * 4;
  v.sync_state = (const uint32_t*)c; c += (size_t)nsync * 4;
  if (c > end) return fail(err, KX_E_BLOB, "truncated stage body");
  v.has_tbl = (h[15] & KXP_STAGE_HAS_TABLES) != 0;
  v.ntables = 0; v.tables = nullptr;
  if (v.has_tbl) {
    if ((size_t)(end - c) < 4) return fail(err, KX_E_BLOB, "truncated symbol tables");
    memcpy(&v.ntables, c, 4); c += 4;
    if (v.ntables == 0 || v.ntables > KXP_MAX_TABLES || (size_t)(end - c) < (size_t)v.ntables * 256) return fail(err, KX_E_BLOB, "truncated symbol tables");
    v.tables = c; c += (size_t)v.ntables * 256;
  }
  // every index the tables hold is checked against the table it points into before it is used (a truncated or corrupt
  // blob must give KX_E_BLOB, not an out-of-bounds read)
  if (q0 >= nstates) return fail(err, KX_E_BLOB, "start state out of range");
  for (size_t i = 0; i < sc; ++i) {
    if (v.delta[i] != KXP_NO_STATE && v.delta[i] >= nstates) return fail(err, KX_E_BLOB, "transition target out of range");
    if (v.delta[i] != KXP_NO_STATE && v.pback[i] >= nback) return fail(err, KX_E_BLOB, "backward row out of range");
  }
  for (uint32_t i = 0; i <= npc; ++i) if (v.pcoff[i] > pcpl || (i && v.pcoff[i] < v.pcoff[i - 1])) return fail(err, KX_E_BLOB, "path constant pool offsets out of order");
  for (size_t i = 0; i < v.nent(); ++i) {
    const uint32_t e = v.back[i];
    if (e != KXP_DEAD_LEAF && (v.pcOf(e) >= npc || (e & 0xFF) >= Lm || v.tbOf(e) > v.ntables || (v.tbOf(e) && !((e >> 8) & 1)))) return fail(err, KX_E_BLOB, "backward entry out of range");
  }
  for (uint32_t j = 0; j < Lm; ++j) if (v.init_const[j] >= npc) return fail(err, KX_E_BLOB, "initial constant out of range");
  for (uint32_t q = 0; q < nstates; ++q)
    if (v.nleaves[q] == 0 || v.nleaves[q] > Lm || (v.fin_leaf[q] != KXP_NO_LEAF && v.fin_leaf[q] >= v.nleaves[q])) return fail(err, KX_E_BLOB, "leaf count out of range");
  for (int b = 0; b < 256; ++b) if (v.cls[b] >= C) return fail(err, KX_E_BLOB, "byte class out of range");
  for (size_t i = 0; i < (size_t)nsync * C; ++i) if (v.sync_next[i] != KXP_SYNC_UNKNOWN && v.sync_next[i] >= nsync) return fail(err, KX_E_BLOB, "synchronising automaton target out of range");
  for (uint32_t i = 0; i < nsync; ++i) if (v.sync_state[i] < KXP_SYNC_UNKNOWN && v.sync_state[i] >= nstates) return fail(err, KX_E_BLOB, "synchronising automaton state out of range");
  if (nstates == 0 || C == 0 || Lm == 0 || Lm > 254 || (size_t)(nstates + 1) * C * 4 + OFF_FWD > 0x3FFF0)
    return fail(err, KX_E_BLOB, "program outside engine limits (states x classes > 256 KiB, or more than 254 leaves)");
  return 0;
}

// the blob's own header: *first = the first stage's section, *nstages their number
inline int readBlobHeader(const void* blob, size_t blob_len, const uint8_t** first, uint32_t* nstages, std::string& err) {
  if (!blob) return fail(err, KX_E_ARG, "null argument");
  const uint8_t* b = (const uint8_t*)blob;
  if (blob_len < 20 || memcmp(b, KXP_MAGIC, 8)) return fail(err, KX_E_BLOB, "not a KXP blob");
  uint32_t ver, ns, il;
  memcpy(&ver, b + 8, 4); memcpy(&ns, b + 12, 4); memcpy(&il, b + 16, 4);
  if (ver != KXP_VERSION || ns == 0 || ns > 64) return fail(err, KX_E_BLOB, "unsupported KXP version");
  if ((unsigned long long)20 + pad4(il) > blob_len) return fail(err, KX_E_BLOB, "truncated blob header");
  *first = b + 20 + pad4(il); *nstages = ns;
  return 0;
}

// the engine's own pool: every path constant starts on a 16-byte boundary and is zero-padded to a multiple of 16
// (k_emit fetches constants with aligned 16-byte LDS reads); off[pc] = its byte offset there, off[npc] = the pool's end
struct Pool { std::vector<uint32_t> off; std::vector<uint8_t> bytes; };
inline Pool buildPool(const StageView& v) {
  Pool p;
  p.off.assign(v.npc + 1, 0);
  for (uint32_t pc = 0; pc < v.npc; ++pc) {
    p.off[pc] = (uint32_t)p.bytes.size();
    p.bytes.insert(p.bytes.end(), v.pcpool + v.pcoff[pc], v.pcpool + v.pcoff[pc + 1]);
    p.bytes.resize((p.bytes.size() + 15) & ~(size_t)15, 0);
  }
  p.off[v.npc] = (uint32_t)p.bytes.size();
  p.bytes.resize(p.bytes.size() + 16, 0);
  return p;
}

// ------------------------------------------------------------------ chooseLayout: decided once, before any entry is packed
struct Layout {
  uint32_t xlat_tb = 0;      // one table on every copying entry → translate the piece once (xlat): that table + 1
  bool tblmode = false;      // anything else with tables → per-entry table ids
  bool inl = false, jl = false, direct = false;   // DevTables::inl / jl / direct
  bool big = false;          // DevTables::big: the image does not fit 16-bit byte addressing (or the LDS budget); rows are then padded to 16 bytes
  bool general = false;      // wide back entries, per-entry tables, BIG or more than 64 byte classes: the GENERAL kernel instances
  uint32_t cshift = 0;       // class·4 fits a byte up to 64 classes
};
// `alt`: the job-stride alternative of a stage whose configuration leaves the choice to the data (HostStage::has_alt)
inline int chooseLayout(const StageView& v, const kx_config& cfg, bool alt, Layout& L, std::string& err) {
  L = Layout();
  if (v.has_tbl) {
    bool any = false, plain = false, several = false;
    uint32_t top = 0;
    for (size_t i = 0; i < v.nent(); ++i) {
      if (v.back[i] == KXP_DEAD_LEAF) continue;
      const uint32_t tb = v.tbOf(v.back[i]);
      if (tb > top) top = tb;
      if (!((v.back[i] >> 8) & 1)) continue;
      if (!tb) plain = true;
      else { if (any && tb != L.xlat_tb) several = true; any = true; L.xlat_tb = tb; }
    }
    L.tblmode = any && (plain || several || (cfg.force & KX_FORCE_TBLMODE));
    if (!any || L.tblmode) L.xlat_tb = 0;
    if (L.tblmode && top > 7) return fail(err, KX_E_BLOB, "program outside engine limits (more than 7 symbol tables beside plain copies)");
  }
  if (v.act() && v.actRegs() > KXP_MAX_ACTION_REGS) return fail(err, KX_E_BLOB, "too many action registers");
  if (v.act() && v.has_tbl) return fail(err, KX_E_BLOB, "symbol tables in a stage with register actions (a table could write the escape byte)");
  const bool anywide = v.anywide(), force_big = (cfg.force & KX_FORCE_BIG) != 0 /* tests: any program through the BIG instances */;
  const bool compact = !L.tblmode && !anywide && v.C <= 64;   // what every fast layout needs
  const uint32_t pool = v.poolBytes();
  // the inline-constant layout (DevTables::inl) pays one more byte store on every step: taken when one-byte constants are
  // at least as many path entries as longer ones (a static stand-in for "most steps append one"; KX_INL=0/1 overrides)
  size_t one = 0, longer = 0, ent_words = 2 * (size_t)v.Lm;
  for (size_t i = 0; i < v.nent(); ++i) {
    if (v.back[i] == KXP_DEAD_LEAF) continue;
    const uint32_t cl = v.clen(v.pcOf(v.back[i]));
    if (cl == 1) ++one; else if (cl > 1) ++longer;
  }
  const bool inl = (cfg.inline_consts ? cfg.inline_consts == 2 : one > 0 && one >= longer) && compact && v.Lm <= 64 && !force_big;
  // the job-stride layout (DevTables::jl): every constant within the first 64 pool slots of 16 bytes, no wide entry, no
  // symbol tables, the inline layout not taken; KX_JL=0 keeps the vote-and-rank sweep (A/B runs)
  const bool jl = (alt || cfg.job_stride == 2) && !inl && compact && !L.xlat_tb && v.Lm <= 64 && pool <= 64 * 16 && !force_big;
  const bool direct = !inl && !jl && compact && !L.xlat_tb && pool < (1u << 17) && !(cfg.disable & KX_OFF_DIRECT);
  for (uint32_t b = 0; b < v.nback; ++b) ent_words += v.rowLen(b);
  const size_t ent_end = (size_t)OFF_FWD + (v.nstates + 1) * v.C * 4 + ent_words * 4;
  L.big = force_big || ent_end > 65532 || ent_end + (pool + 16) + 8 * ((size_t)v.npc + 1) + 64 + (size_t)v.ntables * 256 > 150 * 1024;
  L.inl = inl && !L.big; L.jl = jl && !L.big; L.direct = direct && !L.big;
  L.cshift = v.C <= 64 ? 0u : 2u;
  L.general = L.tblmode || anywide || L.big || L.cshift != 0;
  return 0;
}

// ------------------------------------------------------------------ chooseDelayed: delay K and merge window J of the delayed form
// The delayed form of the stage (kx_delayed.h), where it has one: delay 1 or 2 (KX_DF_K pins it), image of at most 40 KiB; taken when at most
// a quarter of the transitions reachable from the start state are undecided after K symbols — a static guess at "inputs may never
// get there" (apache_log 11 of 304: a backslash before a quote).  A wrong guess is cheap: a lane that escapes leaves at once, the first
// shard is redone by the general engine and the stage stays there (thousand_sep, 1 of 7: the digit count of the whole number decides,
// every input escapes in its first pieces).  KX_DF=0 switches the form off, KX_DF=2 takes it whatever the share.
// Returns "" and the build to run, or why the stage has none (`out` then holds what was built last, for kx_df_describe).
//
// merged constants (kx_delayed.h): a constant waits up to J steps for the next one; where that does not fit (a merged
// constant beyond 125 bytes, a table beyond the budget) the stage is built without.
// Every step of window multiplies the states by the constants that may be due (apache_log: 145 product states without, 161 / 178 /
// 273 / 338 at J = 1 / 2 / 6 / 8), and k_dforward keeps TWO blocks of 512 lanes per CU only while image + 64 KiB of record staging
// <= 80 KiB (one block: 3.0 -> 3.4-3.9 ms, profiles/r06_experiments.md): by default the largest window whose image still fits;
// kx_config::merge_window pins it.
inline std::string buildWindowed(const kxdf::DfInput& di, const kx_config& cfg, uint32_t K, kxdf::DfBuild& b) {
  std::string w = "-";
  if (cfg.merge_window) { const uint32_t J = cfg.merge_window - 1; if (J) w = kxdf::buildDelayed(di, K, J, 40 * 1024, b); }
  else
    for (uint32_t J : {8u, 6u, 4u, 3u, 2u, 1u}) {
      b = kxdf::DfBuild();
      w = kxdf::buildDelayed(di, K, J, 40 * 1024, b);
      if (w.empty() && !b.capped && b.img.size() * 4 + 64 * 1024 <= 80 * 1024) break;
      w = "-";
    }
  if (!w.empty() || b.capped) { b = kxdf::DfBuild(); w = kxdf::buildDelayed(di, K, 0, 40 * 1024, b); }
  return w;
}
inline std::string chooseDelayed(const kxdf::DfInput& di, const kx_config& cfg, kxdf::DfBuild& out) {
  if (cfg.delayed_form == 1) return "switched off (kx_config::delayed_form = 1)";
  auto acceptable = [&](const kxdf::DfBuild& b) { return (uint64_t)b.nesc_start * 4 <= (uint64_t)b.ntrans_start || cfg.delayed_form == 2; };
  // The delay: the smallest that leaves no start-reachable transition undecided — a resolved value waits in the state until its
  // turn, so every further symbol of delay multiplies the states by the kinds of output (csv2json and iso_datetime_to_json need
  // one symbol, apache_log two) — else 2; KX_DF_K pins it
  std::string why;
  if (cfg.delay == 1 || cfg.delay == 2) why = buildWindowed(di, cfg, cfg.delay, out);
  else {
    kxdf::DfBuild b1, b2;
    const std::string w1 = buildWindowed(di, cfg, 1, b1);
    if (w1.empty() && b1.nesc_start == 0) { out = std::move(b1); why = w1; }
    else {
      const std::string w2 = buildWindowed(di, cfg, 2, b2);
      if (w2.empty() && (acceptable(b2) || !w1.empty() || !acceptable(b1))) { out = std::move(b2); why = w2; }
      else { out = std::move(b1); why = w1; }
    }
  }
  if (why.empty() && !acceptable(out)) why = "too many contexts that need more lookahead";
  if (why.empty() && !dfRecFits(out.img.data(), out.nP + 2, di.C)) why = "the table image outgrows the piece record's fields";
  return why;
}

// ------------------------------------------------------------------ packEntries: the back entries in the chosen layout
// Compact entry: see DevTables.  Actions: one id per distinct path constant that some entry appends (id 0 = no constant); the
// output stage gets a constant's place and length from adesc[id].
struct Entries {
  const StageView& v; const Pool& pool; const Layout& L;
  std::vector<uint32_t> ent, wlen, rowoff, adesc{0, 0}, aid_of;
  uint32_t nullrow_idx = 0, max_const_len = 0;   // first word of the identity row; longest constant any path entry appends
  bool too_many_actions = false;
  Entries(const StageView& v_, const Pool& p_, const Layout& L_) : v(v_), pool(p_), L(L_), rowoff(v_.nback), aid_of(v_.npc, 0) {}
  uint32_t action(uint32_t pc, uint32_t clen) {
    if (!aid_of[pc]) { aid_of[pc] = (uint32_t)adesc.size() / 2; adesc.push_back(pool.off[pc]); adesc.push_back(clen); }
    return aid_of[pc];
  }
  void push(uint32_t parent, uint32_t copy, uint32_t dlen, uint32_t pc, uint32_t tb = 0) {
    const uint32_t head = (copy ? 0u : 1u) | (parent << 2), clen = dlen - copy;
    if (clen > max_const_len && !(L.inl && clen == 1)) max_const_len = clen;
    wlen.push_back(dlen);
    if (L.jl) { ent.push_back(head | (clen ? ((pool.off[pc] >> 4) << 10) | (4u << 16) : 0u) | (dlen << 24)); return; }
    if (L.inl && clen == 1) { ent.push_back(head | ((uint32_t)v.pcpool[v.pcoff[pc]] << 16) | (dlen << 24)); return; }
    uint32_t aid = clen ? action(pc, clen) : 0;
    if (L.inl) {
      if (aid >= (1u << 12)) too_many_actions = true;
      ent.push_back(head | 0x8000u | ((aid & 0x1Fu) << 10) | (((aid >> 5) & 0x7Fu) << 16) | (clen ? 1u << 23 : 0u) | (dlen << 24));
      return;
    }
    if (clen && L.direct) aid = pool.off[pc] >> 4;
    if (aid >= (L.tblmode ? 1u << 10 : 1u << 13)) too_many_actions = true;
    ent.push_back(head | ((aid & 0x1FFFu) << 10) | (L.tblmode ? (tb & 7u) << 20 : 0u) | (clen ? 1u << 23 : 0u) | ((dlen >= 127 ? 127u : dlen) << 24));
  }
  void padRow() { while (ent.size() % (L.big ? 4u : 1u)) push(0, 0, 0, 0); }
};
// bit 1 of an entry: its parent leaf p is a fixed point of the SAME row whose entry only copies the input byte.  In a
// run of identical transitions (a self-loop taken repeatedly) everything below such a step is then known without
// looking: the leaf stays p and every step appends exactly its input byte.
inline void markFixedPoints(Entries& E) {
  const StageView& v = E.v;
  for (uint32_t b = 0; b < v.nback; ++b) {
    const uint32_t rl = (b + 1 < v.nback ? E.rowoff[b + 1] : (uint32_t)E.ent.size()) - E.rowoff[b];
    for (uint32_t j = 0; j < rl && j < v.Lm; ++j) {
      uint32_t& e = E.ent[E.rowoff[b] + j];
      if (v.back[(size_t)b * v.Lm + j] == KXP_DEAD_LEAF) continue;
      const uint32_t pl = (e >> 2) & 0xFFu;
      if (pl >= rl || pl >= v.Lm || v.back[(size_t)b * v.Lm + pl] == KXP_DEAD_LEAF) continue;
      const uint32_t ep = E.ent[E.rowoff[b] + pl];
      if (!E.L.inl && ((ep >> 2) & 0xFFu) == pl && (ep & 1u) == 0 && ((ep >> (E.L.jl ? 18 : 23)) & 1u) == 0 && (ep >> 24) == 1u) e |= 2u;
    }
  }
}
inline int packEntries(Entries& E, std::string& err) {
  const StageView& v = E.v;
  for (uint32_t b = 0; b < v.nback; ++b) {
    E.padRow();
    E.rowoff[b] = (uint32_t)E.ent.size();
    for (uint32_t j = 0, rl = v.rowLen(b); j < rl; ++j) {
      const uint32_t e = v.back[(size_t)b * v.Lm + j];
      if (e == KXP_DEAD_LEAF) { E.push(0, 0, 0, 0); continue; }
      if (v.dlen(e) >= (1u << 23)) return fail(err, KX_E_BLOB, "path constant too long");
      E.push(e & 0xFF, (e >> 8) & 1, v.dlen(e), v.pcOf(e), v.tbOf(e));
    }
  }
  if (E.too_many_actions) return fail(err, KX_E_BLOB, E.L.inl ? "internal: inline-constant layout with more than 4095 longer constants (KX_INL=0 loads the program)" : E.L.tblmode ? "program outside engine limits (more than 1023 distinct path constants beside symbol tables)" : "program has more than 8191 distinct path constants");
  markFixedPoints(E);
  // identity row (parent = leaf, nothing appended): steps past the end of a partial piece point here;
  // a second, all-zero row pads the table so that a probe on a dead path stays inside it
  E.padRow();
  E.nullrow_idx = (uint32_t)E.ent.size();
  for (uint32_t j = 0; j < v.Lm; ++j) E.push(j, 0, 0, 0);
  for (uint32_t j = 0; j < v.Lm; ++j) E.push(0, 0, 0, 0);
  return 0;
}

// ------------------------------------------------------------------ buildImage: what the general engine's kernels read
// k_forward's pair table (two symbols per lookup; see piece_run_pair) when it fits LDS behind the state table
inline std::vector<uint16_t> buildPairTable(const StageView& v, const Layout& L, const kx_config& cfg, uint32_t off_ent, uint32_t& pair_magic) {
  std::vector<uint16_t> pairtab;
  const uint32_t C = v.C, nstates = v.nstates;
  const uint64_t CC = (uint64_t)C * C, rows = (uint64_t)nstates + 1;
  bool ok = !L.general && !(cfg.disable & KX_OFF_PAIR) && rows * CC <= 65535 && off_ent <= PAIR_CLS2_AT && C <= 63;
  pair_magic = 0;
  if (ok) {
    pair_magic = (uint32_t)((1ull << 32) / CC) + 1;
    for (uint64_t q = 0; q < rows && ok; ++q) ok = (uint32_t)((q * CC * pair_magic) >> 32) == q;
  }
  if (!ok) return pairtab;
  pairtab.assign((rows * CC + 1) & ~(uint64_t)1, (uint16_t)(nstates * CC));
  for (uint32_t q = 0; q < nstates; ++q)
    for (uint32_t c1 = 0; c1 < C; ++c1) {
      const uint16_t d1 = v.delta[(size_t)q * C + c1];
      if (d1 == KXP_NO_STATE) continue;
      for (uint32_t c2 = 0; c2 < C; ++c2) {
        const uint16_t d2 = v.delta[(size_t)d1 * C + c2];
        if (d2 != KXP_NO_STATE) pairtab[((size_t)q * C + c1) * C + c2] = (uint16_t)(d2 * CC);
      }
    }
  return pairtab;
}
// synchronising automaton, renumbered: undecided subsets first, decided ones absorbing; one extra
// absorbing row stands for "subset construction was capped here"
inline std::vector<uint16_t> buildSync16(const StageView& v, uint32_t& nmulti) {
  const uint32_t nsync = v.nsync, C = v.C;
  std::vector<uint32_t> newid(nsync);
  nmulti = 0;
  for (uint32_t i = 0; i < nsync; ++i) if (v.sync_state[i] == KXP_SYNC_MULTI) newid[i] = nmulti++;
  { uint32_t t = nmulti; for (uint32_t i = 0; i < nsync; ++i) if (v.sync_state[i] != KXP_SYNC_MULTI) newid[i] = t++; }
  std::vector<uint16_t> sync16(((size_t)(nsync + 1) * (C + 1) + 1) & ~(size_t)1, 0);
  for (uint32_t i = 0; i < nsync; ++i) {
    const bool multi = v.sync_state[i] == KXP_SYNC_MULTI;
    for (uint32_t k = 0; k < C; ++k) {
      uint32_t nx = v.sync_next[(size_t)i * C + k];
      sync16[(size_t)newid[i] * C + k] = (uint16_t)(!multi ? newid[i] : nx == KXP_SYNC_UNKNOWN ? nsync : newid[nx]);
    }
    uint32_t st = v.sync_state[i];
    sync16[(size_t)(nsync + 1) * C + newid[i]] = (uint16_t)(st == KXP_SYNC_MULTI ? 0xFFFF : st == KXP_SYNC_EMPTY ? 0xFFFE : st);
  }
  for (uint32_t k = 0; k < C; ++k) sync16[(size_t)nsync * C + k] = (uint16_t)nsync;
  sync16[(size_t)(nsync + 1) * C + nsync] = 0xFFFD;
  return sync16;
}

struct GeneralImage {
  Layout L; DevTables T{};                 // (pointer fields: byte offsets into `bytes`)
  std::vector<uint8_t> bytes;              // one device allocation: packed | cls | nleaves | fin_leaf | sync16 | init_off | init_len | wlen | pair
  size_t lds_bytes = 0, sync_lds_bytes = 0;   // packed table image (0: BIG, read from global memory); 0 = sync tables stay in global memory
  uint32_t max_const_len = 0;
};
// LDS image: cls4 (256 B, at LDS address 0: the hand-scheduled sweeps read it with no base) | fwd | ent | pool | adesc | symbol tables
inline int buildPacked(const StageView& v, const Pool& pool, const Entries& E, DevTables& T, std::vector<uint32_t>& packed, std::string& err) {
  const Layout& L = E.L;
  const uint32_t C = v.C, nstates = v.nstates, off_ent = OFF_FWD + (nstates + 1) * C * 4;
  if (!L.big && (size_t)off_ent + E.ent.size() * 4 > 65532) return fail(err, KX_E_BLOB, "internal: table sizing");
  if (L.big && E.ent.size() * 4 > 0xFFFF0u) return fail(err, KX_E_BLOB, "program outside engine limits (path table > 1 MiB)");
  T.hshift = L.big ? 2u : 0u; T.rshift = L.big ? 4u : 0u; T.rbase = L.big ? off_ent : 0u;
  T.off_fwd = OFF_FWD; T.off_ent = off_ent; T.off_cls = 0;
  T.deadh = (OFF_FWD + nstates * C * 4) >> T.hshift;    // handle of the absorbing "no transition" state
  T.q0h = (OFF_FWD + v.q0 * C * 4) >> T.hshift;
  auto rowHandle = [&](uint32_t row_word) { return L.big ? (row_word * 4) >> 4 : off_ent + row_word * 4; };
  T.nullrow = rowHandle(E.nullrow_idx);
  packed.assign(OFF_FWD / 4 + (size_t)(nstates + 1) * C, 0);
  for (int b = 0; b < 256; ++b) ((uint8_t*)packed.data())[b] = (uint8_t)(L.cshift ? v.cls[b] : v.cls[b] * 4);
  uint32_t* fwd = packed.data() + OFF_FWD / 4;
  for (size_t i = 0; i < v.sc(); ++i)
    fwd[i] = v.delta[i] == KXP_NO_STATE ? T.deadh : (((OFF_FWD + (uint32_t)v.delta[i] * C * 4) >> T.hshift) | (rowHandle(E.rowoff[v.pback[i]]) << 16));
  for (uint32_t k = 0; k < C; ++k) fwd[v.sc() + k] = T.deadh;
  packed.insert(packed.end(), E.ent.begin(), E.ent.end());
  packed.resize((packed.size() + 3) & ~(size_t)3, 0);               // the pool starts on a 16-byte boundary of the image
  T.off_pool = (uint32_t)packed.size() * 4;
  packed.resize(packed.size() + pool.bytes.size() / 4, 0);
  memcpy((char*)packed.data() + T.off_pool, pool.bytes.data(), pool.bytes.size());
  T.off_adesc = (uint32_t)packed.size() * 4; T.naid = (uint32_t)E.adesc.size() / 2;
  packed.insert(packed.end(), E.adesc.begin(), E.adesc.end());
  packed.resize((packed.size() + 3) & ~(size_t)3, 0);
  T.off_tbl = (uint32_t)packed.size() * 4;
  if (v.ntables) { packed.resize(packed.size() + (size_t)v.ntables * 64, 0); memcpy((char*)packed.data() + T.off_tbl, v.tables, (size_t)v.ntables * 256); }
  if (!L.big && packed.size() * 4 > 150 * 1024) return fail(err, KX_E_BLOB, "internal: table sizing (LDS budget)");
  T.packed_words = (uint32_t)packed.size(); T.stage_words = L.big ? 0u : T.packed_words;
  return 0;
}
// the general engine's image of a stage in the layout chooseLayout picks (`alt`: the job-stride alternative)
inline int buildGeneral(const StageView& v, const Pool& pool, const kx_config& cfg, bool alt, GeneralImage& G, std::string& err) {
  int rc = chooseLayout(v, cfg, alt, G.L, err);
  if (rc) return rc;
  const Layout& L = G.L;
  Entries E(v, pool, L);
  if ((rc = packEntries(E, err))) return rc;
  DevTables& T = G.T;
  std::vector<uint32_t> packed;
  if ((rc = buildPacked(v, pool, E, T, packed, err))) return rc;
  const std::vector<uint16_t> pairtab = buildPairTable(v, L, cfg, T.off_ent, T.pair_magic);
  G.lds_bytes = L.big ? 0 : packed.size() * 4;            // a BIG image is read from global memory (L2), nothing is staged
  G.max_const_len = E.max_const_len;
  if (v.nsync == 0 || v.nsync >= 0xFFF0) return fail(err, KX_E_BLOB, "bad synchronising automaton");
  const std::vector<uint16_t> sync16 = buildSync16(v, T.sync_multi);
  const size_t sync_bytes = sync16.size() * 2, nstates = v.nstates, Lm = v.Lm;
  G.sync_lds_bytes = sync_bytes + 256 <= 64 * 1024 ? sync_bytes + 256 : 0;
  const size_t o_packed = 0, o_cls = o_packed + al256(packed.size() * 4), o_nl = o_cls + 256, o_fl = o_nl + al256(nstates + 1),
               o_sn = o_fl + al256(nstates + 1), o_io = o_sn + al256(sync_bytes), o_il = o_io + al256(Lm * 4), o_wl = o_il + al256(Lm * 4),
               o_pr = o_wl + al256(E.wlen.size() * 4), total = o_pr + al256(pairtab.size() * 2);
  std::vector<uint8_t>& img = G.bytes;
  img.assign(total, 0);
  memcpy(&img[o_packed], packed.data(), packed.size() * 4);
  memcpy(&img[o_cls], v.cls, 256);
  memcpy(&img[o_nl], v.nleaves, nstates); img[o_nl + nstates] = 1;
  memcpy(&img[o_fl], v.fin_leaf, nstates); img[o_fl + nstates] = KXP_NO_LEAF;
  memcpy(&img[o_sn], sync16.data(), sync_bytes);
  for (uint32_t j = 0; j < Lm; ++j) {
    const uint32_t off = pool.off[v.init_const[j]], len = v.clen(v.init_const[j]);
    memcpy(&img[o_io + 4 * j], &off, 4); memcpy(&img[o_il + 4 * j], &len, 4);
  }
  memcpy(&img[o_wl], E.wlen.data(), E.wlen.size() * 4);
  if (!pairtab.empty()) memcpy(&img[o_pr], pairtab.data(), pairtab.size() * 2);
  setOff(T.packed, o_packed); setOff(T.pair, o_pr); setOff(T.wlen, o_wl); setOff(T.cls, o_cls); setOff(T.nleaves, o_nl); setOff(T.fin_leaf, o_fl);
  setOff(T.sync16, o_sn); setOff(T.init_off, o_io); setOff(T.init_len, o_il);
  T.pair_words = (uint32_t)(pairtab.size() / 2);
  T.nstates = v.nstates; T.nclasses = v.C; T.maxleaves = v.Lm; T.cshift = L.cshift; T.big = L.big ? 1u : 0u;
  T.nsync = v.nsync; T.sync_words = (uint32_t)(sync_bytes / 4);
  T.xlat = L.xlat_tb ? T.off_tbl + ((L.xlat_tb - 1) << 8) : 0u; T.tblmode = L.tblmode ? 1u : 0u; T.aid_mask = L.tblmode ? 0x3FFu : 0x1FFFu;
  T.inl = L.inl ? 1u : 0u; T.jl = L.jl ? 1u : 0u; T.direct = L.direct ? 1u : 0u;
  T.short_consts = E.max_const_len <= 16 && !(cfg.disable & KX_OFF_CMPX) ? 1u : 0u;
  T.debug = cfg.debug_flags;
  return 0;
}

// ------------------------------------------------------------------ buildDelayedImage: what the delayed form's kernels read
// the exact slow path's tables (kx_dfkernels.inc: `slow`): the blob's own path form + what every product state owes
inline void buildSlowTables(const StageView& v, const kxdf::DfBuild& df, DfDev& D, std::vector<uint8_t>& sl) {
  const uint32_t nP = df.nP, K = df.K, Lm = v.Lm;
  const size_t sc = v.sc();
  std::vector<uint32_t> pend((size_t)nP * K * Lm, 0), defoff(nP + 1, 0), defpc;
  std::vector<uint16_t> stq(nP);
  for (uint32_t i = 0; i < nP; ++i) {
    const kxdf::DfState& st = df.states[i];
    stq[i] = (uint16_t)st.q;
    for (uint32_t j = 0; j < K; ++j)
      for (uint32_t l = 0; l < Lm; ++l) pend[((size_t)i * K + j) * Lm + l] = st.pend[j].size() == 1 ? st.pend[j][0] : l < st.pend[j].size() ? st.pend[j][l] : st.pend[j][0];
    for (const auto& d : st.def) defpc.push_back(d.first);
    defoff[i + 1] = (uint32_t)defpc.size();
  }
  defpc.push_back(0);
  // per transition, 48 bytes fetched as one: {next state (0xFFFF: none) | its leaves << 16, backward row, 0, 0} + the parent leaf of each of its ≤ 32 leaves
  std::vector<uint32_t> fwd2(sc * 12, 0xFFFFFFFFu);
  for (size_t i = 0; i < sc; ++i) {
    uint32_t* f = &fwd2[12 * i];
    f[2] = f[3] = 0;
    if (v.delta[i] == KXP_NO_STATE) { f[0] = 0xFFFFu; f[1] = 0; continue; }
    f[0] = (uint32_t)v.delta[i] | ((uint32_t)v.nleaves[v.delta[i]] << 16); f[1] = v.pback[i];
    uint8_t* par = (uint8_t*)(f + 4);
    for (uint32_t l = 0; l < v.nleaves[v.delta[i]] && l < 32; ++l) { const uint32_t e = v.back[(size_t)v.pback[i] * Lm + l]; par[l] = e == KXP_DEAD_LEAF ? 0xFF : (uint8_t)(e & 0xFF); }
  }
  const size_t o_delta = 0, o_back = o_delta + al256(sc * 48), o_pcoff = o_back + al256(v.nent() * 4),
               o_pool = o_pcoff + al256(((size_t)v.npc + 1) * 4), o_pend = o_pool + al256(v.pcpl + 16), o_doff = o_pend + al256(pend.size() * 4),
               o_dpc = o_doff + al256(defoff.size() * 4), o_q = o_dpc + al256(defpc.size() * 4), tot = o_q + al256((size_t)nP * 2);
  sl.assign(tot, 0);
  memcpy(&sl[o_delta], fwd2.data(), sc * 48); memcpy(&sl[o_back], v.back, v.nent() * 4);
  memcpy(&sl[o_pcoff], v.pcoff, ((size_t)v.npc + 1) * 4); memcpy(&sl[o_pool], v.pcpool, v.pcpl);
  memcpy(&sl[o_pend], pend.data(), pend.size() * 4); memcpy(&sl[o_doff], defoff.data(), defoff.size() * 4);
  memcpy(&sl[o_dpc], defpc.data(), defpc.size() * 4); memcpy(&sl[o_q], stq.data(), (size_t)nP * 2);
  setOff(D.sl_fmap, o_delta); setOff(D.sl_back, o_back); setOff(D.sl_pcoff, o_pcoff); setOff(D.sl_pcpool, o_pool); setOff(D.sl_pend, o_pend);
  setOff(D.sl_defoff, o_doff); setOff(D.sl_defpc, o_dpc); setOff(D.sl_q, o_q);
  D.sl_Lm = Lm; D.sl_npc = v.npc; D.sl_on = 1;
}
// `T`: the stage's main general image (its handle shift, and the three tables the slow path shares with it)
inline void buildDelayedImage(const StageView& v, const kxdf::DfBuild& df, const kx_config& cfg, const DevTables& T, DfDev& D,
                              std::vector<uint8_t>& img, std::vector<uint8_t>& slow) {   // img: image | start_of_state
  const size_t ib = al256(df.img.size() * 4);
  img.assign(ib + (size_t)v.nstates * 2 + 16, 0);
  memcpy(img.data(), df.img.data(), df.img.size() * 4);
  memcpy(img.data() + ib, df.start_of_state.data(), (size_t)v.nstates * 2);
  D = DfDev{};
  setOff(D.img, 0); D.words = (uint32_t)df.img.size(); setOff(D.start_of_state, ib);
  D.off_pool = df.off_pool; D.deadh = df.deadh; D.esch = df.esch; D.starth = df.starth; D.K = df.K; D.C = v.C;
  D.orig_c4 = v.C * 4; D.hshift = T.hshift; D.nstates = v.nstates; D.J = df.J;
  uint32_t mx = 0; for (uint32_t pc = 0; pc < v.npc; ++pc) mx = v.clen(pc) > mx ? v.clen(pc) : mx;
  D.short_consts = mx <= 16 && !(cfg.disable & KX_OFF_CMPX) ? 1u : 0u; D.debug = T.debug; D.wide = df.wide ? 1u : 0u;
  if (v.Lm <= 32 && !(cfg.disable & KX_OFF_SLOW)) {
    buildSlowTables(v, df, D, slow);
    D.sl_nleaves = T.nleaves; D.sl_fin_leaf = T.fin_leaf; D.sl_cls = T.cls;
  }
}

// ------------------------------------------------------------------ buildStage: all of the above for one stage of a blob
struct HostStage {
  uint32_t nstates = 0, nclasses = 0, q0 = 0, maxleaves = 1;
  std::vector<uint8_t> h_nleaves, h_fin_leaf;          // host copies for the control path
  std::vector<uint32_t> h_init_off, h_init_len;
  std::vector<uint8_t> h_pool;
  DevTables T{};
  size_t lds_bytes = 0;                                // packed table image
  size_t sync_lds_bytes = 0;                           // 0 = sync tables stay in global memory
  uint32_t max_const_len = 0;                          // longest constant any path entry appends
  bool general = false;                                   // wide back entries or > 64 byte classes: run the GENERAL kernel instances
  bool big = false;                                       // image in global memory, scaled handles (DevTables::big); implies general
  uint32_t handleOf(uint32_t state) const { return (OFF_FWD + state * nclasses * 4) >> (big ? 2 : 0); }
  uint32_t stateOf(uint32_t handle) const { return ((handle << (big ? 2 : 0)) - OFF_FWD) / (nclasses * 4); }
  bool act = false; uint32_t act_regs = 0;                // the stage's output is a token stream: action post-pass with that many registers
  DevTables Talt{}; bool has_alt = false;                 // the job-stride alternative (kx_engine.hip: Stage has the why)
  kxdf::DfBuild df; DfDev D{}; bool has_df = false;       // the delayed form (kx_delayed.h)
  std::vector<uint32_t> df_pc_off, df_pc_len;   // per path constant: offset in h_pool, length (the host writes a shard's tail)
  std::string df_why;                            // why the stage has no delayed form ("" if it has one)
  // the bytes to upload: T / Talt / D.img / D.sl_* point into them by offset until they are on the device
  std::vector<uint8_t> img, img_alt, img_df, img_slow;
};
enum : unsigned { WITH_ALT = 1u, WITH_DELAYED = 2u };
// The job-stride layout wins where a piece holds many constants and loses where it holds few — a property of the DATA — so a stage
// that qualifies for it and whose configuration pins nothing keeps BOTH images (kx_engine.hip: Stage::use_alt).
inline void buildAlternative(const StageView& v, const Pool& pool, const kx_config& cfg, HostStage& S) {
  if (cfg.job_stride != 0 || S.general || S.big || S.T.inl || S.T.xlat || S.T.jl) return;
  GeneralImage alt; std::string ignored;
  if (buildGeneral(v, pool, cfg, true, alt, ignored) || !alt.T.jl || alt.lds_bytes > S.lds_bytes || alt.L.general) return;
  S.Talt = alt.T; S.img_alt = std::move(alt.bytes); S.has_alt = true;
}
// `what`: WITH_ALT, WITH_DELAYED — kx_validate wants neither, the kx_df_* probes no alternative; c moves behind the stage
inline int buildStage(const uint8_t*& c, const uint8_t* end, const kx_config& cfg, unsigned what, HostStage& S, std::string& err) {
  StageView v;
  int rc = readStage(c, end, v, err);
  if (rc) return rc;
  const Pool pool = buildPool(v);
  GeneralImage G;
  if ((rc = buildGeneral(v, pool, cfg, false, G, err))) return rc;
  S.nstates = v.nstates; S.nclasses = v.C; S.q0 = v.q0; S.maxleaves = v.Lm; S.act = v.act(); S.act_regs = v.actRegs();
  S.T = G.T; S.img = std::move(G.bytes); S.lds_bytes = G.lds_bytes; S.sync_lds_bytes = G.sync_lds_bytes; S.max_const_len = G.max_const_len;
  S.general = G.L.general; S.big = G.L.big;
  S.h_nleaves.assign(v.nleaves, v.nleaves + v.nstates); S.h_nleaves.push_back(1);
  S.h_fin_leaf.assign(v.fin_leaf, v.fin_leaf + v.nstates); S.h_fin_leaf.push_back(KXP_NO_LEAF);
  S.h_pool = pool.bytes;
  S.h_init_off.resize(v.Lm); S.h_init_len.resize(v.Lm);
  for (uint32_t j = 0; j < v.Lm; ++j) { S.h_init_off[j] = pool.off[v.init_const[j]]; S.h_init_len[j] = v.clen(v.init_const[j]); }
  S.df_pc_off.assign(pool.off.begin(), pool.off.begin() + v.npc); S.df_pc_len.resize(v.npc);
  for (uint32_t pc = 0; pc < v.npc; ++pc) S.df_pc_len[pc] = v.clen(pc);
  if (what & WITH_ALT) buildAlternative(v, pool, cfg, S);
  if (what & WITH_DELAYED) {
    const kxdf::DfInput di{v.nstates, v.C, v.q0, v.Lm, v.nback, v.npc, v.cls, v.delta, v.pback, v.nleaves, v.back, v.pcoff, v.pcpool, v.init_const,
                           pool.off.data(), pool.bytes.data(), (uint32_t)pool.bytes.size(), v.has_tbl};
    S.df_why = chooseDelayed(di, cfg, S.df);
    S.has_df = S.df_why.empty();
    if (S.has_df) buildDelayedImage(v, S.df, cfg, S.T, S.D, S.img_df, S.img_slow);
  }
  return 0;
}

// kx_stage_describe_cfg's report (include/kxhip.h): the decision, and the structs with their pointer fields as the offsets they still are
inline void describeStage(const HostStage& S, uint32_t which, kx_stage_info& I) {
  const std::vector<uint8_t>& bytes = which == KX_STAGE_MAIN ? S.img : which == KX_STAGE_ALT ? S.img_alt : which == KX_STAGE_DELAYED ? S.img_df : S.img_slow;
  const DevTables& T = which == KX_STAGE_ALT && S.has_alt ? S.Talt : S.T;
  const DfDev& D = S.D;
  I = kx_stage_info{};
  I.size = sizeof I; I.which = which; I.image_bytes = bytes.size();
  I.general = S.general; I.big = S.big; I.has_alt = S.has_alt; I.has_df = S.has_df; I.actions = S.act; I.action_regs = S.act_regs;
  I.max_const_len = S.max_const_len; I.lds_bytes = S.lds_bytes; I.sync_lds_bytes = S.sync_lds_bytes;
#define KX_T(f) I.t.f = T.f
#define KX_TO(f) I.t.f = offOf(T.f)
  KX_TO(packed); KX_TO(pair); KX_TO(wlen); KX_TO(cls); KX_TO(nleaves); KX_TO(fin_leaf); KX_TO(sync16); KX_TO(init_off); KX_TO(init_len);
  KX_T(packed_words); KX_T(off_fwd); KX_T(off_ent); KX_T(off_pool); KX_T(off_cls); KX_T(off_adesc); KX_T(naid); KX_T(nstates); KX_T(nclasses);
  KX_T(q0h); KX_T(maxleaves); KX_T(deadh); KX_T(nullrow); KX_T(cshift); KX_T(debug); KX_T(big); KX_T(hshift); KX_T(rshift); KX_T(rbase);
  KX_T(stage_words); KX_T(pair_words); KX_T(pair_magic); KX_T(nsync); KX_T(sync_multi); KX_T(sync_words); KX_T(off_tbl); KX_T(xlat);
  KX_T(tblmode); KX_T(aid_mask); KX_T(inl); KX_T(jl); KX_T(direct); KX_T(short_consts);
#undef KX_T
#undef KX_TO
#define KX_D(f) I.d.f = D.f
#define KX_DO(f) I.d.f = offOf(D.f)
  KX_DO(img); KX_DO(start_of_state); KX_DO(sl_fmap); KX_DO(sl_back); KX_DO(sl_nleaves); KX_DO(sl_fin_leaf); KX_DO(sl_cls); KX_DO(sl_pcoff);
  KX_DO(sl_pcpool); KX_DO(sl_pend); KX_DO(sl_defoff); KX_DO(sl_defpc); KX_DO(sl_q);
  KX_D(words); KX_D(off_pool); KX_D(deadh); KX_D(esch); KX_D(starth); KX_D(K); KX_D(C); KX_D(orig_c4); KX_D(hshift); KX_D(short_consts);
  KX_D(debug); KX_D(nstates); KX_D(J); KX_D(wide); KX_D(sl_Lm); KX_D(sl_npc); KX_D(sl_on);
#undef KX_D
#undef KX_DO
}

}  // namespace kxst
#endif
