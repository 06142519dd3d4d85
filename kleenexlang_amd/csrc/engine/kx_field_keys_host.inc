// kx_field_keys_host.inc — field mode by key (kx_run_batch_field_keys, include/kxhip.h; kernels in kx_field_keys.inc).  Included
// at the end of kx_engine.hip between kx_field_project_host.inc, whose rules and the files' before it it applies, and
// kx_records_host.inc.  The driver is kx_field_list_host.inc's runFieldList with `keyed` set.  Here: the rules of a kx_field_keys
// (the byte rules are kx_field_keys.h's, which the command line applies too), the names' table, and the entry point.

#include "kx_field_keys.h"

namespace {

// the rules of a kx_field_keys (`who`) beside the framing of its list, found before any device work; rsep: the one-byte record
// separator, or -1 (the batch call knows none)
int checkFieldKeys(const kx_field_keys& k, const kx_batch_field_list& l, int rsep, const char* who) {
  auto no = [&](const std::string& what) { return setErr(KX_E_ARG, std::string(who) + ": " + what); };
  if (k.size != sizeof(kx_field_keys)) return no("kx_field_keys::size is not this library's");
  if (k.n_names < 1 || k.n_names > KX_FIELD_ITEMS) return no("a key list has 1 to 16 names");
  if (k.pad[0] || k.pad[1] || k.pad[2]) return no("reserved words must be 0");
  for (uint32_t r : k.reserved) if (r) return no("reserved words must be 0");
  if (k.flags & ~KX_KEYS_WORDS) return no("unknown flag bits");
  if (k.optional_mask >> k.n_names) return no("optional_mask has a bit at or above n_names");
  const bool words = (k.flags & KX_KEYS_WORDS) != 0;
  if (const char* clash = kxFieldKeyByteClash(k.kv, words ? -1 : (int)l.fs, words, rsep, l.quote, l.escape))
    return no(std::string("the key separator cannot be ") + clash);
  for (uint32_t t = 0; t < k.n_names; ++t) {
    if (!k.names[t]) return no("a null name pointer");
    if (k.name_len[t] < 1 || k.name_len[t] > KX_FIELD_NAME_MAX) return no("a name has 1 to 255 bytes");
    if (const char* clash = kxFieldKeyNameClash(k.names[t], k.name_len[t], k.kv, words ? -1 : (int)l.fs, words, rsep))
      return no(std::string("a name cannot hold ") + clash);
    for (uint32_t u = 0; u < t; ++u)
      if (k.name_len[u] == k.name_len[t] && memcmp(k.names[u], k.names[t], k.name_len[t]) == 0) return no("two names are equal");
  }
  return 0;
}

// the rules of the projection of a keyed call: its items are names
int checkKeyedProject(const kx_field_project& pr, const kx_field_keys& k, const kx_batch_field_list& l, const kx_field_codec* codec, const char* who) {
  auto no = [&](const char* what) { return setErr(KX_E_ARG, std::string(who) + ": " + what); };
  if (pr.size != sizeof(kx_field_project)) return no("kx_field_project::size is not this library's");
  if (pr.n_items < 1 || pr.n_items > KX_FIELD_ITEMS) return no("a projection has 1 to 16 items");
  for (uint32_t t = 0; t < pr.n_items; ++t)
    if (pr.items[t].lo != 0 || pr.items[t].hi >= k.n_names) return no("with keys an item is {0, the index of a name}");
  if (pr.ofs_len > 8) return no("the output field separator is at most 8 bytes");
  if (pr.flags & ~KX_PROJECT_WORDS) return no("unknown flag bits");
  for (uint32_t r : pr.reserved) if (r) return no("reserved words must be 0");
  if (codec) {
    if (pr.ofs_len != 1) return no("with a codec the output field separator is exactly one byte");
    if ((int)pr.ofs[0] == l.quote || (int)pr.ofs[0] == l.escape) return no("the output field separator cannot be the quote or the escape byte");
    for (uint32_t i = 0; i < codec->n_special; ++i) if (pr.ofs[0] == codec->special[i]) return no("the output field separator cannot be a special byte");
  }
  return 0;
}

// the driver's view of a kx_field_keys whose rules have passed
void fillKeyedRun(const kx_field_keys& k, KeyedRun* r) {
  memset(r->tab, 0, sizeof r->tab);
  uint16_t* const tl = reinterpret_cast<uint16_t*>(r->tab);
  uint32_t at = 0;
  for (uint32_t t = 0; t < k.n_names; ++t) {
    tl[t] = (uint16_t)k.name_len[t]; tl[16 + t] = (uint16_t)at;
    memcpy(r->tab + 64 + at, k.names[t], k.name_len[t]);
    at += k.name_len[t];
  }
  r->all = (1u << k.n_names) - 1u;
  r->req = r->all & ~k.optional_mask;
  r->kv = k.kv;
}

// what kx_run_batch_field_keys and the records driver share: the rules, then the driver (rsep: see checkFieldKeys)
int fieldKeysEntry(const char* who, int rsep, kx_program* p, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs,
                   const kx_batch_field_list* l, const kx_field_keys* keys, const kx_field_codec* codec, const kx_field_project* proj, void* d_out,
                   size_t cap, uint64_t* d_out_off, kx_batch_doc* d_docs, uint32_t* d_fail_field, size_t* out_len, kx_batch_stats* stats,
                   void* stream) {
  if (!p || !out_len || !l || !keys) return setErr(KX_E_ARG, "null argument");
  if (keys->size != sizeof(kx_field_keys)) return setErr(KX_E_ARG, std::string(who) + ": kx_field_keys::size is not this library's");
  if (l->size != sizeof(kx_batch_field_list)) return setErr(KX_E_ARG, std::string(who) + ": kx_batch_field_list::size is not this library's");
  if (l->n_ranges != 0) return setErr(KX_E_ARG, std::string(who) + ": kx_batch_field_list::n_ranges must be 0: the names select the fields");
  const bool words = (keys->flags & KX_KEYS_WORDS) != 0;
  kx_batch_field_list one = *l, ll = *l;   // (the framing's own rules are the list's: checked with a list of one field)
  one.n_ranges = 1; one.ranges[0] = kx_field_range{1, 1};
  kx_field_codec cc{};
  if (words) {
    if (const int rc = checkFieldWords(&one, codec, who, &ll, &cc)) return rc;
  } else {
    if (const int rc = checkFieldList(one, who)) return rc;
    if (codec) {
      if (const int rc = checkFieldCodec(*codec, one, who)) return rc;
      cc = *codec;
    }
  }
  ll.n_ranges = 0; ll.ranges[0] = kx_field_range{0, 0};
  if (const int rc = checkFieldKeys(*keys, ll, rsep, who)) return rc;
  if (proj) if (const int rc = checkKeyedProject(*proj, *keys, ll, codec ? &cc : nullptr, who)) return rc;
  KeyedRun kr;
  fillKeyedRun(*keys, &kr);
  return runFieldList(p, d_in, d_in_off, n_docs, &ll, codec ? &cc : nullptr, d_out, cap, d_out_off, d_docs, d_fail_field, out_len, stats, stream, who,
                      words, proj, false, &kr);
}

}  // namespace

extern "C" int kx_run_batch_field_keys(kx_program* p, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_field_list* l,
                                       const kx_field_keys* keys, const kx_field_codec* codec, const kx_field_project* proj, void* d_out, size_t cap,
                                       uint64_t* d_out_off, kx_batch_doc* d_docs, uint32_t* d_fail_field, size_t* out_len, kx_batch_stats* stats,
                                       void* stream) {
  return fieldKeysEntry("kx_run_batch_field_keys", -1, p, d_in, d_in_off, n_docs, l, keys, codec, proj, d_out, cap, d_out_off, d_docs, d_fail_field,
                        out_len, stats, stream);
}
