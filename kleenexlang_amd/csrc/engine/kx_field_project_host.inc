// kx_field_project_host.inc — the projection of field mode (kx_run_batch_field_project, include/kxhip.h; kernels in
// kx_field_project.inc).  Included at the end of kx_engine.hip between kx_field_words_host.inc, whose rules and the two files'
// before it it applies, and kx_records_host.inc.  The driver is kx_field_list_host.inc's runFieldList with `proj` set.  Here: the
// rules of a kx_field_project, and the entry point; kx_run_batch_field_header is the same call with the driver's identity switch.

namespace {

// the rules of a kx_field_project by itself (`who`), found before any device work
int checkFieldProject(const kx_field_project& pr, const char* who) {
  auto no = [&](const char* what) { return setErr(KX_E_ARG, std::string(who) + ": " + what); };
  if (pr.size != sizeof(kx_field_project)) return no("kx_field_project::size is not this library's");
  if (pr.n_items < 1 || pr.n_items > KX_FIELD_ITEMS) return no("a projection has 1 to 16 items");
  if (!kxFieldItemsAreValid(pr.items, pr.n_items)) return no("an item needs lo >= 1 and hi = 0 (open) or hi >= lo");
  if (pr.ofs_len > 8) return no("the output field separator is at most 8 bytes");
  if (pr.flags & ~KX_PROJECT_WORDS) return no("unknown flag bits");
  for (uint32_t r : pr.reserved) if (r) return no("reserved words must be 0");
  return 0;
}

// ... beside its list (whose own rules have passed) and its codec (null, or the one the driver takes: its rules have passed too)
int checkFieldProjectWith(const kx_field_project& pr, const kx_batch_field_list& l, const kx_field_codec* codec, const char* who) {
  auto no = [&](const char* what) { return setErr(KX_E_ARG, std::string(who) + ": " + what); };
  kx_field_range u[KX_FIELD_RANGES] = {};
  uint32_t nu = 0;
  if (kxFieldItemsUnion(pr.items, pr.n_items, u, &nu)) return no("the items' union has more than 8 ranges in its normal form");
  if (nu != l.n_ranges || memcmp(u, l.ranges, nu * sizeof(kx_field_range)) != 0) return no("kx_batch_field_list::ranges is not the normal form of the items' union");
  if (codec) {
    if (pr.ofs_len != 1) return no("with a codec the output field separator is exactly one byte");
    if ((int)pr.ofs[0] == l.quote || (int)pr.ofs[0] == l.escape) return no("the output field separator cannot be the quote or the escape byte");
    for (uint32_t i = 0; i < codec->n_special; ++i) if (pr.ofs[0] == codec->special[i]) return no("the output field separator cannot be a special byte");
  }
  return 0;
}

// what kx_run_batch_field_project and kx_run_batch_field_header (`identity`) share: the rules, then the driver
int fieldProjectEntry(const char* who, bool identity, kx_program* p, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs,
                      const kx_batch_field_list* l, const kx_field_codec* codec, const kx_field_project* proj, void* d_out, size_t cap,
                      uint64_t* d_out_off, kx_batch_doc* d_docs, uint32_t* d_fail_field, size_t* out_len, kx_batch_stats* stats, void* stream) {
  if (!p || !out_len || !l || !proj) return setErr(KX_E_ARG, "null argument");
  if (const int rc = checkFieldProject(*proj, who)) return rc;
  const bool words = (proj->flags & KX_PROJECT_WORDS) != 0;
  kx_batch_field_list ll = *l;
  kx_field_codec cc{};
  if (words) {
    if (const int rc = checkFieldWords(l, codec, who, &ll, &cc)) return rc;
  } else {
    if (const int rc = checkFieldList(*l, who)) return rc;
    if (codec) {
      if (const int rc = checkFieldCodec(*codec, *l, who)) return rc;
      cc = *codec;
    }
  }
  if (const int rc = checkFieldProjectWith(*proj, ll, codec ? &cc : nullptr, who)) return rc;
  return runFieldList(p, d_in, d_in_off, n_docs, &ll, codec ? &cc : nullptr, d_out, cap, d_out_off, d_docs, d_fail_field, out_len, stats, stream, who,
                      words, proj, identity);
}

}  // namespace

extern "C" int kx_run_batch_field_project(kx_program* p, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_field_list* l,
                                          const kx_field_codec* codec, const kx_field_project* proj, void* d_out, size_t cap, uint64_t* d_out_off,
                                          kx_batch_doc* d_docs, uint32_t* d_fail_field, size_t* out_len, kx_batch_stats* stats, void* stream) {
  return fieldProjectEntry("kx_run_batch_field_project", false, p, d_in, d_in_off, n_docs, l, codec, proj, d_out, cap, d_out_off, d_docs, d_fail_field,
                           out_len, stats, stream);
}

extern "C" int kx_run_batch_field_header(kx_program* p, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_field_list* l,
                                         const kx_field_codec* codec, const kx_field_project* proj, void* d_out, size_t cap, uint64_t* d_out_off,
                                         kx_batch_doc* d_docs, uint32_t* d_fail_field, size_t* out_len, kx_batch_stats* stats, void* stream) {
  return fieldProjectEntry("kx_run_batch_field_header", true, p, d_in, d_in_off, n_docs, l, codec, proj, d_out, cap, d_out_off, d_docs, d_fail_field,
                           out_len, stats, stream);
}
