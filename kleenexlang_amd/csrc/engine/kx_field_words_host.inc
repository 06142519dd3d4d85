// kx_field_words_host.inc — field mode on words (kx_run_batch_field_words, include/kxhip.h; kernels in kx_field_words.inc).
// Included at the end of kx_engine.hip between kx_field_values_host.inc, whose codec rules it applies, and kx_records_host.inc.
// The driver is kx_field_list_host.inc's runFieldList with `words` set.  Here: the blank rules (also kx_run_batch_field_project's), and the entry point.

namespace {

inline bool kxIsBlank(int b) { return b == 0x20 || b == 0x09; }

// the rules of a words call (`who`), found before any device work; *ll and *cc are then the list and the codec the driver takes:
// the list with fs = 0, the codec (if there is one) with the tab appended to its special bytes
int checkFieldWords(const kx_batch_field_list* l, const kx_field_codec* codec, const char* who, kx_batch_field_list* ll, kx_field_codec* cc) {
  auto no = [&](const char* what) { return setErr(KX_E_ARG, std::string(who) + ": " + what); };
  if (l->size != sizeof(kx_batch_field_list)) return no("kx_batch_field_list::size is not this library's");
  if (l->fs != 0) return no("kx_batch_field_list::fs must be 0: the fields are the words between blanks");
  if (kxIsBlank(l->quote)) return no("the quote byte cannot be a blank");
  if (kxIsBlank(l->escape)) return no("the escape byte cannot be a blank");
  *ll = *l;
  ll->fs = 0x20;   // (for the list's own rules only: the kernels of this path do not read it)
  if (const int rc = checkFieldList(*ll, who)) return rc;
  ll->fs = 0;
  *cc = kx_field_codec{};
  if (codec) {
    if (codec->size != sizeof(kx_field_codec)) return no("kx_field_codec::size is not this library's");
    if (codec->n_special > 7) return no("at most 7 special bytes (the library adds the tab)");
    for (uint32_t i = 0; i < codec->n_special; ++i) if (kxIsBlank(codec->special[i])) return no("a special byte cannot be a blank");
    *cc = *codec;
    cc->special[cc->n_special++] = 0x09;
    if (const int rc = checkFieldCodec(*cc, *ll, who)) return rc;
  }
  return 0;
}

}  // namespace

extern "C" int kx_run_batch_field_words(kx_program* p, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_field_list* l,
                                        const kx_field_codec* codec, void* d_out, size_t cap, uint64_t* d_out_off, kx_batch_doc* d_docs,
                                        uint32_t* d_fail_field, size_t* out_len, kx_batch_stats* stats, void* stream) {
  static const char* const who = "kx_run_batch_field_words";
  if (!p || !out_len || !l) return setErr(KX_E_ARG, "null argument");
  kx_batch_field_list ll;
  kx_field_codec cc;
  if (const int rc = checkFieldWords(l, codec, who, &ll, &cc)) return rc;
  return runFieldList(p, d_in, d_in_off, n_docs, &ll, codec ? &cc : nullptr, d_out, cap, d_out_off, d_docs, d_fail_field, out_len, stats, stream, who,
                      true);
}
