// kx_field_values_host.inc — field mode on unquoted values (kx_run_batch_field_values, include/kxhip.h; kernels in
// kx_field_values.inc).  Included at the end of kx_engine.hip between kx_field_list_host.inc, whose driver runFieldList runs the
// call, and kx_records_host.inc.  Here: the rules of a kx_field_codec, and the entry point.

namespace {

// the rules of a kx_field_codec beside its list `l` (`who`), found before any device work (checkFieldList has passed)
int checkFieldCodec(const kx_field_codec& c, const kx_batch_field_list& l, const char* who) {
  auto no = [&](const char* what) { return setErr(KX_E_ARG, std::string(who) + ": " + what); };
  if (c.size != sizeof(kx_field_codec)) return no("kx_field_codec::size is not this library's");
  if (c.n_special > 8) return no("at most 8 special bytes");
  for (uint32_t r : c.reserved) if (r) return no("reserved words must be 0");
  if (l.quote < 0 && l.escape < 0) return no("values need a quote or an escape byte");
  for (uint32_t i = 0; i < c.n_special; ++i)
    if ((int)c.special[i] == l.quote || (int)c.special[i] == l.escape) return no("a special byte cannot be the quote or the escape byte");
  return 0;
}

}  // namespace

extern "C" int kx_run_batch_field_values(kx_program* p, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_field_list* l,
                                         const kx_field_codec* codec, void* d_out, size_t cap, uint64_t* d_out_off, kx_batch_doc* d_docs,
                                         uint32_t* d_fail_field, size_t* out_len, kx_batch_stats* stats, void* stream) {
  static const char* const who = "kx_run_batch_field_values";
  if (!p || !out_len || !l || !codec) return setErr(KX_E_ARG, "null argument");
  if (const int rc = checkFieldList(*l, who)) return rc;
  if (const int rc = checkFieldCodec(*codec, *l, who)) return rc;
  return runFieldList(p, d_in, d_in_off, n_docs, l, codec, d_out, cap, d_out_off, d_docs, d_fail_field, out_len, stats, stream, who);
}
