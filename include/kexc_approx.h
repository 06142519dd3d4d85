/* kexc_approx.h — C ABI of libkexc.so for approximate matching (`t<k>` terms; --metric / --approxmode / --ite).
 *
 * Declared apart from kexc_api.h, whose set of entry points is pinned.  Same conventions: returns 0 and a malloc'd
 * blob (release with kexc_free), or 1 with the message in kexc_last_error(). */
#ifndef KEXC_APPROX_H
#define KEXC_APPROX_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* kexc_compile_flags for a Kleenex source, with the flags that say how its `t<k>` terms are rewritten (Options.hs:103-128):
 * metric 0 = LCS, 1 = Hamming, 2 = Levenshtein (`--metric`); mode 0 = correction, 1 = matching, 2 = explicit (`--approxmode`);
 * iterative non-zero = `--ite` (k rewrites of one error each instead of the k-fold one).  A source without `<k>` terms
 * compiles to the same blob whatever these are. */
int kexc_compile_approx(const char* source, size_t source_len, const char* source_name, int opt_level, int lookahead, int metric,
                        int mode, int iterative, unsigned char** blob, size_t* blob_len);

#ifdef __cplusplus
}
#endif
#endif
