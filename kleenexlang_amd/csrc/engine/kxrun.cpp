// kxrun.cpp — host driver of a compiled Kleenex binary (`kexc compile … --out BIN`).
//
// Keeps the command-line contract of the reference's generated binaries
// (crt/crt.c:326-467): `BIN < in > out`; `-i` prints compile info and exits 2;
// `-t` prints "time (ms): N" on stderr; `-h`/unknown prints usage on stdout and
// exits 1; a rejected input prints "Match error at input symbol <count>!" on
// stderr and exits 1.  `-p/--phase K` runs only phase K, stdin to stdout, as in
// the reference (crt.c:390-393,408-411); without it the phases of a pipeline run
// as chained device-resident stages inside one process (instead of
// fork()+pipe(), crt.c:414-454).  `--gpus N` (no counterpart in the reference) shards a regular
// file on stdin over N GPUs (kx_run_fd_sharded).  `--records[=SEP]` (no counterpart either) runs every SEP-terminated record
// (default a newline) as its own input (kx_run_records_fd): the accepted records' outputs go to stdout, one
// "Match error at input symbol S in record R!" line per rejected record to stderr, and the run goes on to the end.  With
// `--quote[=Q]` (default a double quote) a separator inside Q-quoted fields ends no record (kx_run_records_fd_quoted).  With
// `--escape[=E]` (default a backslash) a byte after an unescaped E is only data: never a separator, a quote or an escape
// (kx_run_records_fd_escaped, with or without --quote).  With `--rs=STR` the separator is the 1 to 8 bytes STR spells, and records
// end after its leftmost, non-overlapping copies (kx_run_records_fd_rs).  With `--chomp` every record is run without its separator
// (a last record without one is run whole), and with `--ors=STR` the 0 to 8 bytes STR spells follow the output of every accepted
// record (kx_run_records_fd_opts): the framing is the command line's, the program sees only the record.  With `--field=K` the
// program runs on field K of every record — the fields lie between the `--fs=F` bytes (default a tab) that the quote and the
// escape rules leave live — and the rest of the record is copied around its output (kx_run_records_fd_fields); a record with
// fewer fields writes nothing and is reported as "Record R has no field K!".  With `--field=LIST` (2,5-7,9-: anything but one
// plain number) the program runs on every field of the list, each a whole input of its own, and the record is written only if all
// of them are accepted (kx_run_records_fd_field_list; the list's parser is kx_field_list.h).  With `--unquote` (with --field, and
// --quote or --escape) the program runs on the VALUE of each selected field, and the field is replaced by the spelling of its
// output, quoted and escaped as it needs (kx_run_records_fd_field_values; --field=K is then the list K-K).  With `--blanks` (with
// --field, not with --fs) the fields are the words between runs of live spaces and tabs, as awk's default splitting has them, and
// every blank is copied as it is (kx_run_records_fd_field_words; --field=K is then the list K-K, with or without --unquote).  With
// `--only` (with --field) an accepted record writes the outputs of the selected fields alone, in the order the list was WRITTEN
// (up to 16 items, which may overlap and repeat) and joined by the 0 to 8 bytes of `--ofs=STR` (spelled as --ors; default the --fs
// byte, or one space with --blanks), then separator and --ors as ever (kx_run_records_fd_field_project; kxParseFieldOrder).  What
// --field, --fs, --unquote, --blanks, --only and --ofs refuse exits with status 2.  With `--header[=N]` (with --records; default 1)
// the first N records are header records — never run, copied, or with --only projected like the records behind them — and the
// items of --field may be NAMES of cells of header record N (kx_run_records_fd_table; the list's parser is kx_field_names.h): the
// option's text is then parsed behind the option loop.  A name no cell has ends the run with status 2.  With `--keys[=C]` (with
// --field, not with --header; default C: =) the fields are key=value pairs: every item of --field is a NAME (kx_field_keys.h; a
// last `?` makes it optional), a name selects the first field whose bytes before its first live C spell it, and the program runs
// on what follows that C (kx_run_records_fd_field_keys); a record that lacks a required name is reported as "Record R has no field
// NAME!".  The option's text is parsed behind the option loop as well.
//
// BIN = this executable ++ KXP blob ++ libdir ++ trailer (see kexc main.cpp).
// The engine is loaded with dlopen so that this file carries no HIP dependency.
#include <dlfcn.h>
#include <getopt.h>
#include <sys/time.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/kxhip.h"
#include "kx_field_list.h"
#include "kx_field_names.h"
#include "kx_field_keys.h"

// The engine's switches are fields of kx_config (include/kxhip.h); the library reads no environment variable for them.  A produced
// binary keeps honouring the variable names that earlier rounds' scripts use: they are read HERE, once, and mapped onto the struct.
static kx_config configFromEnv() {
  kx_config c{};
  auto num = [](const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; };
  auto tri = [&](const char* name) -> uint32_t { const char* e = getenv(name); return !e ? 0u : atoi(e) ? 2u : 1u; };   // unset: auto, 0: off, else: on
  if (const char* e = getenv("KX_DF")) { const int v = atoi(e); c.delayed_form = v == 0 ? 1u : v == 2 ? 2u : 0u; }
  c.delay = (uint32_t)num("KX_DF_K", 0);
  if (getenv("KX_DF_J")) c.merge_window = (uint32_t)num("KX_DF_J", 0) + 1;
  c.inline_consts = tri("KX_INL");
  c.job_stride = getenv("KX_JL") ? tri("KX_JL") : getenv("KX_JL_AUTO_OFF") ? 1u : 0u;
  if (getenv("KX_NO_DIRECT")) c.disable |= KX_OFF_DIRECT;
  if (getenv("KX_NO_PAIR")) c.disable |= KX_OFF_PAIR;
  if (getenv("KX_NO_CMPX")) c.disable |= KX_OFF_CMPX;
  if (getenv("KX_NO_COOP")) c.disable |= KX_OFF_COOP;
  if (getenv("KX_NO_SLOW")) c.disable |= KX_OFF_SLOW;
  if (getenv("KX_FORCE_BIG")) c.force |= KX_FORCE_BIG;
  if (getenv("KX_FORCE_TBLMODE")) c.force |= KX_FORCE_TBLMODE;
  if (getenv("KX_ACT_SEQ")) c.force |= KX_FORCE_ACT_SEQ;
  if (getenv("KX_SHARD_SAME_DEVICE")) c.force |= KX_FORCE_SAME_DEVICE;
  c.emit_waves = (uint32_t)num("KX_EMIT_WAVES", 0);
  c.emit_half = tri("KX_EMIT_HALF");
  c.emit_inplace = tri("KX_EMIT_INPLACE");
  c.emit_staging = (uint32_t)num("KX_EMIT_STG", 0);
  c.df_backoff = (uint32_t)num("KX_DF_BACKOFF_OFF", 0) ? 1u : 0u;
  c.debug_flags = (uint32_t)num("KX_DEBUG_FLAGS", 0);
  c.act_par_min = (uint32_t)num("KX_ACT_PAR_MIN", 0);
  c.act_prefix3_min = (uint32_t)num("KX_ACT_PREFIX3_MIN", 0);
  c.act_lanes = tri("KX_ACT_LANES");
  c.act_chunk = (uint32_t)num("KX_ACT_CHUNK", 0);
  c.batch_actions = tri("KX_BATCH_ACTIONS");   // (0: every document of an action stage takes the route; else the batch replay)
  return c;
}

static void usage(const char* name) {
  fprintf(stdout, "Normal usage: %s < infile > outfile\n", name);
  fprintf(stdout, "- \"%s\": reads from stdin and writes to stdout.\n", name);
  fprintf(stdout, "- \"%s -i\": prints compilation info.\n", name);
  fprintf(stdout, "- \"%s -t\": runs normally, but prints timing to stderr.\n", name);
  fprintf(stdout, "- \"%s --records[=SEP]\": runs every line (or SEP-terminated record) as its own input; rejected ones are reported on stderr.\n", name);
  fprintf(stdout, "- \"%s --records[=SEP] --quote[=Q]\": the same, but a SEP inside Q-quoted fields (default Q: \") ends no record.\n", name);
  fprintf(stdout, "- \"%s --records[=SEP] [--quote[=Q]] --escape[=E]\": the same, but a byte after an unescaped E (default E: \\) is only data.\n", name);
  fprintf(stdout, "- \"%s --records --rs=STR\": records end after the 1 to 8 bytes STR spells (\\r\\n, \\n\\n, \\xHH ...), leftmost and non-overlapping.\n", name);
  fprintf(stdout, "- \"%s --records ... --chomp\": every record is run without its separator (a last record without one is run whole).\n", name);
  fprintf(stdout, "- \"%s --records ... --ors=STR\": the 0 to 8 bytes STR spells follow the output of every accepted record.\n", name);
  fprintf(stdout, "- \"%s --records ... --field=K [--fs=F]\": runs field K (from 1; fields end at F, default a tab) of every record, the rest is copied.\n", name);
  fprintf(stdout, "- \"%s --records ... --field=LIST [--fs=F]\": the same on every field of LIST (2,5-7,9-); a record is written only if all of them are accepted.\n", name);
  fprintf(stdout, "- \"%s --records ... --quote|--escape --field=K|LIST [--fs=F] --unquote\": the program runs on the unquoted value of every selected field; its output is quoted again as it needs.\n", name);
  fprintf(stdout, "- \"%s --records ... --field=K|LIST --blanks [--unquote]\": the fields are the words between runs of spaces and tabs (awk's default); every blank is copied as it is.\n", name);
  fprintf(stdout, "- \"%s --records ... --field=K|LIST [--fs=F | --blanks] [--unquote] --only [--ofs=STR]\": writes only the selected fields' outputs, in the order LIST is written (4,2 or 2,1,2), joined by STR (0 to 8 bytes; default F, or a space with --blanks).\n", name);
  fprintf(stdout, "- \"%s --records ... --header[=N] [--field=LIST ...]\": the first N records (default 1) are header rows: never run, copied (with --only: projected), and LIST may name columns of row N (id,city or 2,name,5-; \\, is a comma in a name). With --keys[=C] in place of --header the fields are key=value pairs (C, default =, ends the key) and LIST names keys (ts,msg? - a last ? makes one optional): the program runs on the value of the first field with each key.\n", name);
}

// --records=SEP, --quote=Q, --escape=E: one literal byte, or \n \t \r \0 \\ \xHH.  false if it is none of these.
static bool parseSeparator(const char* a, uint8_t* sep) {
  auto hex = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
  const size_t n = strlen(a);
  if (n == 1) { *sep = (uint8_t)a[0]; return true; }
  if (n == 2 && a[0] == '\\') {
    switch (a[1]) {
      case 'n': *sep = '\n'; return true;
      case 't': *sep = '\t'; return true;
      case 'r': *sep = '\r'; return true;
      case '0': *sep = 0; return true;
      case '\\': *sep = '\\'; return true;
      default: return false;
    }
  }
  if (n == 4 && a[0] == '\\' && a[1] == 'x' && hex(a[2]) >= 0 && hex(a[3]) >= 0) { *sep = (uint8_t)(hex(a[2]) * 16 + hex(a[3])); return true; }
  return false;
}

// --rs=STR: 1 to 8 byte spellings, each a literal byte or \n \t \r \0 \\ \xHH; a backslash always starts an escape.  false if
// STR is not that; else *len bytes in rs.
static bool parseSeparatorString(const char* a, uint8_t* rs, uint32_t* len) {
  auto hex = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
  uint32_t n = 0;
  for (const char* p = a; *p;) {
    if (n == 8) return false;
    if (*p != '\\') { rs[n++] = (uint8_t)*p++; continue; }
    switch (p[1]) {
      case 'n': rs[n++] = '\n'; p += 2; break;
      case 't': rs[n++] = '\t'; p += 2; break;
      case 'r': rs[n++] = '\r'; p += 2; break;
      case '0': rs[n++] = 0; p += 2; break;
      case '\\': rs[n++] = '\\'; p += 2; break;
      case 'x':
        if (hex(p[2]) < 0 || hex(p[3]) < 0) return false;   // (a NUL ends the test early: hex('\0') < 0)
        rs[n++] = (uint8_t)(hex(p[2]) * 16 + hex(p[3]));
        p += 4;
        break;
      default: return false;
    }
  }
  *len = n;
  return n >= 1;
}

// --ors=STR: as --rs, but 0 to 8 byte spellings (an empty STR: no output separator)
static bool parseOutputSeparator(const char* a, uint8_t* ors, uint32_t* len) {
  if (!*a) { *len = 0; return true; }
  return parseSeparatorString(a, ors, len);
}

// the engine's `name`; without it, null after the message that this library has none and which option (`needs`) wants a newer one
static void* engineSymbol(void* h, const char* argv0, const char* name, const char* needs) {
  void* f = dlsym(h, name);
  if (!f) fprintf(stderr, "%s: this libkxhip.so has no %s (%s a newer engine library)\n", argv0, name, needs);
  return f;
}

int main(int argc, char** argv) {
  // locate the payload appended to this executable
  FILE* self = fopen("/proc/self/exe", "rb");
  if (!self) { perror("/proc/self/exe"); return 1; }
  fseek(self, 0, SEEK_END);
  long size = ftell(self);
  char trailer[24];
  if (size < 24 || fseek(self, size - 24, SEEK_SET) || fread(trailer, 1, 24, self) != 24 || memcmp(trailer + 16, "KXRUNTRL", 8)) {
    fprintf(stderr, "%s: no compiled program attached (use `kexc compile prog.kex --out BIN`)\n", argv[0]);
    return 1;
  }
  uint64_t bl, dl;
  memcpy(&bl, trailer, 8); memcpy(&dl, trailer + 8, 8);
  if (bl < 20 || bl > (uint64_t)size || dl > (uint64_t)size || bl + dl + 24 > (uint64_t)size) { fprintf(stderr, "%s: corrupt payload trailer\n", argv[0]); return 1; }
  std::vector<unsigned char> blob(bl);
  std::string libdir(dl, '\0');
  fseek(self, size - 24 - (long)dl - (long)bl, SEEK_SET);
  if (fread(blob.data(), 1, bl, self) != bl || fread(&libdir[0], 1, dl, self) != dl) { fprintf(stderr, "corrupt payload\n"); return 1; }
  fclose(self);

  static struct option long_options[] = {{"phase", required_argument, 0, 'p'}, {"gpus", required_argument, 0, 'g'},
                                         {"records", optional_argument, 0, 'r'}, {"quote", optional_argument, 0, 'q'},
                                         {"escape", optional_argument, 0, 'e'}, {"rs", required_argument, 0, 's'},
                                         {"chomp", no_argument, 0, 'c'}, {"ors", required_argument, 0, 'o'},
                                         {"field", required_argument, 0, 'f'}, {"fs", required_argument, 0, 'F'},
                                         {"unquote", no_argument, 0, 'u'}, {"blanks", no_argument, 0, 'b'},
                                         {"only", no_argument, 0, 'y'}, {"ofs", required_argument, 0, 'O'},
                                         {"header", optional_argument, 0, 'H'}, {"keys", optional_argument, 0, 'K'},
                                         {0, 0, 0, 0}};
  bool timing = false, records = false, quoted = false, escaped = false, sep_given = false, multi = false, chomp = false, ors_given = false;
  uint8_t sep = '\n', quote = '"', escape = '\\', rs[8] = {}, ors[8] = {};
  uint32_t rs_len = 0, ors_len = 0, field = 0;
  bool field_given = false, fs_given = false, unquote = false, blanks = false;
  kx_field_range ranges[KX_FIELD_RANGES] = {};   // --field=LIST in normal form (n_ranges = 0: --field=K, one plain number)
  uint32_t n_ranges = 0;
  uint8_t fsep = '\t';
  bool only = false, ofs_given = false;
  const char* field_text = nullptr;              // --field's text: with --only it is parsed once more, as written
  kx_field_range items[KX_FIELD_ITEMS] = {};     // --only: the list as written
  uint32_t n_items = 0, ofs_len = 0;
  uint8_t ofs[8] = {};
  long phase = 0, gpus = 0;
  bool header_given = false, has_names = false;
  uint32_t header = 1;
  std::vector<KxFieldNameItem> named;            // --header with a name in --field: the list as written
  bool keys_given = false;
  uint8_t kvsep = '=';
  KxFieldKeys keyed;                             // --keys: --field's names
  for (int i = 1; i < argc && strcmp(argv[i], "--") != 0; ++i) {   // (with --header or --keys the text of --field is parsed behind the loop)
    if (!strcmp(argv[i], "--header") || !strncmp(argv[i], "--header=", 9)) header_given = true;
    if (!strcmp(argv[i], "--keys") || !strncmp(argv[i], "--keys=", 7)) keys_given = true;
  }
  // --field's text without names: null, or the exit status after the message
  auto parseFieldNumbers = [&](const char* text) -> int {
    n_ranges = 0; field = 0;
    if (strpbrk(text, ",-")) {   // a list; one plain number (and what is neither) takes the single-field path below
      if (const char* why = kxParseFieldList(text, ranges, &n_ranges)) {
        fprintf(stderr, "Invalid --field: %s (a number from 1 to 4294967295, or a list such as 2,5-7,9-: %s)\n", text, why);
        return 2;
      }
      return 0;
    }
    char* end = nullptr;
    const unsigned long long v = (*text >= '0' && *text <= '9') ? strtoull(text, &end, 10) : 0;
    if (!end || *end || v < 1 || v > 0xFFFFFFFFull || strlen(text) > 10) { fprintf(stderr, "Invalid --field: %s (a number from 1 to 4294967295)\n", text); return 2; }
    field = (uint32_t)v;
    return 0;
  };
  int c;
  while ((c = getopt_long(argc, argv, "ihtp:", long_options, nullptr)) != -1) {
    switch (c) {
      case 'i': {
        uint32_t il; memcpy(&il, blob.data() + 16, 4);
        if ((uint64_t)il + 20 > blob.size()) { fprintf(stderr, "%s: corrupt payload\n", argv[0]); return 1; }
        std::string info((const char*)blob.data() + 20, il);
        for (size_t p; (p = info.find("\\n")) != std::string::npos;) info.replace(p, 2, "\n");
        fprintf(stdout, "%s\n", info.c_str());
        return 2;
      }
      case 't': timing = true; break;
      case 'g': gpus = atol(optarg); if (gpus < 1 || gpus > 64) { fprintf(stderr, "Invalid number of GPUs: %ld given\n", gpus); return 1; } break;
      case 'p': phase = atol(optarg); if (phase < 1) { fprintf(stderr, "Invalid phase: %ld given\n", phase); return 1; } break;
      case 'r':
        records = true;
        if (optarg) sep_given = true;
        if (optarg && !parseSeparator(optarg, &sep)) { fprintf(stderr, "Invalid record separator: %s\n", optarg); return 1; }
        break;
      case 'q':
        quoted = true;
        if (optarg && !parseSeparator(optarg, &quote)) { fprintf(stderr, "Invalid quote character: %s\n", optarg); return 1; }
        break;
      case 'e':
        escaped = true;
        if (optarg && !parseSeparator(optarg, &escape)) { fprintf(stderr, "Invalid escape character: %s\n", optarg); return 1; }
        break;
      case 's':
        multi = true;
        if (!parseSeparatorString(optarg, rs, &rs_len)) { fprintf(stderr, "Invalid record separator: %s\n", optarg); return 1; }
        break;
      case 'c': chomp = true; break;
      case 'o':
        ors_given = true;
        if (!parseOutputSeparator(optarg, ors, &ors_len)) { fprintf(stderr, "Invalid output record separator: %s\n", optarg); return 1; }
        break;
      case 'f':
        field_given = true;
        field_text = optarg;
        if (!header_given && !keys_given) if (const int bad = parseFieldNumbers(optarg)) return bad;
        break;
      case 'K':
        keys_given = true;
        if (optarg && !parseSeparator(optarg, &kvsep)) { fprintf(stderr, "Invalid --keys: %s (one byte)\n", optarg); return 2; }
        break;
      case 'H': {
        header_given = true;
        if (!optarg) break;
        char* end = nullptr;
        const unsigned long long v = (*optarg >= '0' && *optarg <= '9') ? strtoull(optarg, &end, 10) : 0;
        if (!end || *end || v < 1 || v > 0xFFFFFFFFull || strlen(optarg) > 10) { fprintf(stderr, "Invalid --header: %s (a number from 1 to 4294967295)\n", optarg); return 2; }
        header = (uint32_t)v;
        break;
      }
      case 'F':
        fs_given = true;
        if (!parseSeparator(optarg, &fsep)) { fprintf(stderr, "Invalid --fs: %s (one byte)\n", optarg); return 2; }
        break;
      case 'u': unquote = true; break;
      case 'b': blanks = true; break;
      case 'y': only = true; break;
      case 'O':
        ofs_given = true;
        if (!parseOutputSeparator(optarg, ofs, &ofs_len)) { fprintf(stderr, "Invalid output field separator: %s\n", optarg); return 2; }
        break;
      case 'h':
      default: usage(argv[0]); return 1;
    }
  }
  // (refused before the engine library is loaded)
  if (header_given && !records) { fprintf(stderr, "%s: --header needs --records\n", argv[0]); return 2; }
  if (keys_given && !field_given) { fprintf(stderr, "%s: --keys needs --field\n", argv[0]); return 2; }
  if (keys_given && header_given) { fprintf(stderr, "%s: --keys cannot be combined with --header\n", argv[0]); return 2; }
  if (keys_given) {                    // --field's text: every item is a name
    if (const char* why = kxParseFieldKeys(field_text, &keyed)) {
      fprintf(stderr, "Invalid --field: %s (with --keys a list of at most 16 names such as ts,msg?: %s)\n", field_text, why);
      return 2;
    }
  }
  if (header_given && field_given) {   // --field's text, which may hold names of header cells
    has_names = kxFieldTextHasName(field_text);
    if (!has_names) { if (const int bad = parseFieldNumbers(field_text)) return bad; }
    else if (const char* why = kxParseFieldNames(field_text, &named)) {
      fprintf(stderr, "Invalid --field: %s (with --header a list of at most 16 numbers, ranges and column names such as 2,name,5-: %s)\n", field_text, why);
      return 2;
    }
  }
  if (records && phase) { fprintf(stderr, "%s: --records cannot be combined with --phase\n", argv[0]); return 1; }
  if (records && gpus) { fprintf(stderr, "%s: --records cannot be combined with --gpus\n", argv[0]); return 1; }
  if (quoted && !records) { fprintf(stderr, "%s: --quote needs --records\n", argv[0]); return 1; }
  if (quoted && quote == sep) { fprintf(stderr, "%s: the quote character cannot be the record separator\n", argv[0]); return 1; }
  if (escaped && !records) { fprintf(stderr, "%s: --escape needs --records\n", argv[0]); return 1; }
  if (escaped && escape == sep) { fprintf(stderr, "%s: the escape character cannot be the record separator\n", argv[0]); return 1; }
  if (escaped && quoted && escape == quote) { fprintf(stderr, "%s: the escape character cannot be the quote character\n", argv[0]); return 1; }
  if (multi && !records) { fprintf(stderr, "%s: --rs needs --records\n", argv[0]); return 1; }
  if (multi && sep_given) { fprintf(stderr, "%s: --rs cannot be combined with --records=SEP\n", argv[0]); return 1; }
  if (multi && (quoted || escaped)) { fprintf(stderr, "%s: --rs cannot be combined with --quote or --escape\n", argv[0]); return 1; }
  if (chomp && !records) { fprintf(stderr, "%s: --chomp needs --records\n", argv[0]); return 1; }
  if (ors_given && !records) { fprintf(stderr, "%s: --ors needs --records\n", argv[0]); return 1; }
  if (field_given && !records) { fprintf(stderr, "%s: --field needs --records\n", argv[0]); return 2; }
  auto isBlank = [](uint8_t b) { return b == ' ' || b == '\t'; };
  if (blanks && !field_given) { fprintf(stderr, "%s: --blanks needs --field\n", argv[0]); return 2; }
  if (blanks && fs_given) { fprintf(stderr, "%s: --blanks cannot be combined with --fs\n", argv[0]); return 2; }
  if (blanks && (multi ? rs_len == 1 && isBlank(rs[0]) : isBlank(sep))) { fprintf(stderr, "%s: with --blanks the record separator cannot be a space or a tab\n", argv[0]); return 2; }
  if (blanks && quoted && isBlank(quote)) { fprintf(stderr, "%s: with --blanks the --quote character cannot be a space or a tab\n", argv[0]); return 2; }
  if (blanks && escaped && isBlank(escape)) { fprintf(stderr, "%s: with --blanks the --escape character cannot be a space or a tab\n", argv[0]); return 2; }
  if (fs_given && !field_given) { fprintf(stderr, "%s: --fs needs --field\n", argv[0]); return 2; }
  if (field_given && (multi ? rs_len == 1 && fsep == rs[0] : fsep == sep)) { fprintf(stderr, "%s: --fs cannot be the record separator\n", argv[0]); return 2; }
  if (field_given && quoted && fsep == quote) { fprintf(stderr, "%s: --fs cannot be the --quote character\n", argv[0]); return 2; }
  if (field_given && escaped && fsep == escape) { fprintf(stderr, "%s: --fs cannot be the --escape character\n", argv[0]); return 2; }
  if (unquote && !field_given) { fprintf(stderr, "%s: --unquote needs --field\n", argv[0]); return 2; }
  if (unquote && !quoted && !escaped) { fprintf(stderr, "%s: --unquote needs --quote or --escape\n", argv[0]); return 2; }
  if (only && !field_given) { fprintf(stderr, "%s: --only needs --field\n", argv[0]); return 2; }
  if (ofs_given && !only) { fprintf(stderr, "%s: --ofs needs --only\n", argv[0]); return 2; }
  if (keys_given) {   // the key separator and the names beside the bytes of the framing
    const int rsep = multi ? (rs_len == 1 ? (int)rs[0] : -1) : (int)sep;
    if (const char* clash = kxFieldKeyByteClash(kvsep, blanks ? -1 : (int)fsep, blanks, rsep, quoted ? (int)quote : -1, escaped ? (int)escape : -1)) {
      fprintf(stderr, "%s: the --keys character cannot be %s\n", argv[0], clash);
      return 2;
    }
    for (const std::string& nm : keyed.names)
      if (const char* clash = kxFieldKeyNameClash((const uint8_t*)nm.data(), nm.size(), kvsep, blanks ? -1 : (int)fsep, blanks, rsep)) {
        fprintf(stderr, "%s: with --keys the name \"%s\" of --field cannot hold %s\n", argv[0], kxPrintableName(nm).c_str(), clash);
        return 2;
      }
  }
  if (only) {   // the list as written (a plain number is the list K-K); its union is what the list's own parse gave
    if (!has_names && !keys_given)
      if (const char* why = kxParseFieldOrder(field_text, items, &n_items, ranges, &n_ranges)) {
        fprintf(stderr, "Invalid --field: %s (with --only a list of at most 16 items such as 4,2 or 2,1,2: %s)\n", field_text, why);
        return 2;
      }
    if (!ofs_given) { ofs[0] = blanks ? (uint8_t)' ' : fsep; ofs_len = 1; }
    if (unquote && ofs_len != 1) { fprintf(stderr, "%s: with --unquote --ofs is exactly one byte\n", argv[0]); return 2; }
    if (unquote && quoted && ofs[0] == quote) { fprintf(stderr, "%s: with --unquote --ofs cannot be the --quote character\n", argv[0]); return 2; }
    if (unquote && escaped && ofs[0] == escape) { fprintf(stderr, "%s: with --unquote --ofs cannot be the --escape character\n", argv[0]); return 2; }
    if (unquote && (multi ? rs_len == 1 && ofs[0] == rs[0] : ofs[0] == sep)) { fprintf(stderr, "%s: with --unquote --ofs cannot be the record separator\n", argv[0]); return 2; }
    if (unquote && blanks && ofs[0] == '\t') { fprintf(stderr, "%s: with --unquote and --blanks --ofs cannot be the tab\n", argv[0]); return 2; }
  }
  if ((unquote || blanks) && !n_ranges && !has_names && !keys_given) { ranges[0] = kx_field_range{field, field}; n_ranges = 1; }   // --field=K on values or words: the list K-K
  struct timeval t0, t1;
  if (timing) gettimeofday(&t0, nullptr);

  const char* env = getenv("KXHIP_LIB");
  std::string lib = env ? env : libdir + "/libkxhip.so";
  void* h = dlopen(lib.c_str(), RTLD_NOW);
  if (!h) { fprintf(stderr, "%s: cannot load the HIP engine: %s\n", argv[0], dlerror()); return 1; }
  auto load = (int (*)(const void*, size_t, const kx_config*, kx_program**))dlsym(h, "kx_load_config");
  auto run = (int (*)(kx_program*, int, int, kx_stats*))dlsym(h, "kx_run_fd");
  auto lasterr = (const char* (*)(void))dlsym(h, "kx_last_error");
  if (!load || !run || !lasterr) { fprintf(stderr, "%s: engine library lacks required symbols\n", argv[0]); return 1; }
  kx_stats st;
  int rc;
  kx_config cfg = configFromEnv();
  if (records) {
    const bool framing = chomp || ors_len;   // (--ors= alone is the default: no output separator)
    auto runr = (decltype(&kx_run_records_fd))engineSymbol(h, argv[0], "kx_run_records_fd", "--records needs");
    decltype(&kx_run_records_fd_quoted) runq = nullptr;
    decltype(&kx_run_records_fd_escaped) rune = nullptr;
    decltype(&kx_run_records_fd_rs) runm = nullptr;
    decltype(&kx_run_records_fd_opts) runo = nullptr;
    decltype(&kx_run_records_fd_fields) runf = nullptr;
    decltype(&kx_run_records_fd_field_list) runl = nullptr;
    decltype(&kx_run_records_fd_field_words) runw = nullptr;
    decltype(&kx_run_records_fd_field_project) runp = nullptr;
    decltype(&kx_run_records_fd_table) runt = nullptr;
    decltype(&kx_run_records_fd_field_keys) runk = nullptr;
    if (!runr) return 1;
    if (keys_given && !(runk = (decltype(runk))engineSymbol(h, argv[0], "kx_run_records_fd_field_keys", "--keys needs"))) return 1;
    if (header_given && !(runt = (decltype(runt))engineSymbol(h, argv[0], "kx_run_records_fd_table", "--header needs"))) return 1;
    if (!runt && !runk && quoted && !(runq = (decltype(runq))engineSymbol(h, argv[0], "kx_run_records_fd_quoted", "--quote needs"))) return 1;
    if (!runt && !runk && escaped && !(rune = (decltype(rune))engineSymbol(h, argv[0], "kx_run_records_fd_escaped", "--escape needs"))) return 1;
    if (!runt && !runk && multi && !(runm = (decltype(runm))engineSymbol(h, argv[0], "kx_run_records_fd_rs", "--rs needs"))) return 1;
    if (!runt && !runk && only && !(runp = (decltype(runp))engineSymbol(h, argv[0], "kx_run_records_fd_field_project", "--only needs"))) return 1;
    if (!runt && !runk && field_given && !n_ranges && !(runf = (decltype(runf))engineSymbol(h, argv[0], "kx_run_records_fd_fields", "--field needs"))) return 1;
    if (!runt && !runk && blanks && !only && !(runw = (decltype(runw))engineSymbol(h, argv[0], "kx_run_records_fd_field_words", "--blanks needs"))) return 1;
    if (!runt && !runk && n_ranges && !unquote && !blanks && !only && !(runl = (decltype(runl))engineSymbol(h, argv[0], "kx_run_records_fd_field_list", "--field=LIST needs"))) return 1;
    if (!runt && !runk && unquote && !blanks && !only && !(runl = (decltype(runl))engineSymbol(h, argv[0], "kx_run_records_fd_field_values", "--unquote needs"))) return 1;   // (the same signature)
    if (!runt && !runk && framing && !(runo = (decltype(runo))engineSymbol(h, argv[0], "kx_run_records_fd_opts", "--chomp and --ors need"))) return 1;
    // record mode is where the single-document route is unusable (a third of a millisecond per record): stages with register
    // actions are replayed by the batch kernels unless KX_BATCH_ACTIONS=0 asks for the route
    if (!cfg.batch_actions) cfg.batch_actions = 2;
    kx_program* prog = nullptr;
    if (load(blob.data(), blob.size(), &cfg, &prog)) { fprintf(stderr, "%s: %s\n", argv[0], lasterr()); return 1; }
    kx_records_stats rs_stats;
    if (header_given) {   // every combination goes through the one entry point that knows header records
      kx_records_opts o{};
      o.size = sizeof o;
      o.mode = multi ? KX_RECORDS_RS : escaped ? KX_RECORDS_ESCAPED : quoted ? KX_RECORDS_QUOTED : KX_RECORDS_BYTE;
      o.sep = sep;
      o.quote = quoted ? (int)quote : -1;
      o.escape = escaped ? (int)escape : -1;
      memcpy(o.rs, rs, 8); o.rs_len = rs_len;
      o.chomp = chomp ? 1u : 0u;
      memcpy(o.ors, ors, 8); o.ors_len = ors_len;
      kx_records_table t{};
      t.size = sizeof t; t.header = header; t.fs = fsep;
      t.flags = (blanks ? KX_TABLE_WORDS : 0u) | (unquote ? KX_TABLE_UNQUOTE : 0u) | (only ? KX_TABLE_ONLY : 0u);
      if (has_names) {   // the list as written, its names by index
        for (const KxFieldNameItem& it : named) {
          if (it.is_name) {
            t.items[t.n_items++] = kx_field_range{0u, t.n_names};
            t.names[t.n_names] = (const uint8_t*)it.name.data(); t.name_len[t.n_names++] = (uint32_t)it.name.size();
          } else {
            t.items[t.n_items++] = kx_field_range{(uint32_t)it.lo, it.hi == 1ull << 32 ? 0u : (uint32_t)it.hi};
          }
        }
      } else if (only) {
        t.n_items = n_items; memcpy(t.items, items, sizeof items);
      } else if (n_ranges) {   // (a set: its normal form is a list as good as the written one)
        t.n_items = n_ranges; memcpy(t.items, ranges, sizeof ranges);
      } else if (field_given) {
        t.n_items = 1; t.items[0] = kx_field_range{field, field}; t.flags |= KX_TABLE_SINGLE;
      }
      if (only) { t.ofs_len = ofs_len; memcpy(t.ofs, ofs, 8); }
      rc = runt(prog, STDIN_FILENO, STDOUT_FILENO, &o, &t, STDERR_FILENO, &rs_stats);
      if (rc == KX_E_HEADER) { fprintf(stderr, "%s: %s\n", argv[0], lasterr()); return 2; }
    } else if (framing || field_given) {
      kx_records_opts o{};
      o.size = sizeof o;
      o.mode = multi ? KX_RECORDS_RS : escaped ? KX_RECORDS_ESCAPED : quoted ? KX_RECORDS_QUOTED : KX_RECORDS_BYTE;
      o.sep = sep;
      o.quote = quoted ? (int)quote : -1;
      o.escape = escaped ? (int)escape : -1;
      memcpy(o.rs, rs, 8); o.rs_len = rs_len;
      o.chomp = chomp ? 1u : 0u;
      memcpy(o.ors, ors, 8); o.ors_len = ors_len;
      kx_field_keys kk{};
      uint32_t kitems[KX_FIELD_ITEMS] = {};
      if (keys_given) {
        kk.size = sizeof kk; kk.n_names = (uint32_t)keyed.names.size(); kk.optional_mask = keyed.optional_mask; kk.kv = kvsep;
        kk.flags = (blanks ? KX_KEYS_WORDS : 0u) | (unquote ? KX_KEYS_UNQUOTE : 0u) | (only ? KX_KEYS_ONLY : 0u);
        for (uint32_t j = 0; j < kk.n_names; ++j) { kk.names[j] = (const uint8_t*)keyed.names[j].data(); kk.name_len[j] = (uint32_t)keyed.names[j].size(); }
        for (size_t j = 0; j < keyed.items.size(); ++j) kitems[j] = keyed.items[j];
      }
      rc = keys_given  ? runk(prog, STDIN_FILENO, STDOUT_FILENO, &o, &kk, fsep, kitems, (uint32_t)keyed.items.size(), ofs, ofs_len, STDERR_FILENO, &rs_stats)
           : only      ? runp(prog, STDIN_FILENO, STDOUT_FILENO, &o, items, n_items, fsep, ofs, ofs_len,
                                (blanks ? KX_PROJECT_WORDS : 0u) | (unquote ? KX_PROJECT_UNQUOTE : 0u), STDERR_FILENO, &rs_stats)
           : blanks    ? runw(prog, STDIN_FILENO, STDOUT_FILENO, &o, ranges, n_ranges, unquote ? 1 : 0, STDERR_FILENO, &rs_stats)
           : n_ranges  ? runl(prog, STDIN_FILENO, STDOUT_FILENO, &o, ranges, n_ranges, fsep, STDERR_FILENO, &rs_stats)
           : field_given ? runf(prog, STDIN_FILENO, STDOUT_FILENO, &o, field, fsep, STDERR_FILENO, &rs_stats)
                       : runo(prog, STDIN_FILENO, STDOUT_FILENO, &o, STDERR_FILENO, &rs_stats);
    } else if (multi) rc = runm(prog, STDIN_FILENO, STDOUT_FILENO, rs, rs_len, STDERR_FILENO, &rs_stats);
    else if (escaped) rc = rune(prog, STDIN_FILENO, STDOUT_FILENO, sep, quoted ? (int)quote : -1, escape, STDERR_FILENO, &rs_stats);
    else rc = quoted ? runq(prog, STDIN_FILENO, STDOUT_FILENO, sep, quote, STDERR_FILENO, &rs_stats) : runr(prog, STDIN_FILENO, STDOUT_FILENO, sep, STDERR_FILENO, &rs_stats);
    if (rc != 0 && rc != KX_MATCH_ERROR) { fprintf(stderr, "%s: %s\n", argv[0], lasterr()); return 1; }
    if (timing) {   // (a rejected record does not end the run: the time is printed either way)
      gettimeofday(&t1, nullptr);
      fprintf(stderr, "time (ms): %ld\n", (long)((t1.tv_sec - t0.tv_sec) * 1000 + (t1.tv_usec - t0.tv_usec) / 1000));
    }
    return rc == KX_MATCH_ERROR ? 1 : 0;
  }
  if (gpus) {
    auto runs = (int (*)(const void*, size_t, const kx_config*, int, int, int, kx_stats*))dlsym(h, "kx_run_fd_sharded_cfg");
    if (phase) { fprintf(stderr, "%s: --gpus cannot be combined with --phase\n", argv[0]); return 1; }
    if (!runs) { fprintf(stderr, "%s: this libkxhip.so has no kx_run_fd_sharded_cfg (--gpus needs the engine library of round 6 or later)\n", argv[0]); return 1; }
    rc = runs(blob.data(), blob.size(), &cfg, (int)gpus, STDIN_FILENO, STDOUT_FILENO, &st);
  } else {
  kx_program* prog = nullptr;
  if (load(blob.data(), blob.size(), &cfg, &prog)) { fprintf(stderr, "%s: %s\n", argv[0], lasterr()); return 1; }
  if (phase) {
    auto setcfg = (int (*)(kx_program*, const kx_config*))dlsym(h, "kx_set_config");
    auto nst = (uint32_t (*)(const kx_program*))dlsym(h, "kx_num_stages");
    if (!setcfg || !nst) { fprintf(stderr, "%s: engine library lacks required symbols\n", argv[0]); return 1; }
    if ((unsigned long)phase > nst(prog)) { fprintf(stderr, "Invalid phase: %ld given\n", phase); return 1; }   // (crt.c match(): default case)
    cfg.phase = (uint32_t)phase;
    if (setcfg(prog, &cfg)) { fprintf(stderr, "%s: %s\n", argv[0], lasterr()); return 1; }
  }
  rc = run(prog, STDIN_FILENO, STDOUT_FILENO, &st);
  }
  if (rc == KX_MATCH_ERROR) {
    // `kexc simulate` runs its program through this driver and wants the reference simulators' words instead of the
    // compiled binary's (Commands.hs:285,298 "Reject"; SymbolicSST.hs:425,427)
    const char* sim = getenv("KX_SIM_MESSAGES");
    if (sim && strcmp(sim, "sst") != 0) fprintf(stderr, "Reject\n");
    else if (sim) fprintf(stderr, "%s\n", st.fail_stage == 0 && st.fail_pos >= st.in_bytes ? "End of input reached, but final state is not accepting." : "No match");
    else fprintf(stderr, "Match error at input symbol %zu!\n", (size_t)st.fail_pos);
    return 1;
  }
  if (rc) { fprintf(stderr, "%s: %s\n", argv[0], lasterr()); return 1; }
  if (timing) {
    gettimeofday(&t1, nullptr);
    long ms = (t1.tv_sec - t0.tv_sec) * 1000 + (t1.tv_usec - t0.tv_usec) / 1000;
    fprintf(stderr, "time (ms): %ld\n", ms);
  }
  return 0;
}
