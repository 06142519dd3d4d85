"""Record mode as ONE model, and the generators of the record-stream tests (test_records_stream.py, test_records_stream_gpu.py).

  Options            the keywords of one run, as Program.run_records_fd takes them (kwargs) and as the binary takes them (args)
  stream_model       what a run writes: stdout, the report, the per-record results and the stats — composed from host.py's pure-Python
                     models and the CPU oracle alone
  written_before     of a KX_E_HEADER outcome: the bytes that the windows in front of the failing one have written
  option_sets        every admissible splitter x route pair under a pairwise cover of chomp, ors, header and naming
  stream             about 13 KiB of records suited to an option set: accepted, rejected, too short, without a key, empty
  seam_probes        the short constructs of an option set that carry state across a window's edge
  seam_streams       one stream per byte of a probe: the edge at byte 4096 falls at offset 0, 1, ... len(probe) of it
  populations        what a stream holds, counted from the model alone; FLOORS are asserted against them

No torch, no engine library, no fixtures: nothing here starts the GPU."""
import json
import os
import random

from kleenexlang_amd import host, program_path
from oracle import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ------------------------------------------------------------------------------------------------------------------- programs
FLIP = open(program_path("flip_ab")).read()
GROW = 'main := "<" /[^\\n]*/ ">"\n'                                                  # (the three of test_records_keys_gpu.py)
SOME = 'main := ~/a/ | /aa/ | /b*/ | /ab/\n'
MAP = 'main := (~/_/ " " | ~/-/ "," | ~/%/ "\\"" | /[a-z0-9]/)*\n'
with open(os.path.join(GOLDEN, "action_vectors.json"), encoding="utf-8") as _f:
    ACTION = next(t for t in json.load(_f)["line_tests"] if t["name"] == "actionbug")["program"]   # register actions: lines of c
PROGRAMS = {"flip": FLIP, "grow": GROW, "some": SOME, "map": MAP, "action": ACTION}
# values a program accepts and values it rejects ("grow" rejects a newline alone: _values spells one as the splitter allows)
VALUES = {"flip": ([b"a", b"b", b"ab", b"ba", b"abba", b"bab", b""], [b"c", b"ac", b"bcb"]),
          "some": ([b"a", b"aa", b"b", b"bbb", b"ab", b""], [b"ba", b"aaa", b"abb"]),
          "map": ([b"a", b"ab9", b"a_b", b"a-b", b"a%b", b"z", b""], [b"X", b"aXb", b"Xa"]),
          "grow": ([b"a", b"ab", b"ba", b"abc", b""], []),
          "action": ([b"c", b"cc", b"ccc", b""], [b"x", b"cx", b"cxc"])}
PAD = {"flip": b"a", "some": b"b", "map": b"z", "grow": b"z", "action": b"c"}       # a filler byte the program accepts


def _pad(opt):
    """the filler byte of `opt`: the program's, or where a separator holds that one a z, which ends every partial separator"""
    return PAD[opt.prog] if PAD[opt.prog] not in opt.sep_bytes else b"z"


# -------------------------------------------------------------------------------------------------------------------- options
def _spell(b):
    """bytes as the binary's options spell them: letters and digits as themselves, every other byte as \\xHH"""
    return "".join(chr(c) if chr(c).isalnum() and c < 0x80 else "\\x%02X" % c for c in b)


class Options:
    """The keywords of one record-mode run, and `prog`, the name of the program (PROGRAMS) it is meant for."""
    DEFAULTS = dict(sep=b"\n", quote=None, escape=None, rs=None, chomp=False, ors=b"", field=None, fields=None, fs=None, blanks=False,
                    unquote=False, only=False, ofs=None, header=0, keys=None, optional=())

    def __init__(self, prog="flip", splitter="byte", route="whole", **kw):
        if set(kw) - set(self.DEFAULTS):
            raise TypeError("Options: unknown keywords %r" % sorted(set(kw) - set(self.DEFAULTS)))
        self.__dict__.update(self.DEFAULTS)
        self.__dict__.update(kw)
        self.prog, self.splitter, self.route = prog, splitter, route

    def kwargs(self):
        """the keyword dict of Program.run_records / run_records_fd: what differs from the defaults"""
        return {k: getattr(self, k) for k, d in self.DEFAULTS.items() if getattr(self, k) != d}

    def _list_text(self):
        items = []
        for it in self.fields:
            if isinstance(it, (bytes, bytearray)):
                items.append(_spell(it) + ("?" if self.keys is not None and bytes(it) in self.optional else ""))
            elif isinstance(it, (tuple, list)):
                items.append("%d-%s" % (it[0], "" if it[1] is None else it[1]))
            else:
                items.append(str(it))
        if len(items) == 1 and items[0].isdigit():
            items[0] = "%s-%s" % (items[0], items[0])          # (one plain number would take the single-field path)
        return ",".join(items)

    def args(self):
        """the argument list of the produced binary"""
        a = ["--records" if self.sep == b"\n" else "--records=" + _spell(self.sep)]
        if self.quote is not None:
            a.append("--quote" if self.quote == b'"' else "--quote=" + _spell(self.quote))
        if self.escape is not None:
            a.append("--escape" if self.escape == b"\\" else "--escape=" + _spell(self.escape))
        if self.rs is not None:
            a.append("--rs=" + _spell(self.rs))
        if self.chomp:
            a.append("--chomp")
        if self.ors:
            a.append("--ors=" + _spell(self.ors))
        if self.field is not None:
            a.append("--field=%d" % self.field)
        if self.fields is not None:
            a.append("--field=" + self._list_text())
        if self.fs is not None:
            a.append("--fs=" + _spell(self.fs))
        a += [f for f, on in (("--unquote", self.unquote), ("--blanks", self.blanks), ("--only", self.only)) if on]
        if self.ofs is not None:
            a.append("--ofs=" + _spell(self.ofs))
        if self.header:
            a.append("--header" if self.header == 1 else "--header=%d" % self.header)
        if self.keys is not None:
            a.append("--keys" if self.keys == b"=" else "--keys=" + _spell(self.keys))
        return a

    @property
    def named(self):
        return bool(self.header) and self.keys is None and self.fields is not None and any(isinstance(it, (bytes, bytearray)) for it in self.fields)

    @property
    def sep_bytes(self):
        return self.rs if self.rs is not None else self.sep

    def ident(self):
        """a short label: splitter, route, program and the overlay (c: chomp, oL: ors of L bytes, hN: header, n: by name)"""
        flags = "".join(c for c, on in (("c", self.chomp), ("o%d" % len(self.ors), self.ors), ("h%d" % self.header, self.header), ("n", self.named)) if on)
        return "%s-%s-%s%s" % (self.splitter, self.route, self.prog, "-" + flags if flags else "")

    def __repr__(self):
        return "Options(%s, %s)" % (self.prog, ", ".join("%s=%r" % kv for kv in self.kwargs().items()))


# ---------------------------------------------------------------------------------------------------------------------- model
def _run(blob, doc, cache={}):
    """the CPU oracle on one value: its output, or (pos, stage) of the rejection; memoised by value"""
    k = (blob, doc)
    if k not in cache:
        try:
            cache[k] = oracle.run(blob, doc)
        except oracle.OracleMatchError as e:
            cache[k] = (e.pos, e.stage)
    return cache[k]


def split_model(data, opt, carry=None):
    """(offsets, tail, carry out) of `data` under the splitter of `opt`, from `carry` (None: the stream's start) — the parity or
    state of the quoted and escaped splits, the context of a multi-byte separator.  tail: the last record has no valid separator."""
    if opt.rs is not None:
        offs, ctx, tail_len = host.split_rs_records_model(data, opt.rs, carry or b"")
        return offs, tail_len > 0, ctx
    if opt.escape is not None:
        offs, state = host.split_escaped_records_model(data, opt.sep, opt.quote, opt.escape, carry or 0)
        more = host.split_escaped_records_model(data + b"\0", opt.sep, opt.quote, opt.escape, carry or 0)[0]
    elif opt.quote is not None:
        offs = host.split_records_model(data, opt.sep, opt.quote, carry or 0)
        state = (carry or 0) ^ (data.count(opt.quote) & 1)
        more = host.split_records_model(data + b"\0", opt.sep, opt.quote, carry or 0)
    else:
        offs, state, more = host.split_records_model(data, opt.sep), 0, host.split_records_model(data + b"\0", opt.sep)
    return offs, bool(data) and len(data) not in more[:-1], state       # (one more byte: the end is a boundary iff a separator ends it)


def _lowbit(x):
    return (x & -x).bit_length() - 1


def _printable(name):
    return "".join(chr(c) if 0x20 <= c < 0x7F else "\\x%02X" % c for c in name)


def _header_rows(data, offs, nh, n, tail, sep_len, opt, items, ranges, fs, ofs, special):
    """the entries of the nh header records: copied; with `items` (only=) projected by the identity, a short one reported"""
    chomp, ors, Q, E = opt.chomp, opt.ors, opt.quote, opt.escape
    if items is None:
        out = []
        for i in range(nh):
            cut = 0 if tail and i == n - 1 else sep_len
            out.append((data[offs[i]:offs[i + 1] - cut] + (b"" if chomp else data[offs[i + 1] - cut:offs[i + 1]]) + ors, None))
        return out
    last_whole = tail and nh == n
    if opt.blanks:
        recs = host.blank_field_list_records_model(data, offs[:nh + 1], sep_len, last_whole, ranges, Q, E)
    else:
        recs = host.field_list_records_model(data, offs[:nh + 1], sep_len, last_whole, ranges, fs, Q, E)
    out = []
    for i, m in enumerate(recs):
        if isinstance(m, int):
            out.append((("nofield", m, None), "Record %d has no field %d!\n" % (i + 1, host.field_list_missing(ranges, m))))
            continue
        _, flds, sp = m
        cells = [c for lo, hi in items for K, c in flds if lo <= K and (hi is None or K <= hi)]
        if opt.unquote:
            cells = [host.requote_field_model(host.unquote_field_model(c, Q, E), Q is not None and c[:1] == Q, ofs, Q, E, special) for c in cells]
        out.append((ofs.join(cells) + (b"" if chomp else sp) + ors, None))
    return out


def stream_model(blob, data, opt):
    """Record mode on `data` under `opt` → (stdout bytes, report bytes, per-record results, stats).

    A result is the record's output bytes, ("nofield", fields, name) — a NoFieldError's (fields, field) — or ("match", pos, stage,
    field) — a MatchError's.  stats: records, records_rejected, rejected, header_error (None, or the bytes name that no cell of
    header record N has: KX_E_HEADER, HeaderError), offsets and tail (the split), window_of (written_before's input).  With a
    header error the results are None and stdout holds what the records in front of record N write in all: nothing under only=
    with names (they are held), else their copies; written_before cuts that down to the windows that were complete."""
    o, data = opt, bytes(data)
    Q, E, chomp, ors, blanks, unquote = o.quote, o.escape, o.chomp, o.ors, o.blanks, o.unquote
    offs, tail, _ = split_model(data, o)
    offs = list(offs)
    n, sep_len = len(offs) - 1, len(o.sep_bytes)
    stats = dict(records=n, records_rejected=0, rejected=False, header_error=None, offsets=offs, tail=tail)
    keyed = o.keys is not None
    fs = None if blanks else (o.fs if o.fs is not None else b"\t")
    field, fields = o.field, (None if keyed else o.fields)
    items = ranges = None
    ofs = None
    if o.only:
        ofs = o.ofs if o.ofs is not None else (b" " if blanks else fs)
    if (o.only or unquote or blanks) and field is not None:                            # field=K is the list K-K
        field, fields = None, [field]
    special = o.sep + (b"\t" if blanks else b"")
    written = list(fields) if o.named else None

    def numbers(fl):
        if o.only:
            return host._check_field_items(fl)
        return None, host._check_field_ranges(fl)

    nh = min(o.header, n)
    if fields is not None and not o.named:
        items, ranges = numbers(fields)
    if o.named and n >= o.header:                                                      # record N resolves the names
        cut = 0 if tail and o.header == n else sep_len
        cells = host.header_names_model(data[offs[o.header - 1]:offs[o.header] - cut], fs, Q, E, blanks, o.header == 1)
        try:
            items, ranges = numbers(host.resolve_field_names(written, cells))
        except host.HeaderError as ex:
            head = [] if o.only else _header_rows(data, offs, o.header - 1, n, tail, sep_len, o, None, None, fs, ofs, special)
            stats["header_error"] = ex.name
            return b"".join(h for h, _ in head), b"", None, stats
    rows = []                                                                          # (result, report line or None) per record
    if nh:
        if o.named and n < o.header:                                                   # nothing resolves: held for good, or copied
            rows = [(b"", None)] * nh if o.only else _header_rows(data, offs, nh, n, tail, sep_len, o, None, None, fs, ofs, special)
        else:
            rows = _header_rows(data, offs, nh, n, tail, sep_len, o, items if o.only else None, ranges, fs, ofs, special)
    d_offs, first = offs[nh:], nh + 1
    frame = lambda sp: (b"" if chomp else sp) + ors                                    # noqa: E731
    if n > nh and keyed:
        names = list(dict.fromkeys(bytes(f) for f in o.fields))
        order = [names.index(bytes(f)) for f in o.fields]
        required = sum(1 << t for t, nm in enumerate(names) if nm not in o.optional)
        kofs = ofs
        for i, m in enumerate(host.keyed_records_model(data, d_offs, sep_len, tail, names, o.keys, fs, Q, E, blanks, o.optional)):
            R = first + i
            if isinstance(m, int):
                nm = names[_lowbit(required & ~m)]
                rows.append((("nofield", m, nm), "Record %d has no field %s!\n" % (R, _printable(nm))))
                continue
            gaps, flds, sp = m
            res = [_run(blob, host.unquote_field_model(f, Q, E) if unquote else f) for _, f in flds]
            bad = next((j for j, w in enumerate(res) if isinstance(w, tuple)), None)   # the rejected value at the lowest address
            if bad is not None:
                nm = names[flds[bad][0]]
                rows.append((("match", res[bad][0], res[bad][1], nm),
                             "Match error at input symbol %d in field %s of record %d!\n" % (res[bad][0], _printable(nm), R)))
                continue
            if unquote:
                res = [host.requote_field_model(w, Q is not None and f[:1] == Q, kofs if o.only else b" " if blanks else fs, Q, E, special)
                       for w, (_, f) in zip(res, flds)]
            if o.only:
                by = {t: w for (t, _), w in zip(flds, res)}
                body = kofs.join(by[t] for t in order if t in by)
            else:
                body = b"".join(g + w for g, w in zip(gaps, res + [b""]))
            rows.append((body + frame(sp), None))
    elif n > nh and ranges is not None:
        if blanks:
            recs = host.blank_field_list_records_model(data, d_offs, sep_len, tail, ranges, Q, E)
        else:
            recs = host.field_list_records_model(data, d_offs, sep_len, tail, ranges, fs, Q, E)
        for i, m in enumerate(recs):
            R = first + i
            if isinstance(m, int):
                rows.append((("nofield", m, None), "Record %d has no field %d!\n" % (R, host.field_list_missing(ranges, m))))
                continue
            gaps, flds, sp = m
            res = [_run(blob, host.unquote_field_model(f, Q, E) if unquote else f) for _, f in flds]
            bad = next((j for j, w in enumerate(res) if isinstance(w, tuple)), None)   # the lowest rejected field
            if bad is not None:
                rows.append((("match", res[bad][0], res[bad][1], flds[bad][0]),
                             "Match error at input symbol %d in field %d of record %d!\n" % (res[bad][0], flds[bad][0], R)))
                continue
            if unquote:
                res = [host.requote_field_model(w, Q is not None and f[:1] == Q, ofs if o.only else b" " if blanks else fs, Q, E, special)
                       for w, (_, f) in zip(res, flds)]
            if o.only:
                body = ofs.join(w for lo, hi in items for (K, _), w in zip(flds, res) if lo <= K and (hi is None or K <= hi))
            else:
                body = b"".join(g + w for g, w in zip(gaps, res + [b""]))
            rows.append((body + frame(sp), None))
    elif n > nh and field is not None:
        for i, m in enumerate(host.field_records_model(data, d_offs, sep_len, tail, field, fs, Q, E)):
            R = first + i
            if isinstance(m, int):
                rows.append((("nofield", m, None), "Record %d has no field %d!\n" % (R, field)))
                continue
            w = _run(blob, m[1])
            if isinstance(w, tuple):
                rows.append((("match", w[0], w[1], None), "Match error at input symbol %d in record %d!\n" % (w[0], R)))
            else:
                rows.append((m[0] + w + m[2] + frame(m[3]), None))
    elif n > nh:
        for i, doc in enumerate(host.chomp_records_model(data, d_offs, sep_len if chomp else 0, tail)):
            w = _run(blob, doc)
            if isinstance(w, tuple):
                rows.append((("match", w[0], w[1], None), "Match error at input symbol %d in record %d!\n" % (w[0], first + i)))
            else:
                rows.append((w + ors, None))
    assert len(rows) == n
    results = [r for r, _ in rows]
    stats["records_rejected"] = sum(1 for r in results if not isinstance(r, bytes))
    stats["rejected"] = stats["records_rejected"] > 0
    return b"".join(r for r in results if isinstance(r, bytes)), "".join(ln for _, ln in rows if ln).encode(), results, stats


def window_of(offs, tail, size, window):
    """the window (of `window` bytes) in which each record is run: the one that holds its last byte; the tail in the last window"""
    last = max(0, (size - 1) // window)
    n = len(offs) - 1
    return [last if tail and i == n - 1 else (offs[i + 1] - 1) // window for i in range(n)]


def written_before(data, opt, window, stats):
    """Of a header-error outcome (stats of stream_model): the bytes on stdout when the run ends.  A window's output is written when
    the window is done, and the window in which record N ends is never done: what is written is what the records of the windows in
    front of it give — their copies, or nothing under only= (they are held until the names are resolved)."""
    if opt.only:
        return b""
    offs, tail = stats["offsets"], stats["tail"]
    win = window_of(offs, tail, len(data), window)
    sep_len = len(opt.sep_bytes)
    rows = _header_rows(data, offs, opt.header - 1, len(offs) - 1, tail, sep_len, opt, None, None, None, None, None)
    return b"".join(r for i, (r, _) in enumerate(rows) if win[i] < win[opt.header - 1])


# ---------------------------------------------------------------------------------------------------------------- option sets
SPLITTERS = [("byte", {}), ("quoted", dict(quote=b'"')), ("escq", dict(quote=b'"', escape=b"\\")), ("esc", dict(escape=b"\\")),
             ("rs1", dict(rs=b";")), ("rsn", dict(rs=b";:")), ("rso", dict(rs=b"aba"))]
LISTS = [[2, (4, None)], [1, 3], [(2, 3), 5], [6]]                                     # an open range; an item some records lack
ONLY_LISTS = [[3, 1, 3], [(4, None), 1, (1, 2)], [4, 2], [(4, 5), (5, 6)]]             # repeated, open, overlapping
NAME_LISTS = [[b"name", b"k5"], [b"city", 2], [b"id", (5, None)]]
ONLY_NAME_LISTS = [[b"city", b"id", b"city"], [b"k5", (6, None), b"name"], [b"name", 1]]
HEADER_CELLS = [b"id", b"name", b"city", b"name", b"k5", b"k6", b"k7"]                 # (a duplicate: the lowest wins)
KEY_NAMES = [b"k", b"m"]
# route → (needs a quote or an escape, the keywords it adds)
ROUTES = [("whole", False, {}), ("field", False, dict(field=2, fs=b",")), ("list", False, dict(fields=LISTS, fs=b",")),
          ("list+unquote", True, dict(fields=LISTS, fs=b",", unquote=True)), ("blanks", False, dict(fields=LISTS, blanks=True)),
          ("blanks+unquote", True, dict(fields=LISTS, blanks=True, unquote=True)),
          ("only", False, dict(fields=ONLY_LISTS, fs=b",", only=True)), ("only+blanks", False, dict(fields=ONLY_LISTS, blanks=True, only=True)),
          ("only+unquote", True, dict(fields=ONLY_LISTS, fs=b",", only=True, unquote=True)),
          ("only+blanks+unquote", True, dict(fields=ONLY_LISTS, blanks=True, only=True, unquote=True)),
          ("keys", False, dict(fields=[b"k", b"m"], keys=b"=", fs=b",")),
          ("keys+blanks", False, dict(fields=[b"m", b"k"], keys=b":", blanks=True)),
          ("keys+unquote", True, dict(fields=[b"k", b"m"], keys=b"=", fs=b",", unquote=True)),
          ("keys+only", False, dict(fields=[b"m", b"k", b"m"], keys=b"=", fs=b",", only=True)),
          ("keys+optional", False, dict(fields=[b"k", b"m"], keys=b"=", fs=b",", optional=(b"m",))),
          ("keys+blanks+unquote+only+optional", True, dict(fields=[b"m", b"k", b"m"], keys=b":", blanks=True, unquote=True, only=True, optional=(b"m",)))]
ORS = [b"", b"\n", b"<<eor>>\n"]
OFS = [None, b"|", b"", b"<-ofs->>"]                                                   # (on values: the default, or one byte)


def overlay(route, kw):
    """The rows (chomp, ors, header, named) that lie over a route: a pairwise cover of the dimensions the route admits, picked
    greedily from their product in a fixed order."""
    keyed = "keys" in kw
    headers = [0] if keyed else [0, 1, 3]
    prod = [(c, s, h, nm) for c in (False, True) for s in range(3) for h in headers
            for nm in ((False, True) if h and "fields" in kw else (False,))]
    pairs = lambda row: {(a, row[a], b, row[b]) for a in range(4) for b in range(a + 1, 4)}   # noqa: E731
    need = set().union(*(pairs(r) for r in prod))
    rows = []
    while need:
        best = max(prod, key=lambda r: len(pairs(r) & need))                           # (max keeps the first of equals)
        rows.append(best)
        need -= pairs(best)
    return rows


def _program(splitter, route, chomp, k):
    rs = splitter.startswith("rs")
    if route == "whole":
        cand = (["flip", "grow"] if rs else ["flip", "some", "action"]) if chomp else (["grow"] if rs else ["flip", "action"])
    elif "unquote" in route:
        cand = ["map", "flip"]
    else:
        cand = ["flip", "some"] + ([] if splitter == "byte" else ["grow"])
    return cand[k % len(cand)]


def option_sets():
    """The product: every admissible pairing of splitter and route, each under some rows of the route's overlay so that over the
    route's splitters every row occurs; then three sets whose header row lacks a name (KX_E_HEADER)."""
    sets, k = [], 0
    for route, needs, kw in ROUTES:
        splitters = [s for s in SPLITTERS if not needs or "quote" in s[1] or "escape" in s[1]]
        rows = overlay(route, kw)
        per = -(-len(rows) // len(splitters))
        per = max(per, 2 if len(rows) > len(splitters) else 1)
        for si, (sname, skw) in enumerate(splitters):
            for j in range(per):
                chomp, s, header, named = rows[(si * per + j) % len(rows)]
                o = dict(skw, **kw)
                if "fields" in o and "keys" not in o:
                    pool = (ONLY_NAME_LISTS if o.get("only") else NAME_LISTS) if named else o["fields"]
                    o["fields"] = pool[k % len(pool)]
                if o.get("only"):
                    o["ofs"] = (None, b"|")[k % 2] if o.get("unquote") else OFS[k % 4]
                    if o["ofs"] is None:
                        del o["ofs"]
                if s or chomp:
                    o.update(chomp=chomp, ors=ORS[s])
                if header:
                    o["header"] = header
                sets.append(Options(_program(sname, route, chomp, k), sname, route, **o))
                k += 1
    sets.append(Options("flip", "byte", "list", fields=[b"name", b"nope"], fs=b",", header=1))
    sets.append(Options("flip", "quoted", "only", quote=b'"', fields=[b"nope", b"id"], fs=b",", only=True, header=3, chomp=True, ors=b"\n"))
    sets.append(Options("some", "rsn", "blanks", rs=b";:", fields=[b"id", b"none"], blanks=True, header=3))
    return sets


# -------------------------------------------------------------------------------------------------------------------- streams
def _values(opt):
    good, bad = VALUES[opt.prog]
    if opt.prog == "grow":                                                             # a newline where the splitter lets one stand
        nl = b"a\nb" if opt.rs is not None else b'"a\nb"' if opt.quote is not None else b"a" + opt.escape + b"\nb" if opt.escape is not None else None
        bad = [nl] if nl else []
    return good, bad


def _value(r, opt, bad):
    """one value; now and then dressed with what the splitter and the field rules must see through: quotes around a field or a
    record separator, a doubled quote, escaped separators, quotes and escapes, a proper prefix of a multi-byte separator"""
    good, badv = _values(opt)
    v = r.choice(badv) if bad and badv else r.choice(good)
    Q, E, k = opt.quote, opt.escape, r.random()
    F = b" " if opt.blanks else (opt.fs or b",")
    if Q is not None and k < 0.15:
        v = Q + v[:1] + r.choice([b"", F, opt.sep, Q + Q, b""]) + v[1:] + Q
    elif E is not None and 0.15 <= k < 0.27:
        v = v[:1] + E + r.choice([opt.sep, E, Q or b"a", F]) + v[1:]
    elif opt.rs is not None and len(opt.rs) > 1 and 0.27 <= k < 0.37:
        v += opt.rs[:r.randrange(1, len(opt.rs))]
    return v


def _body(r, opt, kind):
    """a record's body of a kind: ok, bad (a rejected value), short (too few fields, or without a required key), empty"""
    if kind == "empty":
        return b""
    if opt.field is None and opt.fields is None:
        return _value(r, opt, kind == "bad")
    nf = r.randrange(1, 3) if kind == "short" else r.randrange(6, 9)
    vals = [_value(r, opt, kind == "bad" and r.random() < 0.7) for _ in range(nf)]
    if opt.blanks and opt.keys is None:
        vals = [v for v in vals if v] or [_pad(opt)]                                   # (a word is never empty)
    if opt.keys is not None:
        names = list(dict.fromkeys(opt.fields))
        keys = [b"x", b"kk"] if kind == "short" else [nm for nm in names if nm not in opt.optional or r.random() < 0.7]
        r.shuffle(keys)
        keys += [r.choice([b"x", b"k", b"m", b"kk", None]) for _ in range(len(vals) - len(keys))]
        vals = [(k + opt.keys if k is not None else b"") + v for k, v in zip(keys, vals)]
    if opt.blanks:
        join = lambda: r.choice([b" ", b"  ", b"\t", b" \t "])                          # noqa: E731
        return r.choice([b"", b"", b" "]) + b"".join(v + join() for v in vals[:-1]) + vals[-1] + r.choice([b"", b"", b"\t"])
    return (opt.fs or b"\t").join(vals)


def _header(r, opt):
    """the bodies of the header records: notes in front, the names in record N (one of them quoted where there is a quote)"""
    F = b"  " if opt.blanks else (opt.fs or b"\t")
    cells = list(HEADER_CELLS)
    if opt.quote is not None:
        cells[1] = opt.quote + cells[1] + opt.quote
    return [F.join([b"#", b"note%d" % i] + [b"x"] * (i % 3)) for i in range(1, opt.header)] + [F.join(cells)]


KINDS = ("ok",) * 10 + ("bad",) * 4 + ("short",) * 3 + ("empty",) * 2


def _records(r, opt, nbytes):
    """records of random kinds, separators included, until `nbytes` are reached"""
    out, n = [], 0
    while n < nbytes:
        rec = _body(r, opt, r.choice(KINDS)) + opt.sep_bytes
        out.append(rec)
        n += len(rec)
    return out


def stream(opt, seed, nbytes=13000):
    """About `nbytes` of records suited to `opt` (header records first); the last record is filler bytes, on odd seeds without
    a separator."""
    r = random.Random("%s/%d" % (opt.ident(), seed))
    recs = [b + opt.sep_bytes for b in _header(r, opt)] if opt.header else []
    recs += _records(r, opt, nbytes - sum(map(len, recs)))
    recs.append(_pad(opt) * 3 + (b"" if seed & 1 else opt.sep_bytes))
    return b"".join(recs)


def sweep_sets():
    """The option sets of the seam sweep: one per splitter x route pair — of those in option_sets() that name no column the one
    whose list asks least of a record — and per splitter two that resolve names, with header 1 and with header 3, on routes that
    differ from splitter to splitter."""
    top = lambda o: max([it if isinstance(it, int) else it[1] or it[0] for it in (o.fields or []) if not isinstance(it, (bytes, bytearray))] or [0])   # noqa: E731
    pairs = {}
    for o in option_sets()[:-3]:
        if not o.named and ((o.splitter, o.route) not in pairs or top(o) < top(pairs[o.splitter, o.route])):
            pairs[o.splitter, o.route] = o
    for o in option_sets()[:-3]:                                                       # (a pair that names columns in all its sets)
        if (o.splitter, o.route) not in pairs:
            pairs[o.splitter, o.route] = Options(o.prog, o.splitter, o.route, **dict(o.kwargs(), fields=(ONLY_LISTS[2] if o.only else LISTS[1])))
    out = list(pairs.values())
    routes = {r: kw for r, _, kw in ROUTES}
    for i, (sname, skw) in enumerate(SPLITTERS):
        for j, N in enumerate((1, 3)):
            route = ["list", "only", "blanks", "only+blanks"][(i + j) % 4] + ("+unquote" if skw and "rs" not in skw and (i + j) % 2 else "")
            kw = dict(skw, **routes[route])
            kw["fields"] = (ONLY_NAME_LISTS if kw.get("only") else NAME_LISTS)[(i + j) % 3]
            if kw.get("unquote") and kw.get("only"):
                kw["ofs"] = b"|"
            out.append(Options("map" if kw.get("unquote") else "flip", sname, route, header=N, chomp=bool(j), ors=ORS[(i + j) % 3], **kw))
    return out


# ----------------------------------------------------------------------------------------------------------------- seam probes
def seam_probes(opt):
    """(name, kind, bytes) of the constructs of `opt` that carry state across a window's edge, at most about 40 bytes each.  kind
    "records": the probe begins a record; "header": the probe begins inside header record N (N = 1) or ends header record N - 1
    (N = 3), and seam_streams builds the header records around it."""
    Q, E, S = opt.quote, opt.escape, opt.sep_bytes
    F = b" " if opt.blanks else (opt.fs or b",")
    g = VALUES[opt.prog][0]
    a, b = g[0], g[2]
    fielded = opt.field is not None or opt.fields is not None
    kv = (lambda k, v: k + opt.keys + v) if opt.keys is not None else (lambda k, v: v)
    row = lambda *vals: F.join(kv(k, v) for k, v in zip([b"k", b"m", b"x", b"kk", b"y"], vals)) if fielded else b"".join(vals)   # noqa: E731
    full = lambda *vals: row(*(vals + (a,) * ((3 if opt.keys is not None else 5) - len(vals))))   # noqa: E731
    probes = []
    if Q is not None:                                                                  # a quoted field with the separator and ""
        probes.append(("quoted separator", "records", full(a, Q + a + S + b + Q + Q + a + Q) + S))
    if E is not None:                                                                  # an escape before a separator, a quote, an escape
        probes.append(("escapes", "records", full(a + E + S + b, a + E + (Q or b"q") + b, a + E + E) + S))
    if opt.rs is not None and len(opt.rs) > 1:
        probes.append(("separator bytes", "records", full(a, b) + S + S))
        if opt.rs == b"aba":
            probes.append(("overlapping separator", "records", b"b" + b"ababa" + b"b" + S + b"bab" + b"ababab" + S))
    if opt.blanks:
        probes.append(("blanks", "records", b" \t " + full(a, b).replace(b" ", b"  \t \t  ", 2) + b" \t" + S))
    if opt.keys is not None:
        probes.append(("key and value", "records", full(b + a + b, a + b) + S))
    if opt.unquote and Q is not None and opt.prog == "map":                            # " and , in the output: the spelling changes
        probes.append(("respelled value", "records", full(b"a", Q + b"a%b-c" + Q, b"a-b") + S))
    if opt.named and opt.header in (1, 3):
        cells = list(HEADER_CELLS)
        if Q is not None:
            cells[1] = Q + cells[1] + Q
        probes.append(("header names", "header", (F if opt.header == 1 else S) + F.join(cells) + S + F.join([a] * 7) + S))
    if not probes:                                                                     # (the byte splitter's only state: the carried record)
        probes.append(("plain record", "records", full(a, b) + S))
    return probes


def seam_streams(opt, probe, edge=4096, total=9216):
    """[(pos, stream)] for pos = 0 … len(probe): filler, the probe, filler, with the edge at byte `edge` of the stream at offset
    `pos` of the probe.  The filler in front is whole records, the last one padded to the byte; for a "header" probe it is the
    header records themselves — record N - 1 (N = 3), or the first cell of record N (N = 1), made as long as it takes."""
    name, kind, pb = probe
    S, P = opt.sep_bytes, _pad(opt)
    r = random.Random("%s/%s" % (opt.ident(), name))
    if kind == "header":
        front = b"".join(b + S for b in _header(r, opt)[:-2])                           # N = 3: record 1, then record 2, the long one, which
        fill = b"#" if opt.header == 3 else b"c"                                        # the probe ends (N = 1: the long first cell of record 1)
    else:
        recs = [b + S for b in _header(r, opt)] if opt.header else []
        front = b"".join(recs + _records(r, opt, edge - len(pb) - 80 - sum(map(len, recs))))
    tail = b"".join(_records(r, opt, total - edge))
    out = []
    for pos in range(len(pb) + 1):
        lead = edge - pos
        head = front + fill * (lead - len(front)) if kind == "header" else front + P * (lead - len(front) - len(S)) + S
        assert len(head) == lead, (len(head), lead)
        out.append((pos, head + pb + tail))
    return out


# ----------------------------------------------------------------------------------------------------------------- populations
def populations(data, opt, results, stats, window=4096):
    """({kind: count}, [{kind: count} per window]) of a stream, from the model alone.  Kinds: accepted, rejected (a value the
    program rejects), short (too few fields, or no required key), empty (an empty body), header."""
    offs, tail = stats["offsets"], stats["tail"]
    win = window_of(offs, tail, len(data), window)
    total, per = {}, [dict() for _ in range(max(win, default=0) + 1)]
    sep_len = len(opt.sep_bytes)
    for i, res in enumerate(results):
        kinds = ["header" if i < opt.header else "accepted" if isinstance(res, bytes) else "short" if res[0] == "nofield" else "rejected"]
        if offs[i + 1] - offs[i] == (0 if tail and i == len(results) - 1 else sep_len):
            kinds.append("empty")
        for k in kinds:
            total[k] = total.get(k, 0) + 1
            per[win[i]][k] = per[win[i]].get(k, 0) + 1
    return total, per


def carry_positions(opt, streams, edge=4096):
    """(split, cut): at how many of a probe's positions the model's split changes when the carry at the edge is dropped (the second
    window split from the start state), and at how many the edge falls inside a record (the record must be carried)"""
    split = cut = 0
    for _, data in streams:
        carry = split_model(data[:edge], opt)[2]
        split += list(split_model(data[edge:], opt, carry)[0]) != list(split_model(data[edge:], opt)[0])
        cut += edge not in split_model(data, opt)[0]
    return split, cut


# Asserted by test_records_stream.py, which prints the figures it measures from the model.  "streams": four fifths of the minimum
# over the option sets and both seeds (measured: 90 accepted, 72 with a rejected value, 93 too short or without a key, 26 empty
# records in a stream; in its poorest 4 KiB window 3 accepted and 9 rejected ones, the too short among them).  "probes": per probe
# the fewest positions, over the sweep's option sets, at which (the second window's split changes without the carry, the edge falls
# inside a record), as measured.
FLOORS = {"streams": {"accepted": 72, "rejected": 57, "short": 74, "empty": 20, "window accepted": 2, "window rejected": 7},
          "probes": {"plain record": (0, 6), "quoted separator": (6, 12), "escapes": (1, 13), "separator bytes": (2, 8),
                     "overlapping separator": (10, 17), "respelled value": (6, 17), "blanks": (0, 26), "key and value": (0, 14),
                     "header names": (0, 40)}}
