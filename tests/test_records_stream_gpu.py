"""GPU: record mode against ONE model.  Every option set of recstream.option_sets() — each admissible splitter x route pair under a
pairwise cover of chomp, ors, header and naming — runs through Program.run_records_fd (a regular file at windows of 4096, 8192 and
the default, a pipe at 4096) and Program.run_records, and the window edge at byte 4096 is swept through every byte of the constructs
that carry state (recstream.seam_probes).  Every comparison is byte-exact against recstream.stream_model: stdout, the report lines,
the per-record results and the stats."""
import os

import pytest
import recstream as rs
from conftest import blob_of

import test_records_field_gpu as single
from kleenexlang_amd.host import EngineError, HeaderError, MatchError, NoFieldError, Program

pytestmark = pytest.mark.gpu

SETS = rs.option_sets()
SWEEP = rs.sweep_sets()
O = rs.Options
_PROGS = {}


def _prog(opt, window):
    k = (opt.prog, window)
    if k not in _PROGS:
        _PROGS[k] = Program(blob_of(rs.PROGRAMS[opt.prog]), window_bytes=window)
    return _PROGS[k]


def _model(opt, data, cache={}):
    k = (opt.prog, repr(opt), data)
    if k not in cache:
        cache.clear()                                                                   # (one stream at a time: its runs share the model)
        cache[k] = rs.stream_model(blob_of(rs.PROGRAMS[opt.prog]), data, opt)
    return cache[k]


def _fd(prog, opt, data, tmp_path, pipe=False):
    """run_records_fd over files (pipe: the input through a pipe) → (the stats, or the EngineError; stdout bytes; report bytes)"""
    paths = [str(tmp_path / n) for n in ("in", "out", "rep")]
    if pipe:
        fin, wr = os.pipe()
        assert len(data) <= 60000                                                       # (fits the pipe: written before the run reads)
        os.write(wr, data)
        os.close(wr)
    else:
        with open(paths[0], "wb") as f:
            f.write(data)
        fin = os.open(paths[0], os.O_RDONLY)
    fout = os.open(paths[1], os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    frep = os.open(paths[2], os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    try:
        res = prog.run_records_fd(fin, fout, report_fd=frep, **opt.kwargs())
    except EngineError as e:
        res = e
    finally:
        for fd in (fin, fout, frep):
            os.close(fd)
    with open(paths[1], "rb") as fo, open(paths[2], "rb") as fr:
        return res, fo.read(), fr.read()


def _first_diff(a, b):
    i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return i, a[max(0, i - 30):i + 30], b[max(0, i - 30):i + 30]


def check_fd(opt, data, window, tmp_path, pipe=False, ctx=None):
    """one run_records_fd against the model: stdout, the report, the return and the stats"""
    out, err, res, st = _model(opt, data)
    got, gout, gerr = _fd(_prog(opt, window), opt, data, tmp_path, pipe)
    ctx = (opt, window, pipe, ctx)
    if st["header_error"] is not None:
        assert isinstance(got, EngineError) and 'no cell of header record %d is named "%s"' % (opt.header, rs._printable(st["header_error"])) in str(got), (ctx, got)
        assert (gout, gerr) == (rs.written_before(data, opt, window or 1 << 30, st), b""), ctx
        return
    assert not isinstance(got, EngineError), (ctx, got)
    assert gerr == err, (ctx, _first_diff(gerr, err))
    assert gout == out, (ctx, _first_diff(gout, out))
    windows = max(1, -(-len(data) // window)) if window else 1
    assert (got["records"], got["records_rejected"], got["rejected"], got["windows"], got["in_bytes"], got["out_bytes"]) == \
        (st["records"], st["records_rejected"], st["rejected"], windows, len(data), len(out)), (ctx, got)


def _norm(res):
    return [("nofield", g.fields, g.field) if isinstance(g, NoFieldError) else ("match", g.pos, g.stage, g.field) if isinstance(g, MatchError) else g
            for g in res]


def check_records(opt, data):
    """Program.run_records on the same bytes: the per-record results"""
    _, _, res, st = _model(opt, data)
    prog = _prog(opt, 0)
    if st["header_error"] is not None:
        with pytest.raises(HeaderError) as e:
            prog.run_records(data, **opt.kwargs())
        assert e.value.name == st["header_error"], opt
        return
    got = _norm(prog.run_records(data, **opt.kwargs()))
    assert len(got) == len(res) and got == res, (opt, next((i, g, w) for i, (g, w) in enumerate(zip(got, res)) if g != w))


# ---------------------------------------------------------------------------------------------------------- a. the product
@pytest.mark.parametrize("k", range(len(SETS)), ids=["%03d-%s" % (k, o.ident()) for k, o in enumerate(SETS)])
def test_every_option_set_on_every_driver(k, tmp_path):
    opt = SETS[k]
    data = rs.stream(opt, k & 1)                                                        # (odd: a tail without a separator)
    for window in (4096, 8192, 0):
        check_fd(opt, data, window, tmp_path)
    check_fd(opt, data, 4096, tmp_path, pipe=True)
    check_records(opt, data)
    _, _, res, st = _model(opt, data)
    assert st["header_error"] is not None or {bytes, tuple} == {type(r) for r in res}


# ---------------------------------------------------------------------------------------------------------- b. the seam sweep
PROBES = [(k, p) for k, o in enumerate(SWEEP) for p in rs.seam_probes(o) if not o.named or p[1] == "header"]


@pytest.mark.parametrize("j", range(len(PROBES)), ids=["%02d-%s-%s" % (k, SWEEP[k].ident(), p[0].replace(" ", "_")) for k, p in PROBES])
def test_the_window_edge_at_every_byte_of_a_probe(j, tmp_path):
    """one probe of one option set: the edge at every byte of it (tens of runs), the middle position once more in one 8 KiB window"""
    k, probe = PROBES[j]
    opt = SWEEP[k]
    streams = rs.seam_streams(opt, probe)
    for pos, data in streams:
        check_fd(opt, data, 4096, tmp_path, ctx=(probe[0], pos))
    pos, data = streams[len(streams) // 2]
    check_fd(opt, data, 8192, tmp_path, ctx=(probe[0], pos))
    check_records(opt, data)


def test_every_sweep_set_has_a_probe():
    assert {k for k, _ in PROBES} == set(range(len(SWEEP)))


# ---------------------------------------------------------------------------------------------------------- c. lengths
ROUTES = {"whole+chomp": O("flip", chomp=True, ors=b"|"),
          "only+blanks": O("flip", "byte", "only+blanks", fields=[3, 1], blanks=True, only=True, ofs=b"-"),
          "keys": O("flip", "byte", "keys", fields=[b"k", b"m"], keys=b"=", fs=b",", optional=(b"m",))}


def _record(route, r, n=None):
    """record r of a route's filler (every seventh holds a rejected value); with n, one of exactly n bytes without its separator,
    the bytes it takes inside a value the program runs on"""
    v = b"c" if r % 7 == 3 else b"ab"[:1 + r % 2]
    parts = {"whole+chomp": (v * 3, b""), "only+blanks": (v + b"  a\t" + v, b" b"), "keys": (b"x=1,k=" + v, b",m=b" + v)}[route]
    more = 0 if n is None else n - len(parts[0]) - len(parts[1])
    assert more >= 0
    return parts[0] + (b"ab" * (more // 2 + 1))[:more] + parts[1]


def _exactly(route, nbytes, sep):
    """records of the route that sum to exactly `nbytes`; sep: the last one ends in a separator"""
    recs, total, r = [], 0, 0
    while nbytes - total > 60:
        recs.append(_record(route, r) + b"\n")
        total += len(recs[-1])
        r += 1
    recs.append(_record(route, r, nbytes - total - (1 if sep else 0)) + (b"\n" if sep else b""))
    data = b"".join(recs)
    assert len(data) == nbytes
    return data


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_stream_lengths_around_the_window_size(route, tmp_path):
    opt = ROUTES[route]
    for k in (1, 2):
        for n in (4096 * k - 1, 4096 * k, 4096 * k + 1):
            for sep in (True, False):
                data = _exactly(route, n, sep)
                _, _, res, st = _model(opt, data)
                assert st["tail"] == (not sep) and {bytes, tuple} == {type(x) for x in res}
                check_fd(opt, data, 4096, tmp_path, ctx=(n, sep))
                check_fd(opt, data, 4096, tmp_path, pipe=True, ctx=(n, sep))
                check_records(opt, data)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_long_records_and_tiny_streams(route, tmp_path):
    """a record longer than two windows, with no separator inside: as the first record, as the tail, directly behind a header row;
    the empty stream; a stream that is one separator"""
    opt = ROUTES[route]
    long = _record(route, 0, 9000)
    some = b"".join(_record(route, r) + b"\n" for r in range(40))
    header = O(opt.prog, opt.splitter, opt.route, **dict(opt.kwargs(), header=1)) if route != "keys" else None   # (keys= comes without header=)
    cases = [(opt, long + b"\n" + some), (opt, some + long), (opt, long), (opt, b""), (opt, b"\n"), (opt, b"\n\n" + some)]
    if header is not None:
        cases += [(header, b"h1 h2 h3\n" + long + b"\n" + some), (header, long + b"\n" + some), (header, b"h1 h2 h3"), (header, b"")]
    for o, data in cases:
        for window in (4096, 8192):
            check_fd(o, data, window, tmp_path, ctx=len(data))
        check_fd(o, data, 4096, tmp_path, pipe=True, ctx=len(data))
        check_records(o, data)
    assert _model(opt, long)[3]["records"] == 1 and isinstance(_model(opt, long)[2][0], bytes)


@pytest.mark.parametrize("only", [False, True])
def test_fewer_records_than_header_rows_and_a_name_that_is_missing(only, tmp_path):
    """by name: a stream shorter than `header` rows resolves nothing — under only= the rows are held for good, else copied; a name
    that no cell has ends the run, and what the windows in front of record N's have written stays written"""
    kw = dict(fields=[b"name", b"id"], blanks=True, header=3, chomp=True, ors=b"|")
    if only:
        kw.update(only=True, ofs=b"-")
    opt = O("flip", "byte", "only+blanks" if only else "blanks", **kw)
    for data in (b"id name\n", b"id name\nid name", b"x\n" + b"#" * 9000, b"x\n" + b"#" * 9000 + b"\n"):
        out, _, res, st = _model(opt, data)
        assert st["header_error"] is None and (out == b"") == only and st["records"] in (1, 2)
        for window in (4096, 0):
            check_fd(opt, data, window, tmp_path, ctx=data[:20])
        check_records(opt, data)
    rows = b"".join(b"a ab b\n" for _ in range(30))
    for data in (b"x\n" + b"#" * 9000 + b"\nid nam\n" + rows, b"x\ny\nid nam\n" + rows, b"x\n" + b"#" * 4090 + b"\nid nam"):
        st = _model(opt, data)[3]
        assert st["header_error"] == b"name"
        if data[:3] != b"x\ny":                                                          # record 1 — in the last case record 2 as well — is written
            assert rs.written_before(data, opt, 4096, st) == (b"" if only else b"x|" if len(data) > 9000 else b"x|" + b"#" * 4090 + b"|")
        for window in (4096, 8192, 0):
            check_fd(opt, data, window, tmp_path, ctx=data[:20])
        check_fd(opt, data, 4096, tmp_path, pipe=True)
        check_records(opt, data)


# ---------------------------------------------------------------------------------------------------------- d. the binary
# one option set per branch of RecordsRun::runPart and way of placing header rows, spread over the splitters
BINARY = [("byte", "whole", lambda o: o.header), ("quoted", "list+unquote", lambda o: o.named),
          ("escq", "only+blanks+unquote", lambda o: o.named), ("esc", "blanks", lambda o: o.header and not o.named),
          ("rs1", "field", lambda o: o.header), ("rsn", "keys+only", lambda o: True), ("rso", "only", lambda o: o.header and not o.named),
          ("quoted", "keys+blanks+unquote+only+optional", lambda o: o.chomp)]


def _pick(splitter, route, want):
    mine = [o for o in SETS if (o.splitter, o.route) == (splitter, route) and want(o)]
    assert mine, (splitter, route)                                                      # (the product still holds the variant this case is for)
    return mine[0]


@pytest.mark.parametrize("k", range(len(BINARY)), ids=["%s-%s" % b[:2] for b in BINARY])
def test_the_produced_binary_on_the_same_streams(k, tmp_path_factory):
    opt = _pick(*BINARY[k])
    exe = single._bin(tmp_path_factory, rs.PROGRAMS[opt.prog])
    data = rs.stream(opt, 1)
    out, err, res, st = _model(opt, data)
    assert st["header_error"] is None and st["rejected"]
    for window in (4096, 1 << 30):
        r = single._run_bin(exe, opt.args(), data, window)
        assert (r.returncode, r.stderr) == (1, err), (opt.args(), window, r.returncode, _first_diff(r.stderr, err))
        assert r.stdout == out, (opt.args(), window, _first_diff(r.stdout, out))
