"""GPU: programs with approximated terms (`t<k>`) on the HIP engine, bit-exact with the CPU oracle.

These transducers have shapes no other test gives the engine: many alternatives alive at once (one per error budget and edit),
error budgets carried across segment and window boundaries, and context decided at the end of a region (the fallback alternative
of a line is only ruled out at its newline)."""
import os
import random
import subprocess
import zlib

import pytest

from kleenexlang_amd import MatchError, Program, build, host
from oracle import oracle

pytestmark = pytest.mark.gpu

KEXC = os.path.join(build.OUT, "kexc")
METRICS = ("LCS", "Hamming", "Levenshtein")
MODES = ("correction", "matching", "explicit")

# (name, source, word approximated, k, has a fallback alternative)
PROGRAMS = [
    # a line within two edits of "kleenex" is corrected and bracketed; any other line is copied
    ("bracket", 'main := (line /\\n/)*\nline := "<" /kleenex/<2> ">" | /[^\\n]*/\n', "kleenex", 2, True),
    # a key within one edit of "name" is rewritten; the "=" after it ends the approximated region
    ("keyval", 'main := (kv /\\n/)*\nkv := key /=/ /[a-z0-9]*/\nkey := "NAME:" /name/<1> | /[a-z]+/\n', "name", 1, True),
    # no fallback: a line beyond one edit is a match error
    ("strict", "main := (/kleenex/<1> /\\n/)*\n", "kleenex", 1, False),
]


@pytest.fixture(autouse=True, params=["delayed", "general"])
def engine_mode(request, monkeypatch):
    """Both engine forms, as in test_engine_gpu.py: the delayed form where a stage has one, and the general engine only (KX_DF=0)."""
    if request.param == "general":
        monkeypatch.setenv("KX_DF", "0")
    else:
        monkeypatch.delenv("KX_DF", raising=False)
    return request.param


_BLOBS = {}


def blob(src, metric, mode):
    key = (src, metric, mode)
    if key not in _BLOBS:
        b = host.compile_flags(src, metric=metric, approx_mode=mode)
        host.validate_blob(b)
        _BLOBS[key] = b
    return _BLOBS[key]


def edited(word, nedits, rng, alpha="abcdeklnxyz"):
    w = list(word)
    for _ in range(nedits):
        op = rng.randrange(3)
        if op == 0 or not w:
            w.insert(rng.randint(0, len(w)), rng.choice(alpha))
        elif op == 1:
            del w[rng.randrange(len(w))]
        else:
            w[rng.randrange(len(w))] = rng.choice(alpha)
    return "".join(w)


def make_input(name, word, k, size, seed):
    """Seeded lines, each the program's word with 0..k+1 random edits (and, for keyval, a key=value line)."""
    rng = random.Random(seed)
    lines, n = [], 0
    while n < size:
        w = edited(word, rng.randint(0, k + 1), rng)
        if name == "keyval":
            if not w.isalpha() or not w.islower():
                w = "".join(c for c in w if "a" <= c <= "z") or "x"
            w += "=" + "".join(rng.choice("ab01") for _ in range(rng.randint(0, 6)))
        lines.append(w)
        n += len(w) + 1
    return ("\n".join(lines) + "\n").encode()


def both(b, data, **cfg):
    """(engine result, oracle result); a result is bytes or ('fail', position)."""
    try:
        want = oracle.run(b, data)
    except oracle.OracleMatchError as e:
        want = ("fail", e.pos)
    p = Program(b, **cfg)
    try:
        got = p.run_host(data)
    except MatchError as e:
        got = ("fail", e.pos)
    finally:
        p.close()
    return got, want


def simulate(src, tmp_path, data, metric, mode):
    f = tmp_path / "p.kex"
    f.write_text(src)
    r = subprocess.run([KEXC, "simulate", "--sim", "lockstep", "--metric", metric, "--approxmode", mode, str(f)], input=data,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.stdout if r.returncode == 0 else None


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("prog", PROGRAMS, ids=lambda p: p[0])
def test_engine_matches_oracle(prog, metric, mode, tmp_path):
    name, src, word, k, fallback = prog
    b = blob(src, metric, mode)
    seed = zlib.crc32((name + metric + mode).encode()) & 0xFFFF
    data = make_input(name, word, k, 1 << 20, seed)
    if not fallback:   # keep the strict program's input within budget, then put one line beyond it in the middle
        good = make_input("bracket", word, k - 1, 1 << 20, seed)
        data = good[: len(good) // 2] + b"QQQ" + edited(word, k + 1, random.Random(seed)).encode() + b"\n" + good[len(good) // 2:]
    for seg in (64, 4096, 0):
        got, want = both(b, data, segment_bytes=seg)
        assert got == want, (name, metric, mode, seg, got[:2] if isinstance(got, tuple) else len(got))
    if not fallback:
        assert isinstance(want, tuple), "the strict program must reject the over-budget line"
    # a slice through the FST simulator (independent of determinization, tables and engine)
    cut = data[:4096]
    cut = cut[: cut.rfind(b"\n") + 1]
    sim = simulate(src, tmp_path, cut, metric, mode)
    try:
        assert sim == oracle.run(b, cut)
    except oracle.OracleMatchError:
        assert sim is None


def test_large_input_at_default_segments():
    """64 MiB of lines through the bracket program, Levenshtein, correction: the default configuration."""
    name, src, word, k, _ = PROGRAMS[0]
    b = blob(src, "Levenshtein", "correction")
    data = make_input(name, word, k, 64 << 20, 11)
    got, want = both(b, data)
    assert got == want


@pytest.mark.parametrize("prog", PROGRAMS, ids=lambda p: p[0])
def test_produced_binary_in_small_windows(prog, tmp_path):
    """`kexc compile --metric Levenshtein --approxmode explicit … --out BIN` in a fresh process, streamed through kx_run_fd in
    windows far smaller than the input, so lines (and the error budgets they carry) cross windows."""
    name, src, word, k, fallback = prog
    f = tmp_path / (name + ".kex")
    f.write_text(src)
    exe = tmp_path / name
    r = subprocess.run([KEXC, "compile", "--quiet", "--metric", "Levenshtein", "--approxmode", "explicit", str(f), "--out", str(exe)],
                       stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr
    data = make_input(name, word, k if fallback else k - 1, 3 << 20, 5)
    b = blob(src, "Levenshtein", "explicit")
    want = oracle.run(b, data)
    for window in (4096, 65536):
        env = dict(os.environ, KX_WINDOW_BYTES=str(window))
        r = subprocess.run(["timeout", "-k", "10", "300", str(exe)], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and r.stdout == want, (name, window, r.returncode, r.stderr[-200:])
