"""Approximate matching: `t<k>` terms under --metric / --approxmode / --ite (no GPU needed).

Checked three ways: the reference's own accept/reject verdicts (golden/approx_vectors.json), an independent brute-force model of
the three distances over small finite languages, and outputs derived by hand from the rewrite tables (golden/approx_derivation.md).
Every blob goes through kx_validate; the CPU oracle runs it."""
import itertools
import json
import os
import random
import subprocess

import pytest
from conftest import GOLDEN

from kleenexlang_amd import build, host, program_path
from kleenexlang_amd.host import CompileError
from oracle import oracle

KEXC = os.path.join(build.OUT, "kexc")
METRICS = ("LCS", "Hamming", "Levenshtein")
MODES = ("correction", "matching", "explicit")

with open(os.path.join(GOLDEN, "approx_vectors.json"), encoding="utf-8") as _f:
    VECTORS = json.load(_f)

_BLOBS = {}


def blob(src, metric="LCS", mode="correction", ite=False):
    key = (src, metric, mode, ite)
    if key not in _BLOBS:
        b = host.compile_flags(src, metric=metric, approx_mode=mode, ite=ite)
        host.validate_blob(b)
        _BLOBS[key] = b
    return _BLOBS[key]


def run(b, data):
    """Oracle output bytes, or None when the program rejects."""
    try:
        return oracle.run(b, data)
    except oracle.OracleMatchError:
        return None


def simulate(src, tmp_path, data, metric, mode, ite=False):
    """`kexc simulate --sim lockstep` (the FST simulator, independent of determinization and tables): bytes or None."""
    f = tmp_path / "p.kex"
    f.write_text(src)
    r = subprocess.run([KEXC, "simulate", "--sim", "lockstep", "--metric", metric, "--approxmode", mode, "--ite=%s" % str(ite).lower(),
                        str(f)], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode == 1 and r.stderr == b"Reject\n":
        return None
    assert r.returncode == 0, r.stderr
    return r.stdout


# ------------------------------------------------------------------ the reference's verdicts
@pytest.mark.parametrize("group", VECTORS["reference_verdicts"], ids=lambda g: g["name"])
def test_reference_verdicts(group, tmp_path):
    src, metric = group["program"], group["metric"]
    for data, accept, name in group["cases"]:
        data = data.encode()
        verdicts = []
        for mode in group["modes"]:
            via_oracle = run(blob(src, metric, mode), data)
            via_sim = simulate(src, tmp_path, data, metric, mode)
            assert via_oracle == via_sim, (name, mode, via_oracle, via_sim)
            verdicts.append(via_oracle is not None)
        assert verdicts == [accept] * len(verdicts), (name, verdicts)   # the modes agree, and with the reference


@pytest.mark.parametrize("case", VECTORS["hand_derived"], ids=lambda c: "case%d" % c["case"])
def test_hand_derived_outputs(case, tmp_path):
    b = blob(case["program"], case["metric"], case["mode"])
    assert run(b, case["in"].encode()) == case["out"].encode()
    assert simulate(case["program"], tmp_path, case["in"].encode(), case["metric"], case["mode"]) == case["out"].encode()


# ------------------------------------------------------------------ brute-force model
# (source of the approximated term, its finite language)
FINITE = [
    ("/ab/ | /cd/ /e/?", ["ab", "cd", "cde"]),
    ("/a/ /[bc]/ /d/", ["abd", "acd"]),
    ("/x/ | /xy/ | /yx/", ["x", "xy", "yx"]),
    ("/ab/ /c/{0,2}", ["ab", "abc", "abcc"]),
    ('"" | /a/ /b/?', ["", "a", "ab"]),
    ("/[ab]/ /[ab]/", ["aa", "ab", "ba", "bb"]),
]


def levenshtein(a, b, sub=True):
    d = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        prev, d[0] = d[0], i
        for j, cb in enumerate(b, 1):
            cur = min(d[j] + 1, d[j - 1] + 1, prev + (0 if ca == cb else (1 if sub else 2)))
            prev, d[j] = d[j], cur
    return d[len(b)]


def distance(metric, a, b):
    if metric == "Hamming":
        return sum(x != y for x, y in zip(a, b)) if len(a) == len(b) else 10 ** 9
    return levenshtein(a, b, sub=metric == "Levenshtein")   # LCS: insertions and deletions only (a substitution costs two)


def inputs(lang, k, seed):
    """Random strings of length 0-8 over the languages' letters, and words of the language with 0..k+1 random edits."""
    rng = random.Random(seed)
    alpha = "abcdexy"
    out = {"".join(rng.choice(alpha) for _ in range(rng.randint(0, 8))) for _ in range(60)}
    for _ in range(80):
        w = list(rng.choice(lang))
        for _ in range(rng.randint(0, k + 1)):
            op = rng.randrange(3)
            if op == 0 or not w:
                w.insert(rng.randint(0, len(w)), rng.choice(alpha))
            elif op == 1:
                del w[rng.randrange(len(w))]
            else:
                w[rng.randrange(len(w))] = rng.choice(alpha)
        out.add("".join(w)[:8])
    return sorted(out)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("idx", range(len(FINITE)))
def test_brute_force_model(metric, k, idx):
    term, lang = FINITE[idx]
    src = "main := (%s)<%d>\n" % (term, k)
    plain = blob("main := %s\n" % term)
    matching, correction, explicit = (blob(src, metric, m) for m in ("matching", "correction", "explicit"))
    for w in inputs(lang, k, seed=1000 * idx + 10 * k + METRICS.index(metric)):
        d = min(distance(metric, w, x) for x in lang)
        data = w.encode()
        m_out = run(matching, data)
        assert (m_out is not None) == (d <= k), (src, metric, w, d)
        if m_out is not None:
            assert m_out == data, (src, metric, w)   # matching mode copies the input
        c_out = run(correction, data)
        assert (c_out is not None) == (d <= k), (src, metric, w, d)
        if c_out is not None:
            # the correction is a word of the language (accepted, and copied, by the plain program) at the least distance: the start
            # sum tries the copies with fewer errors allowed first
            assert run(plain, c_out) == c_out, (src, metric, w, c_out)
            assert distance(metric, w, c_out.decode()) == d, (src, metric, w, c_out)
        assert (run(explicit, data) is not None) == (d <= k), (src, metric, w, d)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("mode", ["matching", "correction"])
def test_iterative_accepts_what_k_fold_accepts(metric, mode):
    """--ite (k rewrites of one error each) and the k-fold rewrite accept the same strings (the reference's KFoldApproximation.hs)."""
    for idx, (term, lang) in enumerate(FINITE[:4]):
        src = "main := (%s)<2>\n" % term
        kf, it = blob(src, metric, mode, False), blob(src, metric, mode, True)
        for w in inputs(lang, 2, seed=77 + idx):
            assert (run(kf, w.encode()) is None) == (run(it, w.encode()) is None), (src, metric, mode, w)


# ------------------------------------------------------------------ the rules
def test_suppressed_approximation_is_the_term_itself():
    for metric, mode in itertools.product(METRICS, MODES):
        assert blob('main := ~(/ab/<1>) "x" ~(/c/<2>)\n', metric, mode) == blob('main := ~(/ab/) "x" ~(/c/)\n', metric, mode)


def test_zero_errors_is_the_term_itself():
    for metric, mode in itertools.product(METRICS, MODES):
        a, b = blob("main := (/ab/ | /c/)<0> /d/\n", metric, mode), blob("main := (/ab/ | /c/) /d/\n")
        for w in ["abd", "cd", "ad", "abcd", "", "xd"]:
            assert run(a, w.encode()) == run(b, w.encode()), (metric, mode, w)


def test_nested_approximation_is_refused(tmp_path):
    src = "main := A<1>\nA := /a/<1> /b/\n"
    with pytest.raises(CompileError, match="Approximated sub-programs cannot contain approximation terms"):
        host.compile_flags(src, metric="Levenshtein")
    f = tmp_path / "n.kex"
    f.write_text(src)
    r = subprocess.run([KEXC, "compile", "--quiet", str(f), "--blob", str(tmp_path / "b")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and r.stderr == b"Approximated sub-programs cannot contain approximation terms\n"


def test_non_right_regular_approximation_is_a_compile_error():
    with pytest.raises(CompileError, match="not right-regular"):
        host.compile_flags("main := A<1>\nA := /a/ A /b/ | /c/\n")


def test_bad_flag_values_give_the_reference_messages(tmp_path):
    f = tmp_path / "p.kex"
    f.write_text("main := /a/<1>\n")
    for flag, val, msg in [("--metric", "lcs", b'"lcs" is not a valid approximation type\n'),
                           ("--approxmode", "Matching", b'"Matching" is not a valid approximation mode\n')]:
        for sub in (["compile", "--quiet"], ["simulate"]):
            r = subprocess.run([KEXC, *sub, flag, val, str(f)], input=b"a", stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert r.returncode == 1 and r.stderr == msg, (sub, r.stderr)
    with pytest.raises(CompileError, match='"Damerau" is not a valid approximation type'):
        host.compile_flags("main := /a/<1>\n", metric="Damerau")
    with pytest.raises(CompileError, match='"fuzzy" is not a valid approximation mode'):
        host.compile_flags("main := /a/<1>\n", approx_mode="fuzzy")


def test_programs_without_approximation_compile_byte_identically():
    srcs = [open(program_path(n)).read() for n in ("apache_log", "csv2json", "flip_ab", "thousand_sep", "add_commas")]
    for src in srcs:
        base = host.compile_flags(src)
        assert base == host.compile_source(src)
        for metric, mode, ite in itertools.product(METRICS, MODES, (False, True)):
            assert host.compile_flags(src, metric=metric, approx_mode=mode, ite=ite) == base, (metric, mode, ite)


def test_kexc_exports_the_approximation_entry_point():
    import ctypes
    import re
    txt = open(os.path.join(build.ROOT, "include", "kexc_approx.h")).read()
    names = set(re.findall(r"\b(kexc_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    assert names == {"kexc_compile_approx"}
    assert hasattr(ctypes.CDLL(os.path.join(build.OUT, "libkexc.so")), "kexc_compile_approx")


def test_cli_flags_reach_compile_and_every_simulator(tmp_path):
    """--metric / --approxmode / --ite reach `kexc compile` (the blob equals the C API's) and `kexc simulate` in all three forms."""
    src = "main := (/kleenex/<2> /\\n/)*\n"
    f = tmp_path / "p.kex"
    f.write_text(src)
    data = b"kleenex\nkleene\nklenex\nkleeenex\n"
    for metric, mode, ite in [("Levenshtein", "explicit", False), ("LCS", "correction", True), ("Hamming", "matching", False)]:
        flags = ["--metric", metric, "--approxmode", mode, "--ite=%s" % str(ite).lower()]
        out = tmp_path / "b.kxp"
        r = subprocess.run([KEXC, "compile", "--quiet", *flags, str(f), "--blob", str(out)], stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr
        b = host.compile_flags(src, name=str(f), metric=metric, approx_mode=mode, ite=ite)   # the blob's info names the source
        assert out.read_bytes() == b
        want = run(b, data)
        for sim in ("lockstep", "backtrack"):
            r = subprocess.run([KEXC, "simulate", "--sim", sim, *flags, str(f)], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert (r.stdout if r.returncode == 0 else None) == want, (metric, mode, sim, r.stderr)
