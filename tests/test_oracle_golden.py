"""CPU: pin the oracle (and the compiler restatement behind it) to the reference's own vectors."""
import hashlib
import os

import pytest
from conftest import GOLDEN, blob_of, line_expected, line_input, same_modulo_trailing_newlines

from kleenexlang_amd import CompileError, workloads
from oracle import oracle


def _names(vectors, key):
    return [t["name"] for t in vectors[key]]


@pytest.mark.parametrize("opt", [0, 3])
@pytest.mark.parametrize("path_form", [False, True])
def test_reference_line_tests(vectors, opt, path_form):
    for t in vectors["line_tests"]:
        blob = blob_of(t["program"], opt)
        got = oracle.run(blob, line_input(t["in"]), path_form=path_form)
        assert same_modulo_trailing_newlines(got, line_expected(t["out"])), (t["name"], got)


@pytest.mark.parametrize("opt", [0, 3])
@pytest.mark.parametrize("path_form", [False, True])
def test_reference_exact_tests(vectors, opt, path_form):
    for t in vectors["exact_tests"]:
        blob = blob_of(t["program"], opt)
        for inp, out in t["cases"]:
            got = oracle.run(blob, inp.encode("utf-8"), path_form=path_form)
            assert got == out.encode("utf-8"), (t["name"], inp, got)


def test_programs_direct_mode_rejects_now_run_with_the_action_post_pass(vectors):
    """What `--act=false` refuses (Commands.hs:165-168) compiles by default: tests/test_register_actions.py holds the vectors."""
    for t in vectors["direct_mode_rejects"]:
        assert oracle.run(blob_of(t["program"]), "c\n".encode()) == "ø".encode()


def test_state_counts_match_literal_restatement(vectors):
    counts = vectors["state_counts"]
    for t in vectors["line_tests"]:
        if t["name"] in counts:
            assert oracle.info(blob_of(t["program"], 0))["nstates"] == counts[t["name"]], t["name"]
    # csv2json: 27 with the reference's regex-range desugaring (`/[0-9]{1,3}/` = one digit + THREE optional ones: `replicate n ie ++
    # replicate m' iquest`, Desugaring.hs:106-115), followed to the letter since round 4; SURVEY App. E's 23 was counted with the
    # standard m - n meaning (it says so) and is reproduced under KEXC_STANDARD_RANGES=1.
    for prog, n in [("apache_log", 306), ("iso_datetime_to_json", 36), ("csv2json", 27), ("thousand_sep", 6),
                    ("add_commas", 7), ("flip_ab", 2)]:
        assert oracle.info(blob_of(prog, 0))["nstates"] == n, prog
    from kleenexlang_amd import host, program_path
    os.environ["KEXC_STANDARD_RANGES"] = "1"
    try:
        assert oracle.info(host.compile_source(open(program_path("csv2json")).read(), opt=0))["nstates"] == 23
    finally:
        del os.environ["KEXC_STANDARD_RANGES"]


def test_regex_ranges_follow_the_references_desugaring():
    """`/x{n,m}/` inside a regex literal = n mandatory + m OPTIONAL copies in the reference (Desugaring.hs:106-115: `replicate n ie ++
    replicate m' iquest`) — unlike the Kleenex term `t{n,m}` (:150-160: m - n).  The reference's binary for csv2json therefore accepts
    a four-digit octet; so does this one (rounds 1-3 rejected it)."""
    from kleenexlang_amd import host
    rx = host.compile_source('main := /x{1,3}/ "!"\n')
    for k in (1, 2, 3, 4):
        assert oracle.run(rx, b"x" * k) == b"x" * k + b"!"
    for bad in (b"", b"xxxxx"):
        with pytest.raises(oracle.OracleMatchError):
            oracle.run(rx, bad)
    term = host.compile_source('main := x{1,3} "!"\nx := /x/\n')
    assert oracle.run(term, b"xxx") == b"xxx!"
    with pytest.raises(oracle.OracleMatchError):
        oracle.run(term, b"xxxx")
    row = b"1,a,b,c@d.e,f,1234.5.6.7\n"
    assert b'"1234.5.6.7"' in oracle.run(blob_of("csv2json"), row)


@pytest.mark.parametrize("opt", [0, 3])
@pytest.mark.parametrize("path_form", [False, True])
def test_reference_samples_match_perl_twins(expected, opt, path_form):
    for prog, e in expected["samples"].items():
        data = open(os.path.join(GOLDEN, e["input"]), "rb").read()
        assert hashlib.sha256(data).hexdigest() == e["input_digest"]["sha256"]
        got = oracle.run(blob_of(prog, opt), data, path_form=path_form)
        assert len(got) == e["expected"]["bytes"], prog
        assert hashlib.sha256(got).hexdigest() == e["expected"]["sha256"], prog


@pytest.mark.parametrize("path_form", [False, True])
def test_seeded_synthetic_match_perl_twins(expected, path_form):
    for e in expected["synthetic"]:
        data = workloads.generate(workloads.PROGRAM_INPUT[e["program"]], e["nbytes"], e["seed"])
        assert hashlib.sha256(data).hexdigest() == e["input_digest"]["sha256"], "generator drifted"
        got = oracle.run(blob_of(e["program"]), data, path_form=path_form)
        assert hashlib.sha256(got).hexdigest() == e["expected"]["sha256"], (e["program"], e["nbytes"])


def _commas(digits):
    s = digits.decode()
    head = len(s) % 3 or 3
    return (s[:head] + "".join("," + s[i:i + 3] for i in range(head, len(s), 3))).encode()


@pytest.mark.parametrize("opt", [0, 3])
def test_config1_add_commas_1mib(opt):
    """BASELINE config 1: 1 MiB random digits; MiB-sized registers in the register form."""
    blob = blob_of("add_commas", opt)
    d = workloads.digits(1 << 20, terminated=True)
    want = _commas(d[:-1]) + b"\n"
    assert len(want) == 1398102
    assert oracle.run(blob, d) == want
    assert oracle.run(blob, d, path_form=True) == want
    d2 = workloads.digits(1 << 20, terminated=False)   # the number never completes: identity
    assert oracle.run(blob, d2) == d2
    assert oracle.run(blob, d2, path_form=True) == d2


def test_match_error_position_and_flush_granularity():
    blob = blob_of("flip_ab")
    with pytest.raises(oracle.OracleMatchError) as e:
        oracle.run(blob, b"abxa\n")
    assert e.value.pos == 2 and e.value.partial == b"ba"
    with pytest.raises(oracle.OracleMatchError) as e:   # end of input in a non-final state
        oracle.run(blob_of("main := /ab/"), b"a")
    assert e.value.pos == 1


def test_reference_runtime_binary_agrees(expected, tmp_path):
    """oracle/_ref = reference-shaped generated C + the reference's own crt/crt.c (built where the
    reference tree exists); elsewhere the same generated C + the restated runtime oracle/crt_port/crt.c
    (`make port`).  It must agree with the restated interpreter byte for byte."""
    import subprocess
    from kleenexlang_amd import build, program_path

    def binary(program):
        exe = oracle.ref_binary(program, 3)
        if exe is None:
            exe = str(tmp_path / program)
            subprocess.check_call([os.path.join(build.OUT, "kexc"), "compile", "--quiet", "--opt", "3", "--backend=c", "--crt-dir",
                                   os.path.join(build.ROOT, "oracle", "crt_port"), program_path(program), "--out", exe])
        return exe
    e = expected["samples"]["apache_log"]
    data = open(os.path.join(GOLDEN, e["input"]), "rb").read()
    out = subprocess.run([binary("apache_log")], input=data, stdout=subprocess.PIPE, check=True).stdout
    assert hashlib.sha256(out).hexdigest() == e["expected"]["sha256"]
    r = subprocess.run([binary("flip_ab")], input=b"abxa\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and r.stderr == b"Match error at input symbol 2!\n" and r.stdout == b""
