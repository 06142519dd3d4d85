"""CPU: quote-aware record mode (kx_split_records_quoted / kx_run_records_fd_quoted, `BIN --records --quote[=Q]`) — the offsets
model against csv.reader, the example RFC 4180 program on the oracle, the ABI, the command line's quote spellings and refusals,
and the Python binding's argument checks.  Nothing here needs a device: every refusal is made before the engine library is loaded
or before a tensor reaches it."""
import csv
import ctypes
import io
import os
import re
import subprocess

import pytest

from kleenexlang_amd import build, host, program_path, workloads
from oracle import oracle

INC = os.path.join(build.ROOT, "include")
EXAMPLE = os.path.join(build.ROOT, "kleenexlang_amd", "examples", "csv_rfc4180.kex")
ISSUE_INPUT = b'a,"b,c",d\n"x\ny","he said ""hi""",\n1,2,3\n'


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "kxhip.h")).read(), flags=re.S)


def test_quoted_model_edge_cases():
    m = lambda d, sep=b"\n", quote=b'"', parity=0: host.split_records_model(d, sep, quote, parity)
    assert m(b"") == [0] and m(b"", parity=1) == [0]
    assert m(b'a"\n"b\nc') == [0, 6, 7]                     # a quoted separator
    assert m(b'"a""\nb"\n') == [0, 8]                      # "" inside a quoted field toggles twice: still quoted
    assert m(b'""\n""\n') == [0, 3, 6]                     # an empty quoted field
    assert m(b'"\n"\n') == [0, 4]                          # a quote as the first byte
    assert m(b'ab\n"') == [0, 3, 4]                        # ... and as the last: the tail is a record
    assert m(b'ab\n"cd\nef\n') == [0, 3, 10]               # an open quote at the end: the rest is one last record
    assert m(b'ab\n"cd\nef\n"') == [0, 3, 11]
    assert m(b'\n"\n', parity=1) == [0, 3]                 # parity 1: the first separator is inside quotes
    assert m(b'x\n', parity=1) == [0, 2]                   # (and a last separator inside quotes leaves a tail)
    assert m(b"a,'b,c',d", b",", b"'") == [0, 2, 8, 9]     # other separators and quotes
    assert m(b'a\0"\0"\0b', b"\0", b'"') == [0, 2, 6, 7]
    assert m(b"a\n\0\n\0\n", b"\n", b"\0") == [0, 2, 6]
    assert m(b"\n" * 5) == host.split_records_model(b"\n" * 5)
    assert m(b'"' * 6) == [0, 6]
    assert m(ISSUE_INPUT) == [0, 10, 34, 40] and len(host.split_records_model(ISSUE_INPUT)) - 1 == 4
    assert m(bytearray(b'x"\n"\n'), ord("\n"), ord('"')) == [0, 5]


def test_quoted_model_counts_the_rows_csv_reader_counts():
    for seed in range(4):
        data = workloads.generate("rfc4180", 400000, seed=seed)
        rows = list(csv.reader(io.StringIO(data.decode("ascii"), newline="")))
        offs = host.split_records_model(data, quote=b'"')
        assert len(offs) - 1 == len(rows)
        assert len(host.split_records_model(data)) - 1 > len(rows)   # (the generated rows do put newlines inside quotes)
        for i in range(0, len(rows), 97):                            # each record is one row
            assert list(csv.reader(io.StringIO(data[offs[i]:offs[i + 1]].decode("ascii"), newline=""))) == [rows[i]]
    assert data.count(b"\r\n") and data.count(b'""')


def test_generator_is_seeded_and_stays_off_the_program_table():
    assert workloads.generate("rfc4180", 50000, seed=3) == workloads.generate("rfc4180", 50000, seed=3)
    assert "rfc4180" not in workloads.PROGRAM_INPUT.values()
    assert not os.path.exists(os.path.join(host.PROGRAM_DIR, "csv_rfc4180.kex"))


def test_quoted_abi_is_declared_and_exported():
    txt = _header()
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    for name in ("kx_split_records_quoted", "kx_run_records_fd_quoted"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
    decl = re.search(r"int\s+kx_split_records_quoted\s*\(([^)]*)\)", txt).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["d_in", "n", "sep", "quote", "parity_in", "base", "d_off", "cap",
                                                                    "n_records", "parity_out", "stream"]


# ---------------------------------------------------------------------------------------------------------- the example on the oracle
@pytest.fixture(scope="module")
def csv_blob():
    return host.compile_file(EXAMPLE)


def _records(blob, data, quote):
    """(accepted outputs joined, rejected record numbers) of every record alone under the model."""
    offs = host.split_records_model(data, quote=quote)
    out, bad = [], []
    for i in range(len(offs) - 1):
        try:
            out.append(oracle.run(blob, data[offs[i]:offs[i + 1]]))
        except oracle.OracleMatchError:
            bad.append(i + 1)
    return b"".join(out), bad


def test_example_program_on_the_oracle(csv_blob):
    assert oracle.run(csv_blob, ISSUE_INPUT) == b'["a", "b,c", "d"]\n["x\\ny", "he said \\"hi\\"", ""]\n["1", "2", "3"]\n'
    with pytest.raises(oracle.OracleMatchError):
        oracle.run(csv_blob, b'a,b"c\n')
    assert _records(csv_blob, ISSUE_INPUT, None)[1] == [2, 3]
    data = workloads.generate("rfc4180", 300000, seed=11)
    whole = oracle.run(csv_blob, data)
    out, bad = _records(csv_blob, data, b'"')
    assert bad == [] and out == whole                       # quoted split: the whole stream's bytes, record by record
    out, bad = _records(csv_blob, data, None)
    assert len(bad) > 10                                    # line split: the rows with a quoted line break are cut and rejected


# ---------------------------------------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def flip_bin(tmp_path_factory):
    exe = tmp_path_factory.mktemp("recq") / "flip"
    r = subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("flip_ab"), "--out", str(exe)], timeout=300)
    assert r.returncode == 0
    return str(exe)


def _run(exe, *args):
    """The binary with an engine library that cannot load: an argument that passes parsing ends at the load."""
    return subprocess.run([exe, *args], input=b"ab\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                          env=dict(os.environ, KXHIP_LIB="/nonexistent/libkxhip.so"))


@pytest.mark.parametrize("args", [["--records", "--quote"], ["--quote", "--records"], ["--records", "--quote='"], ["--records", "--quote=\\x22"],
                                  ["--records=,", "--quote"], ["--records=\\t", "--quote=\\0"], ["--records", "--quote=\\t"],
                                  ["-t", "--records", "--quote=\\\\"], ["--records", "--quote=\\r"]])
def test_good_quote_spellings_reach_the_engine(flip_bin, args):
    r = _run(flip_bin, *args)
    assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("arg", ["", "ab", "\\q", "\\x", "\\x4", "\\xg0", "\\x100", "\\nn", '""', "\\N"])
def test_bad_quotes_are_refused_with_the_exact_message(flip_bin, arg):
    r = _run(flip_bin, "--records", "--quote=" + arg)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr == ("Invalid quote character: %s\n" % arg).encode()


def test_quote_refusals_before_loading(flip_bin):
    for args in (["--quote"], ["--quote=,"], ["-t", "--quote"]):
        r = _run(flip_bin, *args)
        assert r.returncode == 1 and r.stderr == (flip_bin + ": --quote needs --records\n").encode(), (args, r.stderr)
    for args in (["--records", "--quote=\\n"], ["--records=,", "--quote=,"], ["--records=\\x22", "--quote"], ["--quote=\\x0a", "--records"]):
        r = _run(flip_bin, *args)
        assert r.returncode == 1 and r.stderr == (flip_bin + ": the quote character cannot be the record separator\n").encode(), (args, r.stderr)
    r = _run(flip_bin, "--records", "--quote", "--gpus", "2")
    assert r.returncode == 1 and r.stderr.endswith(b": --records cannot be combined with --gpus\n")


def test_usage_mentions_quote(flip_bin):
    r = _run(flip_bin, "-h")
    assert r.returncode == 1 and b"--records[=SEP] --quote[=Q]" in r.stdout and b"--records[=SEP]\"" in r.stdout


# ---------------------------------------------------------------------------------------------------------- Python argument checks
def test_python_argument_errors_before_any_device():
    import torch
    m = host.split_records_model
    for bad, exc in ((b"", ValueError), (b"ab", ValueError), (256, ValueError), ('"', TypeError), (True, TypeError), (b"\n", ValueError),
                     (10, ValueError)):
        with pytest.raises(exc):
            m(b'a"\n', quote=bad)
    with pytest.raises(ValueError, match="record separator"):
        m(b"a,", sep=b",", quote=b",")
    for bad, exc in ((2, ValueError), (-1, ValueError), (True, TypeError), (None, TypeError), (0.0, TypeError)):
        with pytest.raises(exc):
            m(b'a"\n', quote=b'"', parity=bad)
    assert m(b"a\nb", parity=0) == m(b"a\nb")
    v = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        host.split_quoted_records_tensor(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        host.split_quoted_records_tensor(torch.zeros(8, dtype=torch.uint8)[::2])
    with pytest.raises(ValueError, match="record separator"):
        host.split_quoted_records_tensor(v, b"\n", b"\n")
    with pytest.raises(ValueError, match="parity"):
        host.split_quoted_records_tensor(v, parity=2)
    with pytest.raises(host.EngineError, match="HIP device"):
        host.split_quoted_records_tensor(v)
    prog = host.Program.__new__(host.Program)     # (no engine handle: anything that reached the device would fail differently)
    with pytest.raises(ValueError, match="record separator"):
        prog.run_records(b"a\n", quote=b"\n")
    with pytest.raises(ValueError, match="quote"):
        prog.run_records(b"a\n", quote=b"")
    with pytest.raises(TypeError, match="quote"):
        prog.run_records(b"a\n", quote='"')
    with pytest.raises(ValueError, match="record separator"):
        prog.run_records_fd(0, 1, sep=b",", quote=ord(","))
    with pytest.raises(ValueError, match="quote"):
        prog.run_records_fd(0, 1, quote=300)
