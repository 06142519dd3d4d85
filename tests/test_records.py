"""CPU: record mode (kx_split_records / kx_run_records_fd, `BIN --records[=SEP]`) — the offsets model, the ABI, the command line's
separator spellings and refusals, and the Python binding's argument checks.  Nothing here needs a device: every refusal is made
before the engine library is loaded or before a tensor reaches it."""
import ctypes
import os
import re
import subprocess

import pytest

from kleenexlang_amd import build, host, program_path

INC = os.path.join(build.ROOT, "include")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "kxhip.h")).read(), flags=re.S)


def test_split_records_model_edge_cases():
    m = host.split_records_model
    assert m(b"") == [0]                                   # no records
    assert m(b"abc") == [0, 3]                             # no separator: the tail is the one record
    assert m(b"\n") == [0, 1]
    assert m(b"\n\n\n") == [0, 1, 2, 3]                    # only separators: empty-bodied records
    assert m(b"ab\ncd\n") == [0, 3, 6]                     # trailing separator
    assert m(b"ab\ncd") == [0, 3, 5]                       # none
    assert m(b"a\0b\0", b"\0") == [0, 2, 4] == m(b"a\0b\0", 0)
    assert m(b"\xff\xffx", b"\xff") == [0, 1, 2, 3]
    assert m(b"a\nb", b"\xff") == [0, 3]
    assert m(bytearray(b"x,y"), ord(",")) == [0, 2, 3]


def test_records_abi_is_declared_exported_and_mirrored():
    txt = _header()
    for name in ("kx_split_records", "kx_run_records_fd"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt)
        assert hasattr(ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so")), name)
    body = re.search(r"typedef struct kx_records_stats \{(.*?)\} kx_records_stats;", txt, flags=re.S).group(1)
    fields = []
    for decl in re.findall(r"(?:uint32_t|uint64_t|float)\s+([^;]+);", body):
        fields += [f.strip().split("[")[0] for f in decl.split(",")]
    assert fields == [f[0] for f in host.KxRecordsStats._fields_]
    assert ctypes.sizeof(host.KxRecordsStats) == 7 * 8 + 3 * 4 + 4 * 4 + 4   # (padded to 8 bytes)


@pytest.fixture(scope="module")
def flip_bin(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rec") / "flip"
    r = subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("flip_ab"), "--out", str(exe)], timeout=300)
    assert r.returncode == 0
    return str(exe)


def _run(exe, *args, lib="/nonexistent/libkxhip.so"):
    """The binary with an engine library that cannot load: an argument that passes parsing ends at the load, with its own
    message, so no GPU is touched either way."""
    return subprocess.run([exe, *args], input=b"ab\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                          env=dict(os.environ, KXHIP_LIB=lib))


@pytest.mark.parametrize("spelling", ["--records", "--records=\\n", "--records=\\t", "--records=\\r", "--records=\\0", "--records=\\\\",
                                      "--records=\\x00", "--records=\\xff", "--records=\\x2C", "--records=,", "--records=x", "--records=\\"])
def test_good_separator_spellings_reach_the_engine(flip_bin, spelling):
    r = _run(flip_bin, spelling)
    assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr, (spelling, r.stderr)
    r = _run(flip_bin, "-t", spelling)
    assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr


@pytest.mark.parametrize("arg", ["", "ab", "\\q", "\\x", "\\x4", "\\xg0", "\\x100", "\\nn", ",,", "\\N"])
def test_bad_separators_are_refused_with_the_exact_message(flip_bin, arg):
    r = _run(flip_bin, "--records=" + arg)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr == ("Invalid record separator: %s\n" % arg).encode()


def test_records_with_phase_or_gpus_is_refused_before_loading(flip_bin):
    for args in (["--records", "--phase", "1"], ["--phase=1", "--records=,"], ["--records", "--gpus", "2"], ["--gpus=1", "--records"]):
        r = _run(flip_bin, *args)
        assert r.returncode == 1, args
        assert re.fullmatch(rb".*: --records cannot be combined with --(phase|gpus)\n", r.stderr), (args, r.stderr)
        assert b"HIP engine" not in r.stderr


def test_usage_mentions_records(flip_bin):
    r = _run(flip_bin, "-h")
    assert r.returncode == 1 and b"Normal usage" in r.stdout and b"--records[=SEP]" in r.stdout


def test_python_argument_errors_before_any_device():
    import torch
    with pytest.raises(TypeError):
        host.split_records_model("abc")
    for bad, exc in ((b"", ValueError), (b"ab", ValueError), (256, ValueError), (-1, ValueError), ("\n", TypeError), (None, TypeError),
                     (True, TypeError), (1.0, TypeError)):
        with pytest.raises(exc):
            host.split_records_model(b"a\n", bad)
    with pytest.raises(TypeError, match="uint8"):
        host.split_records_tensor(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="1-D"):
        host.split_records_tensor(torch.zeros((2, 2), dtype=torch.uint8))
    with pytest.raises(TypeError, match="torch tensor"):
        host.split_records_tensor(b"abc")
    with pytest.raises(ValueError, match="contiguous"):
        host.split_records_tensor(torch.zeros(8, dtype=torch.uint8)[::2])
    with pytest.raises(ValueError, match="byte"):
        host.split_records_tensor(torch.zeros(4, dtype=torch.uint8), sep=b"ab")
    with pytest.raises(host.EngineError, match="HIP device"):
        host.split_records_tensor(torch.zeros(4, dtype=torch.uint8))
    prog = host.Program.__new__(host.Program)     # (no engine handle: anything that reached the device would fail differently)
    with pytest.raises(TypeError, match="bytes"):
        prog.run_records("a\nb\n")
    with pytest.raises(ValueError):
        prog.run_records(b"a\n", sep=b"")
    with pytest.raises(TypeError, match="in_fd"):
        prog.run_records_fd("0", 1)
    with pytest.raises(TypeError, match="report_fd"):
        prog.run_records_fd(0, 1, report_fd=None)
    with pytest.raises(ValueError):
        prog.run_records_fd(0, 1, sep=300)
