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


def test_abi_refusals_of_every_mode_before_any_device():
    """The argument rules of the four kx_split_records* and the four kx_run_records_fd* entry points of the modes: every bad
    argument is KX_E_ARG (-4) with null device pointers and a null program, so before anything touches a device.  That the rule
    made the refusal, not the null: the same call with good arguments is KX_E_CAPACITY (-3, the size query of an empty buffer)
    for a split, and for a run it leaves another message (the null program's)."""
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    lib.kx_last_error.restype = ctypes.c_char_p
    vp, u8, u32, u64, ci = ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    n, w = ctypes.c_uint64(), ctypes.c_uint32()
    nref, wref = ctypes.byref(n), ctypes.byref(w)
    lib.kx_split_records.argtypes = [vp, ctypes.c_size_t, u8, u64, vp, u64, vp, vp]
    lib.kx_split_records_quoted.argtypes = [vp, ctypes.c_size_t, u8, u8, u32, u64, vp, u64, vp, vp, vp]
    lib.kx_split_records_escaped.argtypes = [vp, ctypes.c_size_t, u8, ci, u8, u32, u64, vp, u64, vp, vp, vp]
    lib.kx_split_records_rs.argtypes = [vp, ctypes.c_size_t, ctypes.c_char_p, u32, ctypes.c_char_p, u32, u64, vp, u64, vp, vp, vp, vp, vp]
    split = {   # (d_in, n) = (null, 0) in front of `mid`; base, d_off, cap, n_records behind it; then the mode's outputs and the stream
        "byte": lambda mid, nr=nref, cap=0, size=0: lib.kx_split_records(None, size, *mid, 0, None, cap, nr, None),
        "quoted": lambda mid, nr=nref: lib.kx_split_records_quoted(None, 0, *mid, 0, None, 0, nr, wref, None),
        "escaped": lambda mid, nr=nref: lib.kx_split_records_escaped(None, 0, *mid, 0, None, 0, nr, wref, None),
        "rs": lambda mid, nr=nref: lib.kx_split_records_rs(None, 0, *mid, 0, None, 0, nr, None, None, None, None),
    }
    good = {"byte": (10,), "quoted": (10, 34, 0), "escaped": (10, 34, 92, 0), "rs": (b"\r\n", 2, b"\r", 1)}
    bad = {"byte": [],
           "quoted": [(10, 10, 0),                                  # quote == sep
                      (10, 34, 2)],                                 # parity_in 2
           "escaped": [(10, 10, 92, 0),                             # quote == sep
                       (10, -1, 10, 0), (10, 34, 10, 0),            # escape == sep
                       (10, 34, 34, 0),                             # quote == escape
                       (10, 256, 92, 0), (10, -2, 92, 0),           # quote no byte value, nor -1
                       (10, 34, 92, 4),                             # state_in 4
                       (10, -1, 92, 1), (10, -1, 92, 3)],           # bit 0 of state_in without a quote
           "rs": [(b"", 0, b"", 0), (b"123456789", 9, b"", 0),      # rs_len 0 and 9
                  (None, 2, b"", 0),
                  (b"\r\n", 2, b"\r\n", 2), (b"\r\n", 2, b"\r\n\r", 3), (b"\r\n", 2, None, 1)]}   # ctx_in_len == rs_len, and more
    for mode, f in split.items():
        assert f(good[mode]) == -3, mode
        assert f(good[mode], nr=None) == -4, mode                   # a null n_records
        for mid in bad[mode]:
            assert f(mid) == -4, (mode, mid)
    assert split["byte"]((10,), cap=1) == -4 and split["byte"]((10,), size=1) == -4   # a capacity without offsets, a size without input
    # the edges of the rules from inside: still accepted
    for mid in ((10, 34, 1), (10, 255, 0)):
        assert split["quoted"](mid) == -3, mid
    for mid in ((10, 34, 92, 3), (10, -1, 92, 2), (10, 255, 0, 0)):
        assert split["escaped"](mid) == -3, mid
    for mid in ((b"x", 1, b"", 0), (b"12345678", 8, b"1234567", 7)):
        assert split["rs"](mid) == -3, mid

    head, tail = [vp, ci, ci], [ci, vp]
    lib.kx_run_records_fd.argtypes = head + [u8] + tail
    lib.kx_run_records_fd_quoted.argtypes = head + [u8, u8] + tail
    lib.kx_run_records_fd_escaped.argtypes = head + [u8, ci, u8] + tail
    lib.kx_run_records_fd_rs.argtypes = head + [ctypes.c_char_p, u32] + tail
    run = {"byte": lib.kx_run_records_fd, "quoted": lib.kx_run_records_fd_quoted, "escaped": lib.kx_run_records_fd_escaped,
           "rs": lib.kx_run_records_fd_rs}
    good = {"byte": (10,), "quoted": (10, 34), "escaped": (10, 34, 92), "rs": (b"\r\n", 2)}
    bad = {"byte": [],
           "quoted": [(10, 10)],
           "escaped": [(10, 10, 92), (10, -1, 10), (10, 34, 10), (10, 34, 34), (10, 256, 92), (10, -2, 92)],
           "rs": [(b"", 0), (b"123456789", 9), (None, 2)]}
    for mode, g in run.items():
        assert g(None, 0, 1, *good[mode], -1, None) == -4, mode     # the null program
        null_program = lib.kx_last_error()
        for mid in bad[mode]:
            assert g(None, 0, 1, *mid, -1, None) == -4, (mode, mid)
            assert lib.kx_last_error() != null_program, (mode, mid)
