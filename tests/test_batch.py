"""CPU: the batched-run ABI (kx_run_batch, include/kxhip.h) and the Python binding's host-side checks — no device needed."""
import ctypes
import os
import re

import pytest

from kleenexlang_amd import build, host

INC = os.path.join(build.ROOT, "include")


def _header():
    return open(os.path.join(INC, "kxhip.h")).read()


def test_kx_run_batch_is_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+kx_run_batch\s*\(", txt)
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    assert hasattr(lib, "kx_run_batch")


def test_batch_structs_mirror_the_header():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, cls in (("kx_batch_doc", host.KxBatchDoc), ("kx_batch_stats", host.KxBatchStats)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
        fields = []
        for decl in re.findall(r"(?:uint32_t|uint64_t|float)\s+([^;]+);", body):
            fields += [f.strip().split("[")[0] for f in decl.split(",")]
        assert fields == [f[0] for f in cls._fields_], (name, fields)
    assert ctypes.sizeof(host.KxBatchDoc) == 16
    assert ctypes.sizeof(host.KxBatchStats) == 5 * 8 + 6 * 4 + 4 * 4


def test_kx_config_carries_batch_doc_max_without_changing_its_size():
    names = [f[0] for f in host.KxConfig._fields_]
    assert names[-2:] == ["batch_doc_max", "reserved"]
    assert ctypes.sizeof(host.KxConfig) == 112   # the size before the field: 4 + 17 + 4 u32, one u64, padded to 8 bytes
    assert host.KxConfig.batch_doc_max.offset + 4 == host.KxConfig.reserved.offset
    assert host.KxConfig.reserved.size == 12


def test_run_batch_refuses_malformed_input_before_touching_a_device():
    import torch
    prog = host.Program.__new__(host.Program)     # (no engine handle: anything that reached the device would fail differently)
    vals = torch.zeros(8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="non-decreasing"):
        prog.run_batch_tensor(vals, torch.tensor([0, 5, 3, 8], dtype=torch.int64))
    with pytest.raises(ValueError, match="outside"):
        prog.run_batch_tensor(vals, torch.tensor([0, 9], dtype=torch.int64))
    with pytest.raises(TypeError, match="int64"):
        prog.run_batch_tensor(vals, torch.tensor([0, 3], dtype=torch.int32))
    with pytest.raises(TypeError, match="uint8"):
        prog.run_batch_tensor(torch.zeros(8, dtype=torch.float32), torch.tensor([0, 3], dtype=torch.int64))
    with pytest.raises(TypeError, match="not bytes"):
        prog.run_batch([b"abc", "abc"])
    with pytest.raises(ValueError):
        host.check_batch_offsets([0, 2, 1], 4)
    host.check_batch_offsets([1, 1, 4], 4)
    assert host.pack_batch([b"ab", b"", bytearray(b"c")]) == (b"abc", [0, 2, 2, 3])


def test_run_batch_without_a_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from kleenexlang_amd import EngineError, Program, compile_file
    with pytest.raises(EngineError):
        Program(compile_file("flip_ab")).run_batch([b"ab\n"])
