"""ctypes bindings over the two C ABIs (include/kexc_api.h, include/kxhip.h).

Python here is plumbing only: it loads the in-tree shared libraries, moves
pointers around and mirrors the error behaviour of the reference's produced
binaries (``Match error at input symbol N!``, exit code 1 — Backends/C.hs:79-81).
There is no CPU fallback: if ``libkxhip.so`` is missing or no HIP device is
present, constructing a :class:`Program` raises.
"""
import contextlib
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
BUILD_DIR = os.path.join(_HERE, "_build")
PROGRAM_DIR = os.path.join(_HERE, "programs")

KX_NKERNELS = 6
KERNEL_NAMES = ("sync", "forward", "head", "backlen", "resolve", "emit")
KX_MAX_LEAVES = 256
NOFAIL = 0xFFFFFFFFFFFFFFFF


class KleenexError(RuntimeError):
    pass


class CompileError(KleenexError):
    pass


class EngineError(KleenexError):
    pass


class MatchError(KleenexError):
    """The input is not in the program's language (reference: exit 1 + stderr message)."""

    def __init__(self, pos, stage=0, field=None):
        super().__init__("Match error at input symbol %d!" % pos)
        self.pos = pos
        self.stage = stage
        self.field = field      # field mode with a list: the number of the rejected field, `pos` counted inside it (keys=: its name)


class NoFieldError(KleenexError):
    """Field mode: the record has fewer fields than the one asked for.  `fields` = the fields it has."""

    def __init__(self, fields, field=None):
        super().__init__("the record has only %d field(s)" % fields if field is None else "the record has no field %r" % (field,))
        self.fields = fields
        self.field = field      # keys=: the first required name the record lacks (`fields` is then the mask of the names it has)


class HeaderError(KleenexError):
    """Record mode with header=: a name of the field list is no cell of header record N (`name`: its bytes), or the fields the
    names select have more than 8 ranges in their normal form (`name` is None)."""

    def __init__(self, name, message=None):
        super().__init__(message or "no cell of the header record is named %r" % (name,))
        self.name = name


class KxStats(ctypes.Structure):
    _fields_ = [("fail_pos", ctypes.c_uint64), ("fail_stage", ctypes.c_uint32),
                ("unsynced_segments", ctypes.c_uint32), ("in_bytes", ctypes.c_uint64),
                ("out_bytes", ctypes.c_uint64), ("kernel_ms", ctypes.c_float * KX_NKERNELS),
                ("total_ms", ctypes.c_float), ("emit_overflow_pieces", ctypes.c_uint32)]

    def as_dict(self):
        return {"unsynced_segments": self.unsynced_segments, "in_bytes": self.in_bytes,
                "out_bytes": self.out_bytes, "total_ms": self.total_ms,
                "emit_overflow_pieces": self.emit_overflow_pieces,
                "kernel_ms": {k: self.kernel_ms[i] for i, k in enumerate(KERNEL_NAMES)}}


class KxShardedResult(ctypes.Structure):
    _fields_ = [("out_len", ctypes.c_uint64), ("out_offset", ctypes.c_uint64), ("total_out", ctypes.c_uint64),
                ("boundary_ms", ctypes.c_float), ("stats", KxStats)]


ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)


class KxConfig(ctypes.Structure):
    """include/kxhip.h::kx_config (0 = default in every field)."""
    _fields_ = [("segment_bytes", ctypes.c_uint32), ("block_threads", ctypes.c_uint32),
                ("collect_timing", ctypes.c_uint32), ("phase", ctypes.c_uint32), ("window_bytes", ctypes.c_uint64)] + \
               [(k, ctypes.c_uint32) for k in ("delayed_form", "delay", "merge_window", "inline_consts", "job_stride", "disable", "force",
                                               "emit_waves", "emit_half", "emit_inplace", "emit_staging", "df_backoff", "debug_flags",
                                               "act_par_min", "act_prefix3_min", "act_lanes", "act_chunk", "batch_actions",
                                               "batch_doc_max")] + \
               [("reserved", ctypes.c_uint32 * 3)]


KX_OFF_DIRECT, KX_OFF_PAIR, KX_OFF_CMPX, KX_OFF_COOP, KX_OFF_SLOW = 1, 2, 4, 8, 16
KX_FORCE_BIG, KX_FORCE_TBLMODE, KX_FORCE_ACT_SEQ, KX_FORCE_SAME_DEVICE = 1, 2, 4, 8


def config_from_env(env=None, **fields):
    """The engine's switches are fields of kx_config; the library reads no environment variable for them.  Tests and profiling
    scripts keep using the variable names of earlier rounds: they are read HERE (and in kxrun.cpp for produced binaries) and mapped
    onto the struct.  `fields` override."""
    env = os.environ if env is None else env
    c = KxConfig()

    def tri(name):      # unset: auto, 0: off, anything else: on
        return 0 if name not in env else (2 if int(env[name]) else 1)

    def num(name):
        return int(env.get(name, "0") or 0)

    if "KX_DF" in env:
        v = int(env["KX_DF"])
        c.delayed_form = 1 if v == 0 else 2 if v == 2 else 0
    c.delay = num("KX_DF_K")
    if "KX_DF_J" in env:
        c.merge_window = int(env["KX_DF_J"]) + 1
    c.inline_consts = tri("KX_INL")
    c.job_stride = tri("KX_JL") if "KX_JL" in env else (1 if "KX_JL_AUTO_OFF" in env else 0)
    for name, bit in (("KX_NO_DIRECT", KX_OFF_DIRECT), ("KX_NO_PAIR", KX_OFF_PAIR), ("KX_NO_CMPX", KX_OFF_CMPX), ("KX_NO_COOP", KX_OFF_COOP),
                      ("KX_NO_SLOW", KX_OFF_SLOW)):
        if name in env:
            c.disable |= bit
    for name, bit in (("KX_FORCE_BIG", KX_FORCE_BIG), ("KX_FORCE_TBLMODE", KX_FORCE_TBLMODE), ("KX_ACT_SEQ", KX_FORCE_ACT_SEQ),
                      ("KX_SHARD_SAME_DEVICE", KX_FORCE_SAME_DEVICE)):
        if name in env:
            c.force |= bit
    c.emit_waves = num("KX_EMIT_WAVES")
    c.emit_half = tri("KX_EMIT_HALF")
    c.emit_inplace = tri("KX_EMIT_INPLACE")
    c.emit_staging = num("KX_EMIT_STG")
    c.df_backoff = 1 if num("KX_DF_BACKOFF_OFF") else 0
    c.debug_flags = num("KX_DEBUG_FLAGS")
    c.act_par_min = num("KX_ACT_PAR_MIN")
    c.act_prefix3_min = num("KX_ACT_PREFIX3_MIN")
    c.act_lanes = tri("KX_ACT_LANES")
    c.act_chunk = num("KX_ACT_CHUNK")
    c.batch_actions = tri("KX_BATCH_ACTIONS")     # (0: every document of an action stage takes the route; else the batch replay)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


class KxBatchDoc(ctypes.Structure):
    """include/kxhip.h::kx_batch_doc — one document's result of kx_run_batch."""
    _fields_ = [("fail_pos", ctypes.c_uint64), ("status", ctypes.c_uint32), ("fail_stage", ctypes.c_uint32)]


class KxBatchStats(ctypes.Structure):
    """include/kxhip.h::kx_batch_stats."""
    _fields_ = [(k, ctypes.c_uint64) for k in ("docs", "docs_rejected", "docs_routed", "in_bytes", "out_bytes")] + \
               [(k, ctypes.c_float) for k in ("forward_ms", "back_ms", "scan_ms", "emit_ms", "routed_ms", "total_ms")] + \
               [("docs_replayed", ctypes.c_uint64), ("actions_ms", ctypes.c_float), ("reserved", ctypes.c_uint32 * 1)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


def _check_batch_args(values, offsets):
    """What run_batch_tensor can refuse without a device: types, dtypes, shapes, and — for offsets held on the host — their
    order and range.  Raises TypeError / ValueError."""
    import torch
    if not isinstance(values, torch.Tensor) or not isinstance(offsets, torch.Tensor):
        raise TypeError("run_batch_tensor: values and offsets must be torch tensors")
    if values.dtype != torch.uint8 or values.dim() != 1:
        raise TypeError("run_batch_tensor: values must be a 1-D uint8 tensor (got %s, %d-D)" % (values.dtype, values.dim()))
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1:
        raise TypeError("run_batch_tensor: offsets must be a 1-D int64 tensor of n_docs + 1 entries")
    if values.numel() and values.stride(0) != 1:
        raise ValueError("run_batch_tensor: values must be contiguous")
    if not offsets.is_cuda:
        check_batch_offsets(offsets.numpy(), values.numel())


def check_batch_offsets(offsets, nvalues):
    """Host-side check of a batch's offsets: non-decreasing, inside [0, nvalues].  Raises ValueError."""
    import numpy as np
    o = np.asarray(offsets, dtype=np.int64)
    if o.ndim != 1 or o.size < 1:
        raise ValueError("batch offsets: a 1-D array of n_docs + 1 entries")
    if o.size > 1 and bool(np.any(o[1:] < o[:-1])):
        raise ValueError("batch offsets: not non-decreasing (document %d)" % int(np.argmax(o[1:] < o[:-1])))
    if int(o[0]) < 0 or int(o[-1]) > nvalues:
        raise ValueError("batch offsets: outside the values buffer [0, %d]" % nvalues)


def pack_batch(docs):
    """A list of bytes-like documents → (values bytes, offsets list).  Raises TypeError for anything else."""
    offs, total = [0], 0
    parts = []
    for i, d in enumerate(docs):
        if not isinstance(d, (bytes, bytearray, memoryview)):
            raise TypeError("run_batch: document %d is %s, not bytes" % (i, type(d).__name__))
        b = bytes(d)
        parts.append(b)
        total += len(b)
        offs.append(total)
    return b"".join(parts), offs


class KxRecordsStats(ctypes.Structure):
    """include/kxhip.h::kx_records_stats."""
    _fields_ = [(k, ctypes.c_uint64) for k in ("records", "records_rejected", "records_routed", "in_bytes", "out_bytes", "windows",
                                               "longest_record")] + \
               [(k, ctypes.c_float) for k in ("split_ms", "batch_ms", "total_ms")] + \
               [("reserved", ctypes.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


def _one_byte(v, what):
    """One byte, as bytes of length 1 or an int in [0, 255] → the int.  Raises TypeError / ValueError naming `what`."""
    if isinstance(v, bool) or not isinstance(v, (bytes, bytearray, int)):
        raise TypeError("%s: one byte (bytes of length 1 or an int), not %s" % (what, type(v).__name__))
    if isinstance(v, int):
        if not 0 <= v <= 255:
            raise ValueError("%s: %d is not a byte value" % (what, v))
        return v
    if len(v) != 1:
        raise ValueError("%s: one byte, not %d" % (what, len(v)))
    return v[0]


def _check_sep(sep):
    """A record separator: one byte, as bytes of length 1 or an int in [0, 255] → the int.  Raises TypeError / ValueError."""
    return _one_byte(sep, "record separator")


def _check_quote(quote, sep):
    """A quote character for the separator `sep`: one byte as _check_sep takes it, not the separator → the int."""
    q = _one_byte(quote, "quote character")
    if q == _check_sep(sep):
        raise ValueError("quote character: %r is also the record separator" % bytes([q]))
    return q


def _check_parity(parity):
    if isinstance(parity, bool) or not isinstance(parity, int):
        raise TypeError("parity: 0 or 1, not %s" % type(parity).__name__)
    if parity not in (0, 1):
        raise ValueError("parity: 0 or 1, not %d" % parity)
    return parity


def split_records_model(data, sep=b"\n", quote=None, parity=0):
    """kx_split_records in pure Python: the n_records + 1 offsets of the records of `data`, each ending after a separator byte
    (a non-empty tail is a last record; empty data has none: [0]).

    With a `quote` byte (kx_split_records_quoted) a separator ends a record only outside quotes: where the parity of the quote
    bytes before it, counted from `parity` at data[0], is even.  A doubled quote toggles twice, so RFC 4180 needs no escape rule;
    the parity after the data is parity ^ (data.count(quote) & 1)."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError("split_records_model: data must be bytes, not %s" % type(data).__name__)
    s = _check_sep(sep)
    _check_parity(parity)
    data = bytes(data)
    if quote is None:
        offs, i = [0], data.find(bytes([s]))
        while i >= 0:
            offs.append(i + 1)
            i = data.find(bytes([s]), i + 1)
    else:
        import re
        q = _check_quote(quote, sep)
        offs, p = [0], parity
        for m in re.finditer(b"[" + re.escape(bytes([q])) + re.escape(bytes([s])) + b"]", data):   # (only quotes and separators)
            if data[m.start()] == q:
                p ^= 1
            elif p == 0:
                offs.append(m.start() + 1)
    if offs[-1] != len(data):
        offs.append(len(data))
    return offs


def _check_escape(escape, sep, quote=None):
    """An escape character for the separator `sep` and the quote byte `quote` (None: none): one byte as _check_sep takes it, neither
    the separator nor the quote → the int."""
    e = _one_byte(escape, "escape character")
    if e == _check_sep(sep):
        raise ValueError("escape character: %r is also the record separator" % bytes([e]))
    if quote is not None and e == _check_quote(quote, sep):
        raise ValueError("escape character: %r is also the quote character" % bytes([e]))
    return e


def _check_state(state, quote):
    """The state at a buffer's first byte of an escaped split: bit 0 the quote parity (only with a quote), bit 1 escaped."""
    if isinstance(state, bool) or not isinstance(state, int):
        raise TypeError("state: an int in 0-3, not %s" % type(state).__name__)
    if not 0 <= state <= 3:
        raise ValueError("state: 0-3, not %d" % state)
    if quote is None and state & 1:
        raise ValueError("state: bit 0 (the quote parity) needs a quote character")
    return state


def split_escaped_records_model(data, sep=b"\n", quote=None, escape=b"\\", state=0):
    """kx_split_records_escaped in pure Python: (offsets, state_out).  An unescaped `escape` byte escapes the next byte; an
    escaped byte is only data (never a separator, a quote or an escape).  With a `quote` byte a separator ends a record only at
    even parity of the unescaped quotes before it.  state bit 0: the quote parity at data[0] (0 without a quote); bit 1: data[0]
    is escaped.  state_out is the state after the last byte; a non-empty tail is a last record, as in split_records_model."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError("split_escaped_records_model: data must be bytes, not %s" % type(data).__name__)
    s = _check_sep(sep)
    q = None if quote is None else _check_quote(quote, sep)
    e = _check_escape(escape, sep, quote)
    _check_state(state, quote)
    data = bytes(data)
    import re
    special = bytes([s, e]) if q is None else bytes([s, e, q])
    p, x, offs, last = state & 1, state >> 1, [0], -1
    for m in re.finditer(b"[" + b"".join(re.escape(bytes([c])) for c in special) + b"]", data):   # (only these bytes matter)
        i, b = m.start(), data[m.start()]
        if x and i != last + 1:
            x = 0                           # (the escaped byte was some other byte)
        last = i
        if x:
            x = 0                           # an escaped byte is only data
        elif b == e:
            x = 1
        elif b == q:
            p ^= 1
        elif p == 0:
            offs.append(i + 1)
    if x and last != len(data) - 1:
        x = 0
    if offs[-1] != len(data):
        offs.append(len(data))
    return offs, p | x << 1


def _check_rs(rs):
    """A multi-byte record separator: bytes of length 1 to 8 → bytes.  Raises TypeError / ValueError."""
    if not isinstance(rs, (bytes, bytearray)):
        raise TypeError("record separator string: bytes of length 1 to 8, not %s" % type(rs).__name__)
    if not 1 <= len(rs) <= 8:
        raise ValueError("record separator string: 1 to 8 bytes, not %d" % len(rs))
    return bytes(rs)


def _check_ctx(ctx, rs):
    if not isinstance(ctx, (bytes, bytearray)):
        raise TypeError("context: bytes shorter than the separator, not %s" % type(ctx).__name__)
    if len(ctx) >= len(rs):
        raise ValueError("context: %d bytes, not shorter than the separator (%d)" % (len(ctx), len(rs)))
    return bytes(ctx)


def split_rs_records_model(data, rs, ctx=b""):
    """kx_split_records_rs in pure Python: (offsets, ctx_out, tail_len).  Records end after the leftmost, non-overlapping copies
    of `rs` (1 to 8 bytes), found left to right as bytes.find finds them: the boundaries of data.split(rs).  `ctx` is the last
    min(len(rs) - 1, length of the unfinished record so far) bytes before data, all of the unfinished record, so that a separator
    may straddle two buffers; ctx_out is the context for the buffer that follows, tail_len the bytes of data behind its last
    selected separator (the last record is complete iff it is 0).  A non-empty tail is a last record, as in split_records_model."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError("split_rs_records_model: data must be bytes, not %s" % type(data).__name__)
    rs = _check_rs(rs)
    ctx = _check_ctx(ctx, rs)
    data = bytes(data)
    m, k, buf = len(rs), len(ctx), ctx + data
    offs, pos = [0], 0
    while True:
        j = buf.find(rs, pos)
        if j < 0:
            break
        pos = j + m                                  # always > k: ctx is shorter than rs
        offs.append(pos - k)
    tail_len = len(data) - max(pos - k, 0)           # bytes of this buffer behind its last selected separator
    if offs[-1] != len(data):
        offs.append(len(data))
    t = buf[pos:]
    return offs, t[len(t) - min(m - 1, len(t)):], tail_len


def _check_ors(ors):
    """An output record separator: bytes of length 0 to 8 → bytes.  Raises TypeError / ValueError."""
    if not isinstance(ors, (bytes, bytearray)):
        raise TypeError("output record separator: bytes of length 0 to 8, not %s" % type(ors).__name__)
    if len(ors) > 8:
        raise ValueError("output record separator: 0 to 8 bytes, not %d" % len(ors))
    return bytes(ors)


def _check_chomp(chomp):
    if not isinstance(chomp, bool):
        raise TypeError("chomp: True or False, not %s" % type(chomp).__name__)
    return chomp


def _check_trim(trim):
    """The trim of a framed batch: an int in [0, 2^32) → the int."""
    if isinstance(trim, bool) or not isinstance(trim, int):
        raise TypeError("trim: a non-negative int, not %s" % type(trim).__name__)
    if not 0 <= trim < 1 << 32:
        raise ValueError("trim: %d is not in [0, 2^32)" % trim)
    return trim


def chomp_records_model(data, offsets, trim, tail):
    """kx_run_batch_framed's documents in pure Python — the normative model of `--chomp`: record i of `data` is
    data[offsets[i]:offsets[i+1]] (a split model's offsets), and the document run for it is that range without its last `trim`
    bytes (the separator: 1 byte, or len(rs)).  With `tail` the last record is the stream's tail — it has no valid separator,
    whatever byte it ends in — and is run whole.  A record that is only its separator is the empty document.  Returns the list of
    the documents' bytes.  Raises ValueError for a range shorter than `trim` (the engine's KX_E_ARG)."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError("chomp_records_model: data must be bytes, not %s" % type(data).__name__)
    trim = _check_trim(trim)
    if not isinstance(tail, bool):
        raise TypeError("chomp_records_model: tail must be True or False, not %s" % type(tail).__name__)
    data, offs = bytes(data), [int(o) for o in offsets]
    check_batch_offsets(offs, len(data))
    n, docs = len(offs) - 1, []
    for i in range(n):
        t = 0 if tail and i == n - 1 else trim
        if offs[i + 1] - offs[i] < t:
            raise ValueError("chomp_records_model: record %d is shorter than the trim (%d)" % (i, t))
        docs.append(data[offs[i]:offs[i + 1] - t])
    return docs


class KxBatchFrame(ctypes.Structure):
    """include/kxhip.h::kx_batch_frame."""
    _fields_ = [("trim", ctypes.c_uint32), ("last_whole", ctypes.c_uint32), ("suffix_len", ctypes.c_uint32),
                ("suffix", ctypes.c_uint8 * 8), ("reserved", ctypes.c_uint32 * 3)]


KX_RECORDS_BYTE, KX_RECORDS_QUOTED, KX_RECORDS_ESCAPED, KX_RECORDS_RS = 0, 1, 2, 3


class KxRecordsOpts(ctypes.Structure):
    """include/kxhip.h::kx_records_opts."""
    _fields_ = [("size", ctypes.c_uint32), ("mode", ctypes.c_uint32), ("sep", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 3),
                ("quote", ctypes.c_int32), ("escape", ctypes.c_int32), ("rs", ctypes.c_uint8 * 8), ("rs_len", ctypes.c_uint32),
                ("chomp", ctypes.c_uint32), ("ors", ctypes.c_uint8 * 8), ("ors_len", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 4)]


class KxBatchFields(ctypes.Structure):
    """include/kxhip.h::kx_batch_fields."""
    _fields_ = [("size", ctypes.c_uint32), ("field", ctypes.c_uint32), ("fs", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 3),
                ("quote", ctypes.c_int32), ("escape", ctypes.c_int32), ("sep_len", ctypes.c_uint32), ("last_whole", ctypes.c_uint32),
                ("keep_sep", ctypes.c_uint32), ("suffix_len", ctypes.c_uint32), ("suffix", ctypes.c_uint8 * 8),
                ("reserved", ctypes.c_uint32 * 4)]


class KxFieldRange(ctypes.Structure):
    """include/kxhip.h::kx_field_range (hi = 0: open)."""
    _fields_ = [("lo", ctypes.c_uint32), ("hi", ctypes.c_uint32)]


class KxBatchFieldList(ctypes.Structure):
    """include/kxhip.h::kx_batch_field_list."""
    _fields_ = [("size", ctypes.c_uint32), ("n_ranges", ctypes.c_uint32), ("ranges", KxFieldRange * 8), ("fs", ctypes.c_uint8),
                ("pad", ctypes.c_uint8 * 3), ("quote", ctypes.c_int32), ("escape", ctypes.c_int32), ("sep_len", ctypes.c_uint32),
                ("last_whole", ctypes.c_uint32), ("keep_sep", ctypes.c_uint32), ("suffix_len", ctypes.c_uint32),
                ("suffix", ctypes.c_uint8 * 8), ("reserved", ctypes.c_uint32 * 4)]


def _field_range_array(ranges):
    """A normal form → (KxFieldRange * 8, n_ranges)."""
    a = (KxFieldRange * 8)()
    for j, (lo, hi) in enumerate(ranges):
        a[j].lo, a[j].hi = lo, hi or 0
    return a, len(ranges)


class KxFieldsKernelStats(ctypes.Structure):
    """include/kxhip.h::kx_fields_kernel_stats."""
    _fields_ = [(k, ctypes.c_float) for k in ("locate_ms", "gather_ms", "scan_ms", "splice_ms")] + [("calls", ctypes.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _check_field(field):
    """A field number: an int in [1, 2^32) → the int."""
    if isinstance(field, bool) or not isinstance(field, int):
        raise TypeError("field: an int from 1, not %s" % type(field).__name__)
    if not 1 <= field < 1 << 32:
        raise ValueError("field: %d is not in [1, 2^32)" % field)
    return field


def _check_fs(fs, quote=None, escape=None, sep=None):
    """A field separator: one byte, not the quote, the escape or the (one-byte) record separator `sep` → the int."""
    f = _one_byte(fs, "field separator")
    if sep is not None and f == _one_byte(sep, "record separator"):
        raise ValueError("field separator: %r is also the record separator" % bytes([f]))
    if quote is not None and f == _one_byte(quote, "quote character"):
        raise ValueError("field separator: %r is also the quote character" % bytes([f]))
    if escape is not None and f == _one_byte(escape, "escape character"):
        raise ValueError("field separator: %r is also the escape character" % bytes([f]))
    return f


def _check_sep_len(sep_len):
    if isinstance(sep_len, bool) or not isinstance(sep_len, int):
        raise TypeError("sep_len: an int from 0 to 8, not %s" % type(sep_len).__name__)
    if not 0 <= sep_len <= 8:
        raise ValueError("sep_len: %d is not in [0, 8]" % sep_len)
    return sep_len


def field_records_model(data, offsets, sep_len, last_whole, field, fs, quote=None, escape=None):
    """kx_run_batch_fields's view of its records in pure Python — the normative model of `--field`: record i of `data` is
    data[offsets[i]:offsets[i+1]]; its body is that range without its last `sep_len` bytes (the separator), the last record whole
    with `last_whole`.  The body's fields lie between its live `fs` bytes: every one; with a `quote` byte one at even parity of
    the quote bytes before it in the record; with an `escape` byte one that is unescaped and at even parity of the record's
    unescaped quotes (an escaped byte is only data).  A body with f live separators has f + 1 fields, the empty body one empty
    field.  Returns, per record, (prefix, field, rest, separator) — body = prefix + field + rest, field number `field` from 1 — or
    the number of fields the record has if that is fewer.  Raises ValueError for a range shorter than `sep_len`."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError("field_records_model: data must be bytes, not %s" % type(data).__name__)
    sep_len, field = _check_sep_len(sep_len), _check_field(field)
    if not isinstance(last_whole, bool):
        raise TypeError("field_records_model: last_whole must be True or False, not %s" % type(last_whole).__name__)
    f = _check_fs(fs, quote, escape)
    q = None if quote is None else _one_byte(quote, "quote character")
    e = None if escape is None else _one_byte(escape, "escape character")
    if q is not None and q == e:
        raise ValueError("escape character: %r is also the quote character" % bytes([e]))
    data, offs = bytes(data), [int(o) for o in offsets]
    check_batch_offsets(offs, len(data))
    n, res = len(offs) - 1, []
    for i in range(n):
        t = 0 if last_whole and i == n - 1 else sep_len
        if offs[i + 1] - offs[i] < t:
            raise ValueError("field_records_model: record %d is shorter than its separator (%d)" % (i, t))
        body, sep = data[offs[i]:offs[i + 1] - t], data[offs[i + 1] - t:offs[i + 1]]
        cuts, parity, esc = [], 0, False                      # the positions of the live separators
        for k, b in enumerate(body):
            if esc:
                esc = False
            elif e is not None and b == e:
                esc = True
            elif q is not None and b == q:
                parity ^= 1
            elif b == f and parity == 0:
                cuts.append(k)
                if len(cuts) == field:
                    break
        if len(cuts) < field - 1:
            res.append(len(cuts) + 1)
            continue
        lo = cuts[field - 2] + 1 if field > 1 else 0
        hi = cuts[field - 1] if len(cuts) >= field else len(body)
        res.append((body[:lo], body[lo:hi], body[hi:], sep))
    return res


FIELD_RANGES_MAX = 8


def _normal_field_ranges(items, what):
    """(lo, hi) pairs with hi None for an open range, each checked already → their normal form: the selected set as sorted,
    disjoint, not adjacent ranges, a tuple of at most 8 pairs."""
    top = 1 << 32                                               # (an open range's end: above every field number)
    norm = []
    for lo, hi in sorted((lo, top if hi is None else hi) for lo, hi in items):
        if norm and lo <= norm[-1][1] + 1:
            norm[-1][1] = max(norm[-1][1], hi)
        else:
            norm.append([lo, hi])
    if len(norm) > FIELD_RANGES_MAX:
        raise ValueError("%s: %d ranges in the normal form of the field list, at most %d" % (what, len(norm), FIELD_RANGES_MAX))
    return tuple((lo, None if hi == top else hi) for lo, hi in norm)


def parse_field_list(text):
    """The LIST of `--field=LIST` → its normal form, a tuple of (lo, hi) pairs with hi None for an open range.  LIST is one or
    more items joined by commas; an item is K, A-B (A <= B) or A- (A and every field behind it); a number has 1 to 10 decimal
    digits and a value from 1 to 4294967295.  Items may come in any order and overlap: "3,2" → ((2, 3),), "4-,2,6" →
    ((2, 2), (4, None)).  Raises ValueError for what the command line refuses: anything else, and a normal form of more than 8
    ranges."""
    if not isinstance(text, str):
        raise TypeError("field list: a str such as '2,5-7,9-', not %s" % type(text).__name__)

    def number(t):
        if not (1 <= len(t) <= 10 and t.isascii() and t.isdigit() and 1 <= int(t) < 1 << 32):
            raise ValueError("field list %r: %r is not a number from 1 to 4294967295" % (text, t))
        return int(t)

    items = []
    for item in text.split(","):
        a, dash, b = item.partition("-")
        lo = number(a)
        hi = lo if not dash else None if not b else number(b)
        if hi is not None and hi < lo:
            raise ValueError("field list %r: the range %s needs A <= B" % (text, item))
        items.append((lo, hi))
    return _normal_field_ranges(items, "field list %r" % text)


def _check_field_ranges(fields):
    """The `fields=` of record mode: a parse_field_list result, or a sequence of field numbers and (lo, hi) pairs (hi None: open)
    → the normal form."""
    if isinstance(fields, (str, bytes, bytearray)) or not isinstance(fields, (tuple, list)):
        raise TypeError("fields: a parse_field_list result or a sequence of ints and (lo, hi) pairs, not %s" % type(fields).__name__)
    if not fields:
        raise ValueError("fields: an empty list selects nothing")
    items = []
    for it in fields:
        if isinstance(it, (tuple, list)):
            if len(it) != 2:
                raise ValueError("fields: a range is a (lo, hi) pair, not %r" % (it,))
            lo, hi = _check_field(it[0]), None if it[1] is None else _check_field(it[1])
            if hi is not None and hi < lo:
                raise ValueError("fields: the range %r needs lo <= hi" % (it,))
        else:
            lo = hi = _check_field(it)
        items.append((lo, hi))
    return _normal_field_ranges(items, "fields")


def field_list_need(ranges):
    """The largest field number a normal form names explicitly: a record with fewer fields runs nothing."""
    lo, hi = ranges[-1]
    return lo if hi is None else hi


def field_list_missing(ranges, nfields):
    """K of "Record R has no field K!": the smallest member of the list above the `nfields` fields a record has."""
    for lo, hi in ranges:
        if hi is None or hi > nfields:
            return max(lo, nfields + 1)
    raise ValueError("the list names no field above %d" % nfields)


def field_list_records_model(data, offsets, sep_len, last_whole, ranges, fs, quote=None, escape=None):
    """kx_run_batch_field_list's view of its records in pure Python — the normative model of `--field=LIST`.  The records, their
    bodies, the live `fs` bytes and the field numbering are field_records_model's; `ranges` is the list (what `fields=` takes).  A
    record with at least field_list_need(ranges) fields gives (gaps, fields, separator): with m selected fields, `fields` is m
    pairs (K, bytes) in field order and `gaps` the m + 1 byte strings around them, so that the body is gaps[0] + fields[0][1] +
    gaps[1] + … + gaps[m].  A record with fewer fields gives the number of fields it has."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError("field_list_records_model: data must be bytes, not %s" % type(data).__name__)
    sep_len, ranges = _check_sep_len(sep_len), _check_field_ranges(ranges)
    if not isinstance(last_whole, bool):
        raise TypeError("field_list_records_model: last_whole must be True or False, not %s" % type(last_whole).__name__)
    f = _check_fs(fs, quote, escape)
    q = None if quote is None else _one_byte(quote, "quote character")
    e = None if escape is None else _one_byte(escape, "escape character")
    if q is not None and q == e:
        raise ValueError("escape character: %r is also the quote character" % bytes([e]))
    data, offs = bytes(data), [int(o) for o in offsets]
    check_batch_offsets(offs, len(data))
    need = field_list_need(ranges)
    n, res = len(offs) - 1, []
    for i in range(n):
        t = 0 if last_whole and i == n - 1 else sep_len
        if offs[i + 1] - offs[i] < t:
            raise ValueError("field_list_records_model: record %d is shorter than its separator (%d)" % (i, t))
        body, sep = data[offs[i]:offs[i + 1] - t], data[offs[i + 1] - t:offs[i + 1]]
        cuts, parity, esc = [], 0, False                      # the positions of the live separators
        for k, b in enumerate(body):
            if esc:
                esc = False
            elif e is not None and b == e:
                esc = True
            elif q is not None and b == q:
                parity ^= 1
            elif b == f and parity == 0:
                cuts.append(k)
        nf = len(cuts) + 1
        if nf < need:
            res.append(nf)
            continue
        begin, end = [0] + [c + 1 for c in cuts], cuts + [len(body)]
        gaps, fields, at = [], [], 0
        for lo, hi in ranges:
            for K in range(lo, (nf if hi is None else hi) + 1):
                gaps.append(body[at:begin[K - 1]])
                fields.append((K, body[begin[K - 1]:end[K - 1]]))
                at = end[K - 1]
        gaps.append(body[at:])
        res.append((gaps, fields, sep))
    return res


BLANKS = b" \t"                                                 # the blanks of `--blanks`: 0x20 and 0x09


def _check_not_blank(quote=None, escape=None, sep=None, special=b""):
    """The bytes of a `blanks=` call that cannot be a blank: the quote, the escape, the one-byte record separator `sep` and the
    special bytes."""
    for what, v in (("quote character", quote), ("escape character", escape), ("record separator", sep)):
        if v is not None and _one_byte(v, what) in BLANKS:
            raise ValueError("%s: %r is a blank, which blanks= makes a field separator" % (what, bytes([_one_byte(v, what)])))
    if any(b in BLANKS for b in special):
        raise ValueError("special: a special byte cannot be a blank with blanks=")


def blank_field_list_records_model(data, offsets, sep_len, last_whole, ranges, quote=None, escape=None):
    """kx_run_batch_field_words's view of its records in pure Python — the normative model of `--field=LIST --blanks`.  The
    records and their bodies are field_records_model's; `ranges` is the list (what `fields=` takes).  A BLANK is the byte 0x20 or
    0x09.  A blank is LIVE under the rule that makes an `fs` byte live there: every one; with a `quote` byte one at even parity of
    the quote bytes before it in the record; with an `escape` byte one that is unescaped and at even parity of the record's
    unescaped quotes (an escaped byte is only data).  The body's fields are its WORDS: the maximal runs of body bytes that are not
    live blanks, numbered from 1.  A field is never empty, quotes and escapes stay in the word, and a body that is empty or all
    live blanks has 0 fields.  The return shape is field_list_records_model's: a record with at least field_list_need(ranges) words
    gives (gaps, fields, separator) — `fields` the m selected (K, bytes) pairs in order, `gaps` the m + 1 byte strings around them,
    every blank of the body in one of them — and a record with fewer gives the number of words it has."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError("blank_field_list_records_model: data must be bytes, not %s" % type(data).__name__)
    sep_len, ranges = _check_sep_len(sep_len), _check_field_ranges(ranges)
    if not isinstance(last_whole, bool):
        raise TypeError("blank_field_list_records_model: last_whole must be True or False, not %s" % type(last_whole).__name__)
    _check_not_blank(quote, escape)
    q = None if quote is None else _one_byte(quote, "quote character")
    e = None if escape is None else _one_byte(escape, "escape character")
    if q is not None and q == e:
        raise ValueError("escape character: %r is also the quote character" % bytes([e]))
    data, offs = bytes(data), [int(o) for o in offsets]
    check_batch_offsets(offs, len(data))
    need = field_list_need(ranges)
    n, res = len(offs) - 1, []
    for i in range(n):
        t = 0 if last_whole and i == n - 1 else sep_len
        if offs[i + 1] - offs[i] < t:
            raise ValueError("blank_field_list_records_model: record %d is shorter than its separator (%d)" % (i, t))
        body, sep = data[offs[i]:offs[i + 1] - t], data[offs[i + 1] - t:offs[i + 1]]
        words, begin, parity, esc = [], None, 0, False        # the words as (begin, end); begin: of the word the walk is in
        for k, b in enumerate(body):
            live = False
            if esc:
                esc = False
            elif e is not None and b == e:
                esc = True
            elif q is not None and b == q:
                parity ^= 1
            elif b in BLANKS and parity == 0:
                live = True
            if not live and begin is None:
                begin = k
            elif live and begin is not None:
                words.append((begin, k))
                begin = None
        if begin is not None:
            words.append((begin, len(body)))
        nf = len(words)
        if nf < need:
            res.append(nf)
            continue
        gaps, fields, at = [], [], 0
        for lo, hi in ranges:
            for K in range(lo, (nf if hi is None else hi) + 1):
                wb, we = words[K - 1]
                gaps.append(body[at:wb])
                fields.append((K, body[wb:we]))
                at = we
        gaps.append(body[at:])
        res.append((gaps, fields, sep))
    return res


FIELD_ITEMS_MAX = 16


def parse_field_order(text):
    """The LIST of `--field=LIST --only` AS WRITTEN → a tuple of (lo, hi) pairs with hi None for an open item, in the order of the
    text: the order of the output.  The number rules are parse_field_list's; items may come in any order, overlap and repeat
    ("2,1,2", "3-,1-2").  Raises ValueError for what the command line refuses: what parse_field_list refuses (the normal form of
    the items' union has at most 8 ranges), and more than 16 items."""
    parse_field_list(text)                                      # (every rule of the text but the number of items)
    items = []
    for item in text.split(","):
        a, dash, b = item.partition("-")
        items.append((int(a), int(a) if not dash else None if not b else int(b)))
    if len(items) > FIELD_ITEMS_MAX:
        raise ValueError("field list %r: %d items, at most %d with only=" % (text, len(items), FIELD_ITEMS_MAX))
    return tuple(items)


def _check_field_items(items):
    """The `items` of a projection: a parse_field_order result, or a sequence of 1 to 16 field numbers and (lo, hi) pairs (hi
    None: open), in any order → (the items as written, a tuple of pairs; the normal form of their union)."""
    ranges = _check_field_ranges(items)                         # (the types, the numbers and the union's 8 ranges)
    if len(items) > FIELD_ITEMS_MAX:
        raise ValueError("fields: %d items, at most %d with only=" % (len(items), FIELD_ITEMS_MAX))
    return tuple((it[0], it[1]) if isinstance(it, (tuple, list)) else (it, it) for it in items), ranges


def project_records_model(data, offsets, sep_len, last_whole, items, fs, quote=None, escape=None, blanks=False):
    """kx_run_batch_field_project's view of its records in pure Python — the normative model of `--field=LIST --only`.  `items` is
    the list as written (what parse_field_order gives, or a sequence of ints and (lo, hi) pairs).  The selected set is the items'
    union, and everything about it is field_list_records_model's — with `blanks` (and fs None) blank_field_list_records_model's —
    for the union's normal form: a record with fewer than `need` fields gives the number of fields it has.  Any other record
    gives ([(K, field bytes), …], separator): for each item in written order the item's fields in ascending field number, an open
    item up to the record's last field.  A field that two items name comes twice; an item none of whose fields the record has (it
    lies inside the union's open range: "3-,9-10" on five fields) gives none.  The list is never empty."""
    if not isinstance(blanks, bool):
        raise TypeError("project_records_model: blanks must be True or False, not %s" % type(blanks).__name__)
    items, ranges = _check_field_items(items)
    if blanks:
        if fs is not None:
            raise ValueError("project_records_model: blanks= cannot be combined with an fs")
        recs = blank_field_list_records_model(data, offsets, sep_len, last_whole, ranges, quote, escape)
    else:
        recs = field_list_records_model(data, offsets, sep_len, last_whole, ranges, fs, quote, escape)
    res = []
    for r in recs:
        if isinstance(r, int):
            res.append(r)
            continue
        _, fields, sep = r
        res.append(([(K, v) for lo, hi in items for K, v in fields if lo <= K and (hi is None or K <= hi)], sep))
    return res


def parse_field_keys(text):
    """The LIST of `--field=LIST --keys` → (names, optional_mask, items): the DISTINCT names as bytes in the order of their first
    item, bit t of the mask set if every item that names names[t] is optional, and the items as written as indices into names.
    The text is cut at the commas that no backslash takes with it.  Every item is a name, an all-digits item too: its bytes (the
    text's UTF-8) spelled as themselves or as \\n \\t \\r \\0 \\\\ \\, \\xHH, 1 to 255 of them; a last `?` that no backslash takes with it
    is no byte of the name and makes the item optional (a literal last `?` is spelled \\x3F).  Raises ValueError for what the
    command line refuses: a bad spelling, an empty name, one of more than 255 bytes, more than 16 items."""
    if not isinstance(text, str):
        raise TypeError("field list: a str such as 'ts,msg?', not %s" % type(text).__name__)
    raw, cuts, taken, i = text.encode("utf-8", "surrogateescape"), [], set(), 0
    while i < len(raw):
        if raw[i] == 0x5C and i + 1 < len(raw):
            i += 1
            taken.add(i)
        elif raw[i] == 0x2C:
            cuts.append(i)
        i += 1
    names, items, required = [], [], 0
    for b, e in zip([0] + [c + 1 for c in cuts], cuts + [len(raw)]):
        optional = e > b and raw[e - 1] == 0x3F and (e - 1) not in taken
        item, name, k = raw[b:e - 1 if optional else e], bytearray(), 0
        while k < len(item):
            if item[k] != 0x5C:
                name.append(item[k])
                k += 1
                continue
            c = item[k + 1:k + 2]
            if c in (b"n", b"t", b"r", b"0", b"\\", b","):
                name += {b"n": b"\n", b"t": b"\t", b"r": b"\r", b"0": b"\0", b"\\": b"\\", b",": b","}[c]
                k += 2
            elif c == b"x" and re.fullmatch(rb"[0-9a-fA-F]{2}", item[k + 2:k + 4]):
                name.append(int(item[k + 2:k + 4], 16))
                k += 4
            else:
                raise ValueError("field list %r: a backslash in a name starts \\n \\t \\r \\0 \\\\ \\, or \\xHH" % text)
        if not name:
            raise ValueError("field list %r: an empty name" % text)
        if len(name) > FIELD_NAME_MAX:
            raise ValueError("field list %r: a name has at most %d bytes" % (text, FIELD_NAME_MAX))
        if len(items) == FIELD_ITEMS_MAX:
            raise ValueError("field list %r: more than %d items" % (text, FIELD_ITEMS_MAX))
        name = bytes(name)
        if name not in names:
            names.append(name)
        items.append(names.index(name))
        if not optional:
            required |= 1 << items[-1]
    return tuple(names), ((1 << len(names)) - 1) & ~required, tuple(items)


def _check_field_keys(what, fields, optional, kv, fs, blanks, quote=None, escape=None, sep=None):
    """The names of a keyed call: `fields`, 1 to 16 bytes names of 1 to 255 bytes (repeats allowed); `optional`, those of them a
    record may lack; `kv`, the key separator C, which is not `fs` (with `blanks`: no blank), the quote, the escape or the one-byte
    record separator `sep`; no name holds C, `fs` (a blank) or `sep` → (the distinct names, optional_mask, the items as indices,
    C as an int)."""
    if not isinstance(fields, (tuple, list)) or not fields or not all(isinstance(n, (bytes, bytearray)) for n in fields):
        raise TypeError("%s: with keys= fields is a sequence of bytes names" % what)
    if len(fields) > FIELD_ITEMS_MAX:
        raise ValueError("%s: fields: %d items, at most %d" % (what, len(fields), FIELD_ITEMS_MAX))
    c = _one_byte(kv, "key separator")
    f = None if blanks else _one_byte(fs, "field separator")
    s = None if sep is None else _one_byte(sep, "record separator")
    if c == f or (blanks and c in BLANKS) or c == s:
        raise ValueError("%s: keys: %r is also the field or the record separator" % (what, bytes([c])))
    if (quote is not None and c == _one_byte(quote, "quote character")) or (escape is not None and c == _one_byte(escape, "escape character")):
        raise ValueError("%s: keys: %r is also the quote or the escape character" % (what, bytes([c])))
    names = []
    for n in fields:
        n = bytes(n)
        if not 1 <= len(n) <= FIELD_NAME_MAX:
            raise ValueError("%s: fields: a name has 1 to %d bytes, not %d" % (what, FIELD_NAME_MAX, len(n)))
        if c in n or (f is not None and f in n) or (blanks and any(b in BLANKS for b in n)) or (s is not None and s in n):
            raise ValueError("%s: fields: the name %r holds the key, the field or the record separator" % (what, n))
        if n not in names:
            names.append(n)
    mask = 0
    for n in optional:
        if not isinstance(n, (bytes, bytearray)) or bytes(n) not in names:
            raise ValueError("%s: optional: %r is no name of fields" % (what, n))
        mask |= 1 << names.index(bytes(n))
    return tuple(names), mask, tuple(names.index(bytes(n)) for n in fields), c


def keyed_records_model(data, offsets, sep_len, last_whole, names, kv=b"=", fs=b"\t", quote=None, escape=None, blanks=False, optional=()):
    """kx_run_batch_field_keys's view of its records in pure Python — the normative model of `--field=LIST --keys[=C]`.  The
    records, their bodies and their fields are field_list_records_model's — with `blanks` (and fs None) the words of
    blank_field_list_records_model.  Inside a field the KEY is the bytes before the field's first live `kv` byte — live under the
    rule that makes an `fs` byte live: parity 0 and not escaped, with the record's running state — and the VALUE everything behind
    that byte up to the field's end; a field without a live `kv` byte has no key, an empty key matches nothing, and keys are
    compared as raw bytes.  Each of `names` (distinct bytes) selects the FIRST field that has it for a key.  A record that lacks a
    name not in `optional` gives an int, the mask of the names it has (bit t: names[t]).  Any other record gives (gaps, fields,
    separator): `fields` the m selected (t, value bytes) pairs in ADDRESS order and `gaps` the m + 1 byte strings around them — keys
    and `kv` bytes included — so that the body is gaps[0] + fields[0][1] + gaps[1] + … + gaps[m]; m may be 0."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError("keyed_records_model: data must be bytes, not %s" % type(data).__name__)
    if not isinstance(blanks, bool) or not isinstance(last_whole, bool):
        raise TypeError("keyed_records_model: blanks and last_whole must be True or False")
    if blanks and fs is not None:
        raise ValueError("keyed_records_model: blanks= cannot be combined with an fs")
    sep_len = _check_sep_len(sep_len)
    given = list(names)
    names, opt, _, c = _check_field_keys("keyed_records_model", given, optional, kv, fs, blanks, quote, escape)
    if len(names) != len(given):
        raise ValueError("keyed_records_model: the names are distinct")
    f = None if blanks else _check_fs(fs, quote, escape)
    if blanks:
        _check_not_blank(quote, escape)
    q = None if quote is None else _one_byte(quote, "quote character")
    e = None if escape is None else _one_byte(escape, "escape character")
    if q is not None and q == e:
        raise ValueError("escape character: %r is also the quote character" % bytes([e]))
    required = ((1 << len(names)) - 1) & ~opt
    data, offs = bytes(data), [int(o) for o in offsets]
    check_batch_offsets(offs, len(data))
    n, res = len(offs) - 1, []
    for i in range(n):
        t = 0 if last_whole and i == n - 1 else sep_len
        if offs[i + 1] - offs[i] < t:
            raise ValueError("keyed_records_model: record %d is shorter than its separator (%d)" % (i, t))
        body, sep = data[offs[i]:offs[i + 1] - t], data[offs[i + 1] - t:offs[i + 1]]
        fields, firstc, begin, parity, esc = [], None, None if blanks else 0, 0, False   # fields: (begin, first live C or None, end)
        for k, b in enumerate(body):
            live = livec = False
            if esc:
                esc = False
            elif e is not None and b == e:
                esc = True
            elif q is not None and b == q:
                parity ^= 1
            elif parity == 0:
                live = b in BLANKS if blanks else b == f
                livec = not live and b == c
            if blanks:
                if not live and begin is None:
                    begin, firstc = k, None
                elif live and begin is not None:
                    fields.append((begin, firstc, k))
                    begin = None
            elif live:
                fields.append((begin, firstc, k))
                begin, firstc = k + 1, None
            if livec and firstc is None:
                firstc = k
        if begin is not None:
            fields.append((begin, firstc, len(body)))
        found, sel = 0, []
        for fbeg, fc, fend in fields:
            key = body[fbeg:fc] if fc is not None else b""
            if key in names and not found >> names.index(key) & 1:
                found |= 1 << names.index(key)
                sel.append((names.index(key), fc + 1, fend))
        if required & ~found:
            res.append(found)
            continue
        gaps, out, at = [], [], 0
        for tix, vb, ve in sel:
            gaps.append(body[at:vb])
            out.append((tix, body[vb:ve]))
            at = ve
        gaps.append(body[at:])
        res.append((gaps, out, sep))
    return res


class KxFieldKeys(ctypes.Structure):
    """include/kxhip.h::kx_field_keys."""
    _fields_ = [("size", ctypes.c_uint32), ("n_names", ctypes.c_uint32), ("names", ctypes.c_char_p * 16), ("name_len", ctypes.c_uint32 * 16),
                ("optional_mask", ctypes.c_uint32), ("kv", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 3), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 4)]


KX_KEYS_WORDS, KX_KEYS_UNQUOTE, KX_KEYS_ONLY = 1, 2, 4


def field_keys_struct(names, optional_mask, kv, flags=0):
    """A kx_field_keys for the distinct bytes `names`.  Nothing is checked here: the library does that."""
    k = KxFieldKeys(size=ctypes.sizeof(KxFieldKeys), n_names=len(names), optional_mask=optional_mask, kv=kv, flags=flags)
    for j, name in enumerate(names[:16]):
        k.names[j], k.name_len[j] = bytes(name), len(name)
    return k


class KxFieldProject(ctypes.Structure):
    """include/kxhip.h::kx_field_project."""
    _fields_ = [("size", ctypes.c_uint32), ("n_items", ctypes.c_uint32), ("items", KxFieldRange * 16), ("ofs_len", ctypes.c_uint32),
                ("ofs", ctypes.c_uint8 * 8), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 4)]


KX_PROJECT_WORDS, KX_PROJECT_UNQUOTE = 1, 2


KX_E_HEADER = -6
KX_TABLE_WORDS, KX_TABLE_UNQUOTE, KX_TABLE_ONLY, KX_TABLE_SINGLE = 1, 2, 4, 8
FIELD_NAME_MAX = 255


class KxRecordsTable(ctypes.Structure):
    """include/kxhip.h::kx_records_table."""
    _fields_ = [("size", ctypes.c_uint32), ("header", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_items", ctypes.c_uint32),
                ("items", KxFieldRange * 16), ("n_names", ctypes.c_uint32), ("names", ctypes.c_char_p * 16),
                ("name_len", ctypes.c_uint32 * 16), ("fs", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 3), ("ofs_len", ctypes.c_uint32),
                ("ofs", ctypes.c_uint8 * 8), ("reserved", ctypes.c_uint32 * 4)]


def records_table(header=0, items=(), flags=0, fs=0, ofs=b""):
    """A KxRecordsTable: `items` as written — ints, (lo, hi) pairs (hi None or 0: open) and bytes names, which go to the table's
    names in the order of their first appearance.  Nothing is checked here: the library does that."""
    t = KxRecordsTable(size=ctypes.sizeof(KxRecordsTable), header=header, flags=flags, n_items=len(items), fs=fs, ofs_len=len(ofs))
    names = []
    for j, it in enumerate(items[:16]):
        if isinstance(it, (bytes, bytearray)):
            if bytes(it) not in names:
                names.append(bytes(it))
            t.items[j].lo, t.items[j].hi = 0, names.index(bytes(it))
        elif isinstance(it, (tuple, list)):
            t.items[j].lo, t.items[j].hi = it[0], it[1] or 0
        else:
            t.items[j].lo = t.items[j].hi = it
    t.n_names = len(names)
    for j, name in enumerate(names):
        t.names[j], t.name_len[j] = name, len(name)
    t.ofs[:min(len(ofs), 8)] = ofs[:8]
    return t


def parse_field_names(text):
    """The LIST of `--header --field=LIST` as written → a tuple of ints (K), (lo, hi) pairs (A-B; A- with hi None) and bytes (a
    NAME), in the order of the text.  The text is cut at the commas that no backslash takes with it (a backslash always takes the
    next character).  An item made only of digits and '-' is a number item with parse_field_order's rules.  Every other item is a
    name: its bytes (the text's UTF-8) spelled as themselves or as \\n \\t \\r \\0 \\\\ \\, \\xHH, 1 to 255 of them.  Raises ValueError for
    what the command line refuses: a bad number item, a bad spelling, a name of more than 255 bytes, more than 16 items, and a list
    of numbers alone whose union has more than 8 ranges."""
    if not isinstance(text, str):
        raise TypeError("field list: a str such as '2,name,5-', not %s" % type(text).__name__)
    raw, cuts, i = text.encode("utf-8", "surrogateescape"), [], 0
    while i < len(raw):
        if raw[i] == 0x5C and i + 1 < len(raw):
            i += 1
        elif raw[i] == 0x2C:
            cuts.append(i)
        i += 1
    items, named = [], False
    for b, e in zip([0] + [c + 1 for c in cuts], cuts + [len(raw)]):
        item = raw[b:e]
        if all(c in b"0123456789-" for c in item):
            (lo, hi), = parse_field_order(item.decode("ascii"))      # (the empty item is refused there)
            items.append(lo if hi == lo else (lo, hi))
            continue
        named, name, k = True, bytearray(), 0
        while k < len(item):
            if item[k] != 0x5C:
                name.append(item[k])
                k += 1
                continue
            c = item[k + 1:k + 2]
            if c in (b"n", b"t", b"r", b"0", b"\\", b","):
                name += {b"n": b"\n", b"t": b"\t", b"r": b"\r", b"0": b"\0", b"\\": b"\\", b",": b","}[c]
                k += 2
            elif c == b"x" and re.fullmatch(rb"[0-9a-fA-F]{2}", item[k + 2:k + 4]):
                name.append(int(item[k + 2:k + 4], 16))
                k += 4
            else:
                raise ValueError("field list %r: a backslash in a name starts \\n \\t \\r \\0 \\\\ \\, or \\xHH" % text)
        if len(name) > FIELD_NAME_MAX:
            raise ValueError("field list %r: a name has at most %d bytes" % (text, FIELD_NAME_MAX))
        items.append(bytes(name))
    if len(items) > FIELD_ITEMS_MAX:
        raise ValueError("field list %r: %d items, at most %d" % (text, len(items), FIELD_ITEMS_MAX))
    if not named:
        parse_field_order(text)
    return tuple(items)


def header_names_model(body, fs, quote=None, escape=None, blanks=False, first=False):
    """The names of the cells of a header record's `body` (the record without its separator) in pure Python — the normative model
    of what `--header` resolves names against.  The cells lie between the live `fs` bytes, as field_records_model has them (the
    empty body has one empty cell); with `blanks` (and fs None) they are the body's words, as blank_field_list_records_model has
    them.  A cell's name is its bytes; with a `quote` or an `escape` byte it is the cell's unquote_field_model value.  With `first`
    (the record is the stream's first) a leading EF BB BF is cut off before anything else."""
    if not isinstance(body, (bytes, bytearray, memoryview)):
        raise TypeError("header_names_model: body must be bytes, not %s" % type(body).__name__)
    for name, v in (("blanks", blanks), ("first", first)):
        if not isinstance(v, bool):
            raise TypeError("header_names_model: %s must be True or False, not %s" % (name, type(v).__name__))
    body = bytes(body)
    if first and body[:3] == b"\xef\xbb\xbf":
        body = body[3:]
    if blanks:
        if fs is not None:
            raise ValueError("header_names_model: blanks= cannot be combined with an fs")
        rec = blank_field_list_records_model(body, [0, len(body)], 0, False, [(1, None)], quote, escape)[0]
    else:
        rec = field_list_records_model(body, [0, len(body)], 0, False, [(1, None)], fs, quote, escape)[0]
    cells = [] if isinstance(rec, int) else [v for _, v in rec[1]]
    if quote is None and escape is None:
        return cells
    return [unquote_field_model(c, quote, escape) for c in cells]


def resolve_field_names(items, names):
    """`items` — ints, (lo, hi) pairs and bytes names, as parse_field_names gives them — against the cell `names` of the header
    record → the items with every name replaced by the number (from 1) of the lowest-numbered cell that has it.  Raises HeaderError
    for a name no cell has."""
    names = [bytes(n) for n in names]
    out = []
    for it in items:
        if isinstance(it, (bytes, bytearray)):
            if bytes(it) not in names:
                raise HeaderError(bytes(it))
            it = names.index(bytes(it)) + 1
        out.append(it)
    return out


def _check_header(what, header, fields):
    """The `header=` keyword of record mode: an int in [0, 2^32); names in `fields` only with header >= 1, each 1 to 255 bytes,
    in a list of at most 16 items → (header, whether `fields` holds a name)."""
    if isinstance(header, bool) or not isinstance(header, int):
        raise TypeError("%s: header must be an int, not %s" % (what, type(header).__name__))
    if not 0 <= header < 1 << 32:
        raise ValueError("%s: header: %d is not in [0, 2^32)" % (what, header))
    names = [it for it in fields if isinstance(it, (bytes, bytearray))] if isinstance(fields, (tuple, list)) else []
    if names and not header:
        raise ValueError("%s: names in fields= need header >= 1" % what)
    if names and len(fields) > FIELD_ITEMS_MAX:
        raise ValueError("%s: fields: %d items, at most %d in a list with a name" % (what, len(fields), FIELD_ITEMS_MAX))
    for n in names:
        if not 1 <= len(n) <= FIELD_NAME_MAX:
            raise ValueError("%s: fields: a name has 1 to %d bytes, not %d" % (what, FIELD_NAME_MAX, len(n)))
    return header, bool(names)


def _field_item_array(items):
    """Items as written → (KxFieldRange * 16, n_items)."""
    a = (KxFieldRange * 16)()
    for j, (lo, hi) in enumerate(items):
        a[j].lo, a[j].hi = lo, hi or 0
    return a, len(items)


def _check_ofs(ofs):
    """An output field separator: 0 to 8 bytes → bytes."""
    if not isinstance(ofs, (bytes, bytearray)):
        raise TypeError("ofs: bytes of length 0 to 8, not %s" % type(ofs).__name__)
    if len(ofs) > 8:
        raise ValueError("ofs: 0 to 8 bytes, not %d" % len(ofs))
    return bytes(ofs)


def _check_ofs_codec(what, ofs, q, e, special):
    """On values OFS is what the spelling protects: one byte that is not the quote, the escape or a special byte."""
    if len(ofs) != 1:
        raise ValueError("%s: with unquote= the ofs is exactly one byte, not %d" % (what, len(ofs)))
    if ofs[0] in (q, e) or ofs[0] in special:
        raise ValueError("%s: with unquote= the ofs cannot be the quote, the escape or a special byte" % what)


class KxFieldCodec(ctypes.Structure):
    """include/kxhip.h::kx_field_codec."""
    _fields_ = [("size", ctypes.c_uint32), ("n_special", ctypes.c_uint32), ("special", ctypes.c_uint8 * 8), ("reserved", ctypes.c_uint32 * 4)]


def _check_codec(what, quote, escape, special=b""):
    """The bytes of the two value models and of `unquote=`: a quote or an escape byte (or both, different), and 0 to 8 special
    bytes that are neither → (Q, E, special) with None for a byte that is not set."""
    if quote is None and escape is None:
        raise ValueError("%s: values need a quote= or an escape= byte" % what)
    q = None if quote is None else _one_byte(quote, "quote character")
    e = None if escape is None else _one_byte(escape, "escape character")
    if q is not None and q == e:
        raise ValueError("escape character: %r is also the quote character" % bytes([e]))
    if not isinstance(special, (bytes, bytearray)):
        raise TypeError("%s: special must be bytes of length 0 to 8, not %s" % (what, type(special).__name__))
    if len(special) > 8:
        raise ValueError("%s: special must be 0 to 8 bytes, not %d" % (what, len(special)))
    if any(b in (q, e) for b in special):
        raise ValueError("%s: a special byte cannot be the quote or the escape character" % what)
    return q, e, bytes(special)


def unquote_field_model(raw, quote=None, escape=None):
    """The VALUE of a field spelled `raw` — the normative model of `--unquote`'s decoding (kx_run_batch_field_values).  The quote
    bytes that open and close quoted stretches and the escape bytes are not part of it: the byte behind an unescaped escape byte is
    data (a last escape byte alone is dropped), a quote that opens right behind one that closed — the "" of a quoted field — is one
    quote byte.  The rule is total and keeps the parity rule of the splitters: a quote in the middle of a field toggles the state,
    an unclosed quote is simply dropped."""
    if not isinstance(raw, (bytes, bytearray, memoryview)):
        raise TypeError("unquote_field_model: raw must be bytes, not %s" % type(raw).__name__)
    Q, E, _ = _check_codec("unquote_field_model", quote, escape)
    raw = bytes(raw)
    out, s, pc, i = bytearray(), 0, False, 0                    # s: inside quotes; pc: the previous byte was a closing quote
    while i < len(raw):
        b = raw[i]
        if E is not None and b == E:
            if i + 1 < len(raw):
                out.append(raw[i + 1])
            i += 2
            pc = False
            continue
        if Q is not None and b == Q:
            if s:
                s, pc = 0, True
            else:
                s = 1
                if pc:
                    out.append(Q)
                pc = False
            i += 1
            continue
        out.append(b)
        pc = False
        i += 1
    return bytes(out)


def requote_field_model(value, was_quoted, fs, quote=None, escape=None, special=b"\n"):
    """The SPELLING of a program output `value` in place of a field — the normative model of `--unquote`'s encoding.  `special`:
    the bytes that must not appear bare (the records driver passes the record separator); `was_quoted`: a quote byte is set and
    the raw field began with it.  Quote, no escape: wrapped — quote, the value with every quote doubled, quote — iff was_quoted or
    the value holds `fs`, the quote or a special byte.  Escape: every escape byte gets an escape byte in front of it; with a quote
    every quote byte too, and the result is wrapped iff was_quoted or the value holds `fs` or a special byte; without one every `fs`
    and special byte gets one as well.  (A rejected field is spelled as nothing: that is the caller's, not this function's.)"""
    if not isinstance(value, (bytes, bytearray, memoryview)):
        raise TypeError("requote_field_model: value must be bytes, not %s" % type(value).__name__)
    if not isinstance(was_quoted, bool):
        raise TypeError("requote_field_model: was_quoted must be True or False, not %s" % type(was_quoted).__name__)
    F = _check_fs(fs, quote, escape)
    Q, E, special = _check_codec("requote_field_model", quote, escape, special)
    value = bytes(value)
    bare = set(special) | {F}
    if E is None:
        if not (was_quoted or any(b in bare or b == Q for b in value)):
            return value
        return bytes([Q]) + value.replace(bytes([Q]), bytes([Q, Q])) + bytes([Q])
    front = {E} | ({Q} if Q is not None else bare)
    body = b"".join(bytes([E, b]) if b in front else bytes([b]) for b in value)
    if Q is not None and (was_quoted or any(b in bare for b in value)):
        return bytes([Q]) + body + bytes([Q])
    return body


def _check_values(values, what):
    import torch
    if not isinstance(values, torch.Tensor):
        raise TypeError("%s: values must be a torch tensor, not %s" % (what, type(values).__name__))
    if values.dtype != torch.uint8 or values.dim() != 1:
        raise TypeError("%s: values must be a 1-D uint8 tensor (got %s, %d-D)" % (what, values.dtype, values.dim()))
    if values.numel() and values.stride(0) != 1:
        raise ValueError("%s: values must be contiguous" % what)


def _records_mode(quote, escape, rs):
    """KX_RECORDS_* of the keywords of a record-mode call (`rs` comes alone; an `escape` may come with a `quote`)."""
    return KX_RECORDS_RS if rs is not None else KX_RECORDS_ESCAPED if escape is not None else \
        KX_RECORDS_QUOTED if quote is not None else KX_RECORDS_BYTE


def _split_tensor(what, values, entry, checks, outs=()):
    """What the split_*_tensor functions (`what`) share: the checks of `values`, then `checks()` — the function's own, giving
    the C arguments of `entry` between n and base — the size query, the allocation and the split.  `outs`: the C arguments
    behind n_records.  Returns the offsets."""
    _check_values(values, what)
    args = checks()
    import torch
    if not values.is_cuda:
        raise EngineError("%s: values must be on a HIP device (there is no CPU fallback)" % what)
    lib = load_engine()
    call = getattr(lib, entry)
    stream = ctypes.c_void_p(torch.cuda.current_stream(values.device).cuda_stream)
    vptr = ctypes.c_void_p(values.data_ptr() if values.numel() else None)
    n = ctypes.c_uint64()
    rc = call(vptr, values.numel(), *args, 0, None, 0, ctypes.byref(n), *outs, stream)
    if rc not in (0, -3):
        raise EngineError(lib.kx_last_error().decode("utf-8", "replace"))
    off = torch.empty(n.value + 1, dtype=torch.int64, device=values.device)
    rc = call(vptr, values.numel(), *args, 0, ctypes.c_void_p(off.data_ptr()), off.numel(), ctypes.byref(n), *outs, stream)
    if rc:
        raise EngineError(lib.kx_last_error().decode("utf-8", "replace"))
    return off


def split_records_tensor(values, sep=b"\n"):
    """kx_split_records: the record offsets of a CUDA uint8 tensor (any start address) as an int64 device tensor of
    n_records + 1 entries, relative to values[0] — the offsets run_batch_tensor takes.  Runs on the current stream, blocks."""
    return _split_tensor("split_records_tensor", values, "kx_split_records", lambda: (_check_sep(sep),))


def split_quoted_records_tensor(values, sep=b"\n", quote=b'"', parity=0):
    """kx_split_records_quoted: split_records_tensor where a separator inside quotes ends no record (split_records_model's
    `quote`).  `parity` is the quote parity at values[0].  Returns (offsets, parity after the last byte)."""
    pout = ctypes.c_uint32()
    off = _split_tensor("split_quoted_records_tensor", values, "kx_split_records_quoted",
                        lambda: (_check_sep(sep), _check_quote(quote, sep), _check_parity(parity)), (ctypes.byref(pout),))
    return off, pout.value


def split_escaped_records_tensor(values, sep=b"\n", quote=None, escape=b"\\", state=0):
    """kx_split_records_escaped: split_records_tensor where an escaped byte is only data and, with a `quote` byte, a separator
    inside quotes ends no record (split_escaped_records_model).  `state` is the state at values[0] (bit 0 quote parity, bit 1
    escaped).  Returns (offsets, state after the last byte)."""
    sout = ctypes.c_uint32()
    off = _split_tensor("split_escaped_records_tensor", values, "kx_split_records_escaped",
                        lambda: (_check_sep(sep), -1 if quote is None else _check_quote(quote, sep), _check_escape(escape, sep, quote),
                                 _check_state(state, quote)), (ctypes.byref(sout),))
    return off, sout.value


def split_rs_records_tensor(values, rs, ctx=b""):
    """kx_split_records_rs: split_records_tensor for a separator `rs` of 1 to 8 bytes (split_rs_records_model); `ctx` is the
    context before values[0].  Returns (offsets, (ctx_out, tail_len))."""
    def checks():
        r = _check_rs(rs)
        c = _check_ctx(ctx, r)
        return r, len(r), c, len(c)

    col, tl, cout = ctypes.c_uint32(), ctypes.c_uint64(), (ctypes.c_uint8 * 8)()
    off = _split_tensor("split_rs_records_tensor", values, "kx_split_records_rs", checks, (cout, ctypes.byref(col), ctypes.byref(tl)))
    return off, (bytes(cout[:col.value]), tl.value)


class KxDfInfo(ctypes.Structure):
    """include/kxhip.h::kx_df_info — the delayed form of one stage."""
    _fields_ = [(k, ctypes.c_uint32) for k in ("available", "delay", "nstates", "nclasses", "image_bytes", "off_pool", "start_handle",
                                               "dead_handle", "escape_handle", "transitions", "escapes", "transitions_start",
                                               "escapes_start", "merge_window")] + [("reason", ctypes.c_char * 96)]


class _KxStageTables(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint64) for k in ("packed", "pair", "wlen", "cls", "nleaves", "fin_leaf", "sync16", "init_off", "init_len")] + \
               [(k, ctypes.c_uint32) for k in ("packed_words", "off_fwd", "off_ent", "off_pool", "off_cls", "off_adesc", "naid", "nstates", "nclasses",
                                               "q0h", "maxleaves", "deadh", "nullrow", "cshift", "debug", "big", "hshift", "rshift", "rbase",
                                               "stage_words", "pair_words", "pair_magic", "nsync", "sync_multi", "sync_words", "off_tbl", "xlat",
                                               "tblmode", "aid_mask", "inl", "jl", "direct", "short_consts", "reserved0")]


class _KxStageDelayed(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint64) for k in ("img", "start_of_state", "sl_fmap", "sl_back", "sl_nleaves", "sl_fin_leaf", "sl_cls", "sl_pcoff",
                                               "sl_pcpool", "sl_pend", "sl_defoff", "sl_defpc", "sl_q")] + \
               [(k, ctypes.c_uint32) for k in ("words", "off_pool", "deadh", "esch", "starth", "K", "C", "orig_c4", "hshift", "short_consts", "debug",
                                               "nstates", "J", "wide", "sl_Lm", "sl_npc", "sl_on", "reserved0")]


class KxStageInfo(ctypes.Structure):
    """include/kxhip.h::kx_stage_info — what the loader builds for one stage (layout decision, DevTables `t`, DfDev `d`)."""
    _fields_ = [("size", ctypes.c_uint32), ("which", ctypes.c_uint32), ("image_bytes", ctypes.c_uint64)] + \
               [(k, ctypes.c_uint32) for k in ("general", "big", "has_alt", "has_df", "actions", "action_regs", "max_const_len", "reserved0")] + \
               [("lds_bytes", ctypes.c_uint64), ("sync_lds_bytes", ctypes.c_uint64), ("t", _KxStageTables), ("d", _KxStageDelayed)]

    def as_dict(self):
        """every field but size / which / reserved, nested ones as "t.inl" """
        out = {}
        for k, _ in self._fields_:
            v = getattr(self, k)
            if isinstance(v, ctypes.Structure):
                out.update({"%s.%s" % (k, f): getattr(v, f) for f, _ in v._fields_ if f != "reserved0"})
            elif k not in ("size", "which", "reserved0"):
                out[k] = v
        return out


KX_STAGE_MAIN, KX_STAGE_ALT, KX_STAGE_DELAYED, KX_STAGE_SLOW = 0, 1, 2, 3


class KxFwdSummary(ctypes.Structure):
    _fields_ = [("synced", ctypes.c_uint32), ("end_state", ctypes.c_uint32),
                ("head_len", ctypes.c_uint64), ("fail_pos", ctypes.c_uint64)]


class KxBwdSummary(ctypes.Structure):
    _fields_ = [("constant", ctypes.c_uint32), ("nleaves", ctypes.c_uint32),
                ("start_leaf", ctypes.c_uint8 * KX_MAX_LEAVES)]


_kexc = None
_kxhip = None


def _lib_path(name):
    return os.path.join(BUILD_DIR, name)


def load_compiler():
    """dlopen libkexc.so (built by ``kleenexlang_amd.build`` / ``__graft_entry__.build``)."""
    global _kexc
    if _kexc is None:
        path = _lib_path("libkexc.so")
        if not os.path.exists(path):
            raise CompileError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
        lib = ctypes.CDLL(path)
        lib.kexc_compile.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int,
                                     ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        lib.kexc_emit_c.argtypes = lib.kexc_compile.argtypes
        lib.kexc_last_error.restype = ctypes.c_char_p
        lib.kexc_free.argtypes = [ctypes.c_void_p]
        _kexc = lib
    return _kexc


def load_engine():
    """dlopen libkxhip.so; raises if it has not been built (no fallback)."""
    global _kxhip
    if _kxhip is None:
        path = _lib_path("libkxhip.so")
        if not os.path.exists(path):
            raise EngineError("HIP engine %s is missing: build it with __graft_entry__.build(); "
                              "there is no CPU fallback" % path)
        try:
            # torch wheels bundle their own libamdhip64.so.7; /opt/rocm ships one with the same soname.
            # Whichever is mapped first serves the whole process, and torch cannot initialise on the
            # other one — so inside a torch process let torch's runtime load first.  (C consumers such
            # as kxrun simply get the system runtime.)
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(path)
        vp, sz, u32, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64
        lib.kx_load.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(vp)]
        lib.kx_load_config.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(KxConfig), ctypes.POINTER(vp)]
        lib.kx_stage_reset_delayed_form.argtypes = [vp, u32]
        lib.kx_stage_reset_delayed_form.restype = None
        lib.kx_validate.argtypes = [ctypes.c_char_p, sz]
        lib.kx_free.argtypes = [vp]
        lib.kx_last_error.restype = ctypes.c_char_p
        lib.kx_set_config.argtypes = [vp, ctypes.POINTER(KxConfig)]
        lib.kx_num_stages.argtypes = [vp]
        lib.kx_num_stages.restype = u32
        lib.kx_stage_has_actions.argtypes = [vp, u32]
        lib.kx_stage_delayed_form.argtypes = [vp, u32]
        lib.kx_df_describe.argtypes = [ctypes.c_char_p, sz, u32, ctypes.POINTER(KxDfInfo), vp, sz]
        lib.kx_df_pending.argtypes = [ctypes.c_char_p, sz, u32, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
        cfgp = ctypes.POINTER(KxConfig)
        lib.kx_df_describe_cfg.argtypes = [ctypes.c_char_p, sz, u32, cfgp, ctypes.POINTER(KxDfInfo), vp, sz]
        lib.kx_stage_describe_cfg.argtypes = [ctypes.c_char_p, sz, u32, cfgp, u32, ctypes.POINTER(KxStageInfo), vp, sz]
        lib.kx_df_pending_cfg.argtypes = [ctypes.c_char_p, sz, u32, cfgp, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
        lib.kx_df_deferred.argtypes = [ctypes.c_char_p, sz, u32, cfgp, u32, ctypes.c_void_p, sz, ctypes.POINTER(sz)]
        lib.kx_df_start_of_state.argtypes = [ctypes.c_char_p, sz, u32, cfgp, u32, ctypes.POINTER(u32)]
        lib.kx_run_device.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(KxStats), vp]
        lib.kx_run_host.argtypes = [vp, ctypes.c_char_p, sz, ctypes.POINTER(vp), ctypes.POINTER(sz),
                                    ctypes.POINTER(KxStats)]
        lib.kx_host_free.argtypes = [vp]
        lib.kx_run_fd.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(KxStats)]
        lib.kx_run_batch.argtypes = [vp, vp, vp, u64, vp, sz, vp, vp, ctypes.POINTER(sz), ctypes.POINTER(KxBatchStats), vp]
        lib.kx_run_batch_framed.argtypes = [vp, vp, vp, u64, ctypes.POINTER(KxBatchFrame), vp, sz, vp, vp, ctypes.POINTER(sz),
                                            ctypes.POINTER(KxBatchStats), vp]
        lib.kx_run_batch_fields.argtypes = [vp, vp, vp, u64, ctypes.POINTER(KxBatchFields), vp, sz, vp, vp, ctypes.POINTER(sz),
                                            ctypes.POINTER(KxBatchStats), vp]
        lib.kx_fields_stats.argtypes = [vp, ctypes.POINTER(KxFieldsKernelStats)]
        lib.kx_run_batch_field_list.argtypes = [vp, vp, vp, u64, ctypes.POINTER(KxBatchFieldList), vp, sz, vp, vp, vp, ctypes.POINTER(sz),
                                                ctypes.POINTER(KxBatchStats), vp]
        lib.kx_run_records_fd_field_list.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(KxRecordsOpts), ctypes.POINTER(KxFieldRange),
                                                     u32, ctypes.c_uint8, ctypes.c_int, ctypes.POINTER(KxRecordsStats)]
        lib.kx_run_batch_field_values.argtypes = [vp, vp, vp, u64, ctypes.POINTER(KxBatchFieldList), ctypes.POINTER(KxFieldCodec), vp, sz, vp, vp, vp,
                                                  ctypes.POINTER(sz), ctypes.POINTER(KxBatchStats), vp]
        lib.kx_run_records_fd_field_values.argtypes = lib.kx_run_records_fd_field_list.argtypes
        lib.kx_run_batch_field_words.argtypes = lib.kx_run_batch_field_values.argtypes
        lib.kx_run_records_fd_field_words.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(KxRecordsOpts), ctypes.POINTER(KxFieldRange),
                                                      u32, ctypes.c_int, ctypes.c_int, ctypes.POINTER(KxRecordsStats)]
        lib.kx_run_batch_field_project.argtypes = [vp, vp, vp, u64, ctypes.POINTER(KxBatchFieldList), ctypes.POINTER(KxFieldCodec),
                                                   ctypes.POINTER(KxFieldProject), vp, sz, vp, vp, vp, ctypes.POINTER(sz),
                                                   ctypes.POINTER(KxBatchStats), vp]
        lib.kx_run_records_fd_field_project.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(KxRecordsOpts), ctypes.POINTER(KxFieldRange),
                                                        u32, ctypes.c_uint8, ctypes.c_char_p, u32, u32, ctypes.c_int,
                                                        ctypes.POINTER(KxRecordsStats)]
        lib.kx_run_batch_field_header.argtypes = lib.kx_run_batch_field_project.argtypes
        lib.kx_run_batch_field_keys.argtypes = [vp, vp, vp, u64, ctypes.POINTER(KxBatchFieldList), ctypes.POINTER(KxFieldKeys),
                                                ctypes.POINTER(KxFieldCodec), ctypes.POINTER(KxFieldProject), vp, sz, vp, vp, vp,
                                                ctypes.POINTER(sz), ctypes.POINTER(KxBatchStats), vp]
        lib.kx_run_records_fd_field_keys.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(KxRecordsOpts), ctypes.POINTER(KxFieldKeys),
                                                     ctypes.c_uint8, ctypes.POINTER(u32), u32, ctypes.c_char_p, u32, ctypes.c_int,
                                                     ctypes.POINTER(KxRecordsStats)]
        lib.kx_run_records_fd_table.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(KxRecordsOpts), ctypes.POINTER(KxRecordsTable),
                                                ctypes.c_int, ctypes.POINTER(KxRecordsStats)]
        lib.kx_run_records_fd_fields.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(KxRecordsOpts), u32, ctypes.c_uint8,
                                                 ctypes.c_int, ctypes.POINTER(KxRecordsStats)]
        lib.kx_run_records_fd_opts.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(KxRecordsOpts), ctypes.c_int,
                                               ctypes.POINTER(KxRecordsStats)]
        lib.kx_split_records.argtypes = [vp, sz, ctypes.c_uint8, u64, vp, u64, ctypes.POINTER(u64), vp]
        lib.kx_run_records_fd.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint8, ctypes.c_int, ctypes.POINTER(KxRecordsStats)]
        lib.kx_split_records_quoted.argtypes = [vp, sz, ctypes.c_uint8, ctypes.c_uint8, u32, u64, vp, u64, ctypes.POINTER(u64),
                                                ctypes.POINTER(u32), vp]
        lib.kx_run_records_fd_quoted.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_int,
                                                 ctypes.POINTER(KxRecordsStats)]
        lib.kx_split_records_escaped.argtypes = [vp, sz, ctypes.c_uint8, ctypes.c_int, ctypes.c_uint8, u32, u64, vp, u64,
                                                 ctypes.POINTER(u64), ctypes.POINTER(u32), vp]
        lib.kx_run_records_fd_escaped.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint8, ctypes.c_int, ctypes.c_uint8,
                                                  ctypes.c_int, ctypes.POINTER(KxRecordsStats)]
        lib.kx_split_records_rs.argtypes = [vp, sz, ctypes.c_char_p, u32, ctypes.c_char_p, u32, u64, vp, u64, ctypes.POINTER(u64),
                                            ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(u32), ctypes.POINTER(u64), vp]
        lib.kx_run_records_fd_rs.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, u32, ctypes.c_int,
                                             ctypes.POINTER(KxRecordsStats)]
        lib.kx_shard_begin.argtypes = [vp, u32, vp, sz, ctypes.c_int, ctypes.c_int, vp, ctypes.POINTER(vp)]
        lib.kx_shard_forward.argtypes = [vp, ctypes.POINTER(KxFwdSummary)]
        lib.kx_shard_fix_head.argtypes = [vp, u32, ctypes.POINTER(KxFwdSummary)]
        lib.kx_shard_backward.argtypes = [vp, ctypes.POINTER(KxBwdSummary)]
        lib.kx_shard_resolve.argtypes = [vp, u32, ctypes.POINTER(u64)]
        lib.kx_shard_emit.argtypes = [vp, vp, sz]
        lib.kx_shard_stats.argtypes = [vp, ctypes.POINTER(KxStats)]
        lib.kx_shard_end.argtypes = [vp]
        lib.kx_run_sharded.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, sz, vp, sz, ctypes.POINTER(KxShardedResult), vp]
        lib.kx_comm_unique_id.argtypes = [ctypes.c_char_p]
        lib.kx_comm_init.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
        lib.kx_comm_free.argtypes = [vp]
        lib.kx_group_create.argtypes = [ctypes.c_int]
        lib.kx_group_create.restype = vp
        lib.kx_group_free.argtypes = [vp]
        lib.kx_group_join.argtypes = [vp, ctypes.c_int]
        lib.kx_group_join.restype = vp
        lib.kx_group_leave.argtypes = [vp]
        _kxhip = lib
    return _kxhip


# ------------------------------------------------------------------ compile
def compile_source(source, name="<memory>", opt=3):
    """Kleenex source text → KXP blob (bytes).  Mirrors ``kexc compile --opt N`` (direct mode)."""
    lib = load_compiler()
    if isinstance(source, str):
        source = source.encode("utf-8")
    blob = ctypes.c_void_p()
    n = ctypes.c_size_t()
    rc = lib.kexc_compile(source, len(source), name.encode(), opt, ctypes.byref(blob), ctypes.byref(n))
    if rc:
        raise CompileError(lib.kexc_last_error().decode("utf-8", "replace"))
    try:
        return ctypes.string_at(blob, n.value)
    finally:
        lib.kexc_free(blob)


APPROX_METRICS = ("LCS", "Hamming", "Levenshtein")          # --metric (Options.hs:103-115), in kexc_compile_approx's numbering
APPROX_MODES = ("correction", "matching", "explicit")         # --approxmode (Options.hs:117-128)


def compile_flags(source, name="<memory>", opt=3, la=False, regex=False, metric="LCS", approx_mode="correction", ite=False):
    """``kexc compile --opt N --la=BOOL`` (regex=True: ``--re``) → KXP blob.  la=True builds the reference's lookahead machine
    (word tests) first and the tables from its path form (include/kexc_api.h::kexc_compile_flags).  metric / approx_mode / ite are
    ``--metric`` / ``--approxmode`` / ``--ite``: how the source's ``t<k>`` terms are rewritten (include/kexc_approx.h)."""
    if metric not in APPROX_METRICS:
        raise CompileError('"%s" is not a valid approximation type' % metric)
    if approx_mode not in APPROX_MODES:
        raise CompileError('"%s" is not a valid approximation mode' % approx_mode)
    lib = load_compiler()
    if isinstance(source, str):
        source = source.encode("utf-8")
    blob = ctypes.c_void_p()
    n = ctypes.c_size_t()
    if regex or (metric, approx_mode, ite) == ("LCS", "correction", False):
        lib.kexc_compile_flags.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        rc = lib.kexc_compile_flags(source, len(source), name.encode(), opt, 1 if la else 0, 1 if regex else 0, ctypes.byref(blob), ctypes.byref(n))
    else:
        lib.kexc_compile_approx.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        rc = lib.kexc_compile_approx(source, len(source), name.encode(), opt, 1 if la else 0, APPROX_METRICS.index(metric),
                                     APPROX_MODES.index(approx_mode), 1 if ite else 0, ctypes.byref(blob), ctypes.byref(n))
    if rc:
        raise CompileError(lib.kexc_last_error().decode("utf-8", "replace"))
    try:
        return ctypes.string_at(blob, n.value)
    finally:
        lib.kexc_free(blob)


def dump_words(source, name="<memory>", regex=False):
    """JSON-decoded lookahead machines (``--la=true``) of a program's stages in path form (test support)."""
    import json
    lib = load_compiler()
    if isinstance(source, str):
        source = source.encode("utf-8")
    txt = ctypes.c_void_p()
    n = ctypes.c_size_t()
    lib.kexc_dump_words.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                    ctypes.POINTER(ctypes.c_size_t)]
    rc = lib.kexc_dump_words(source, len(source), name.encode(), 1 if regex else 0, ctypes.byref(txt), ctypes.byref(n))
    if rc:
        raise CompileError(lib.kexc_last_error().decode("utf-8", "replace"))
    try:
        return json.loads(ctypes.string_at(txt, n.value).decode("utf-8"))
    finally:
        lib.kexc_free(txt)


def emit_c(source, name="<memory>", opt=3):
    """``--backend=c``: reference-shaped C text for the CPU baseline."""
    lib = load_compiler()
    if isinstance(source, str):
        source = source.encode("utf-8")
    txt = ctypes.c_void_p()
    n = ctypes.c_size_t()
    rc = lib.kexc_emit_c(source, len(source), name.encode(), opt, ctypes.byref(txt), ctypes.byref(n))
    if rc:
        raise CompileError(lib.kexc_last_error().decode("utf-8", "replace"))
    try:
        return ctypes.string_at(txt, n.value).decode("utf-8")
    finally:
        lib.kexc_free(txt)


def dump_fst(source, name="<memory>"):
    """JSON-decoded nondeterministic transducers of a program (test support)."""
    import json
    lib = load_compiler()
    if isinstance(source, str):
        source = source.encode("utf-8")
    txt = ctypes.c_void_p()
    n = ctypes.c_size_t()
    lib.kexc_dump_fst.argtypes = lib.kexc_compile.argtypes[:3] + lib.kexc_compile.argtypes[4:]
    rc = lib.kexc_dump_fst(source, len(source), name.encode(), ctypes.byref(txt), ctypes.byref(n))
    if rc:
        raise CompileError(lib.kexc_last_error().decode("utf-8", "replace"))
    try:
        return json.loads(ctypes.string_at(txt, n.value).decode("utf-8"))
    finally:
        lib.kexc_free(txt)


def compile_regex(regex, name="<command line>", opt=3):
    """Regular expression → KXP blob of its bit-coder (``kexc compile --re EXPR`` / ``FILE.re``; Commands.hs:246-275)."""
    lib = load_compiler()
    if isinstance(regex, str):
        regex = regex.encode("utf-8")
    blob = ctypes.c_void_p()
    n = ctypes.c_size_t()
    lib.kexc_compile_regex.argtypes = lib.kexc_compile.argtypes
    rc = lib.kexc_compile_regex(regex, len(regex), name.encode(), opt, ctypes.byref(blob), ctypes.byref(n))
    if rc:
        raise CompileError(lib.kexc_last_error().decode("utf-8", "replace"))
    try:
        return ctypes.string_at(blob, n.value)
    finally:
        lib.kexc_free(blob)


def dump_regex_fst(regex, oracle=True):
    """JSON-decoded transducer of a regex program: its oracle machine, or (oracle=False) the transducer before `oracle`."""
    import json
    lib = load_compiler()
    if isinstance(regex, str):
        regex = regex.encode("utf-8")
    txt = ctypes.c_void_p()
    n = ctypes.c_size_t()
    lib.kexc_dump_regex_fst.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                        ctypes.POINTER(ctypes.c_size_t)]
    rc = lib.kexc_dump_regex_fst(regex, len(regex), 1 if oracle else 0, ctypes.byref(txt), ctypes.byref(n))
    if rc:
        raise CompileError(lib.kexc_last_error().decode("utf-8", "replace"))
    try:
        return json.loads(ctypes.string_at(txt, n.value).decode("utf-8"))
    finally:
        lib.kexc_free(txt)


def validate_blob(blob):
    """Structural check of a KXP blob (no device needed).  Raises EngineError with the engine's message."""
    lib = load_engine()
    blob = bytes(blob)
    if lib.kx_validate(blob, len(blob)):
        raise EngineError(lib.kx_last_error().decode("utf-8", "replace"))


def df_describe(blob, stage=0, with_image=True, cfg=None):
    """The delayed form of a stage, built on the host (no device needed): (KxDfInfo, table image bytes or None).
    cfg: a KxConfig (its load-time fields); None = what the environment's KX_DF* variables say (config_from_env)."""
    lib = load_engine()
    blob = bytes(blob)
    info = KxDfInfo()
    cfg = config_from_env() if cfg is None else cfg
    if lib.kx_df_describe_cfg(blob, len(blob), stage, ctypes.byref(cfg), ctypes.byref(info), None, 0):
        raise EngineError(lib.kx_last_error().decode("utf-8", "replace"))
    img = None
    if with_image and info.image_bytes:
        buf = ctypes.create_string_buffer(info.image_bytes)
        lib.kx_df_describe_cfg(blob, len(blob), stage, ctypes.byref(cfg), ctypes.byref(info), buf, info.image_bytes)
        img = buf.raw
    return info, img


def stage_describe(blob, stage=0, which=KX_STAGE_MAIN, cfg=None, with_image=True):
    """What the loader builds for a stage, on the host (no device needed): (KxStageInfo, bytes of allocation `which` or None if
    the stage has none).  which: KX_STAGE_MAIN / _ALT / _DELAYED / _SLOW.  cfg as for df_describe."""
    lib = load_engine()
    blob = bytes(blob)
    info = KxStageInfo(size=ctypes.sizeof(KxStageInfo))
    cfg = config_from_env() if cfg is None else cfg
    probe = ctypes.create_string_buffer(1 << 20) if with_image else None   # (most images fit: one call)
    if lib.kx_stage_describe_cfg(blob, len(blob), stage, ctypes.byref(cfg), which, ctypes.byref(info), probe, (1 << 20) if with_image else 0):
        raise EngineError(lib.kx_last_error().decode("utf-8", "replace"))
    if not with_image or not info.image_bytes:
        return info, None
    if info.image_bytes > (1 << 20):
        probe = ctypes.create_string_buffer(info.image_bytes)
        lib.kx_stage_describe_cfg(blob, len(blob), stage, ctypes.byref(cfg), which, ctypes.byref(info), probe, info.image_bytes)
    return info, probe.raw[:info.image_bytes]


def df_pending(blob, stage, state, slot, cfg=None):
    """(SST state, [copy | path-constant id << 1 per leaf, or one value]) of a product state's pending slot."""
    lib = load_engine()
    blob = bytes(blob)
    kinds = (ctypes.c_uint32 * KX_MAX_LEAVES)()
    n = ctypes.c_uint32()
    q = ctypes.c_uint32()
    cfg = config_from_env() if cfg is None else cfg
    if lib.kx_df_pending_cfg(blob, len(blob), stage, ctypes.byref(cfg), state, slot, ctypes.byref(q), kinds, ctypes.byref(n)):
        raise EngineError(lib.kx_last_error().decode("utf-8", "replace"))
    return q.value, list(kinds[:n.value])


def df_deferred(blob, stage, state, cfg=None):
    """The constants a product state still has due (merged constants, kx_delayed.h): their bytes, oldest first."""
    lib = load_engine()
    blob = bytes(blob)
    buf = ctypes.create_string_buffer(1024)
    n = ctypes.c_size_t()
    cfg = config_from_env() if cfg is None else cfg
    if lib.kx_df_deferred(blob, len(blob), stage, ctypes.byref(cfg), state, buf, 1024, ctypes.byref(n)):
        raise EngineError(lib.kx_last_error().decode("utf-8", "replace"))
    return buf.raw[:n.value]


def df_start_of_state(blob, stage, sst_state, cfg=None):
    """Handle of (state, nothing pending, nothing due) in the delayed form's table, or 0xFFFF."""
    lib = load_engine()
    blob = bytes(blob)
    h = ctypes.c_uint32()
    cfg = config_from_env() if cfg is None else cfg
    if lib.kx_df_start_of_state(blob, len(blob), stage, ctypes.byref(cfg), sst_state, ctypes.byref(h)):
        raise EngineError(lib.kx_last_error().decode("utf-8", "replace"))
    return h.value


class KexcIlProgram(ctypes.Structure):
    """include/kexc_api.h::kexc_il_program — one IL Program in table form + the path-tree annotation."""
    _u8p, _u16p, _u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint32)
    _fields_ = [("nstates", ctypes.c_uint32), ("nclasses", ctypes.c_uint32), ("init_state", ctypes.c_uint32), ("nregs", ctypes.c_uint32),
                ("class_of", _u8p), ("delta", _u16p), ("action", _u32p), ("final_action", _u32p),
                ("nactions", ctypes.c_uint32), ("action_off", _u32p), ("ops", _u32p),
                ("nconsts", ctypes.c_uint32), ("const_off", _u32p), ("const_pool", _u8p),
                ("maxleaves", ctypes.c_uint32), ("nback", ctypes.c_uint32), ("back_row", _u32p),
                ("nleaves", _u8p), ("final_leaf", _u8p), ("back", _u32p),
                ("npconsts", ctypes.c_uint32), ("pconst_off", _u32p), ("pconst_pool", _u8p), ("init_const", _u32p),
                ("has_actions", ctypes.c_uint32), ("action_regs", ctypes.c_uint32),
                ("ntables", ctypes.c_uint32), ("tbl_width", _u32p), ("tbl_data", _u8p), ("back_table", _u32p),
                ("ntests", ctypes.c_uint32), ("test_block", _u32p), ("test_target", _u32p), ("test_len", _u32p),
                ("test_preds", _u8p), ("test_back", _u32p)]


class KexcPipeline(ctypes.Structure):
    _fields_ = [("is_oracle_action", ctypes.c_int), ("nprograms", ctypes.c_uint32), ("programs", ctypes.POINTER(KexcIlProgram)),
                ("program_size", ctypes.c_uint32)]


def emit_pipeline(programs, env_info=None, out=None, srcout=None, buffer_unit_bits=8, copt=3, cc="cc", word_alignment=True,
                  oracle_action=False, info=None, program_size=None):
    """compileProgram's seam (include/kexc_api.h::kexc_emit_pipeline): `programs` is a list of dicts of numpy arrays
    (keys = the fields of kexc_il_program).  Returns the exit code; raises CompileError with the message on failure."""
    import numpy as np
    lib = load_compiler()
    keep, structs = [], (KexcIlProgram * len(programs))()
    kinds = {"class_of": np.uint8, "delta": np.uint16, "action": np.uint32, "final_action": np.uint32, "action_off": np.uint32, "ops": np.uint32,
             "const_off": np.uint32, "const_pool": np.uint8, "back_row": np.uint32, "nleaves": np.uint8, "final_leaf": np.uint8,
             "back": np.uint32, "pconst_off": np.uint32, "pconst_pool": np.uint8, "init_const": np.uint32}
    def ptr(a, dt):
        return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8 if dt == np.uint8 else ctypes.c_uint16 if dt == np.uint16 else ctypes.c_uint32))
    for st, P in zip(structs, programs):
        st.ntests = int(P.get("ntests", 0))
        if st.ntests:      # block form (--la=true): only the annotation travels, the class tables stay NULL
            for k in ("nstates", "init_state", "maxleaves", "npconsts"):
                setattr(st, k, int(P[k]))
            st.has_actions, st.action_regs = int(P.get("has_actions", 0)), int(P.get("action_regs", 0))
            for k, dt in (("nleaves", np.uint8), ("final_leaf", np.uint8), ("pconst_off", np.uint32), ("pconst_pool", np.uint8), ("init_const", np.uint32),
                          ("test_block", np.uint32), ("test_target", np.uint32), ("test_len", np.uint32), ("test_preds", np.uint8), ("test_back", np.uint32)):
                a = np.ascontiguousarray(np.asarray(P[k], dtype=dt).ravel())
                if a.size == 0:
                    a = np.zeros(1, dtype=dt)
                keep.append(a)
                setattr(st, k, ptr(a, dt))
            continue
        for k in ("nstates", "nclasses", "init_state", "nregs", "nactions", "nconsts", "maxleaves", "nback", "npconsts"):
            setattr(st, k, int(P[k]))
        st.has_actions, st.action_regs = int(P.get("has_actions", 0)), int(P.get("action_regs", 0))
        st.ntables = int(P.get("ntables", 0))
        for k, dt in (("tbl_width", np.uint32), ("tbl_data", np.uint8), ("back_table", np.uint32)) if st.ntables else ():
            a = np.ascontiguousarray(np.asarray(P[k], dtype=dt).ravel())
            keep.append(a)
            setattr(st, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8 if dt == np.uint8 else ctypes.c_uint32)))
        for k, dt in kinds.items():
            a = np.ascontiguousarray(np.asarray(P[k], dtype=dt).ravel())
            if a.size == 0:
                a = np.zeros(1, dtype=dt)
            keep.append(a)
            setattr(st, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8 if dt == np.uint8 else ctypes.c_uint16 if dt == np.uint16 else ctypes.c_uint32)))
    pl = KexcPipeline(1 if oracle_action else 0, len(programs), structs, ctypes.sizeof(KexcIlProgram) if program_size is None else program_size)
    CB = ctypes.CFUNCTYPE(None, ctypes.c_char_p, ctypes.c_void_p)
    cb = CB((lambda line, ctx: info(line.decode())) if info else (lambda line, ctx: None))
    lib.kexc_emit_pipeline_v2.argtypes = [ctypes.c_int, ctypes.c_int, CB, ctypes.c_void_p, ctypes.POINTER(KexcPipeline), ctypes.c_char_p,
                                       ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
    enc = lambda x: None if x is None else str(x).encode()
    rc = lib.kexc_emit_pipeline_v2(buffer_unit_bits, copt, cb, None, ctypes.byref(pl), enc(env_info), enc(cc), enc(out), enc(srcout), 1 if word_alignment else 0)
    if rc:
        raise CompileError(lib.kexc_last_error().decode("utf-8", "replace"))
    return rc


def program_path(name):
    p = os.path.join(PROGRAM_DIR, name if name.endswith(".kex") else name + ".kex")
    if not os.path.exists(p):
        raise FileNotFoundError(p)
    return p


def compile_file(path, opt=3):
    if not os.path.exists(path):
        path = program_path(path)
    with open(path, "rb") as f:
        return compile_source(f.read(), os.path.basename(path), opt)


# ------------------------------------------------------------------- engine
class Program:
    """A compiled Kleenex program loaded on the current HIP device."""

    def __init__(self, blob, segment_bytes=0, block_threads=0, collect_timing=False, window_bytes=0, config=None):
        """config: a KxConfig; None = the environment's KX_* variables mapped onto one (config_from_env) — the library itself reads
        none of them."""
        self._lib = load_engine()
        self._h = ctypes.c_void_p()
        self._blob = bytes(blob)
        self._cfg = config_from_env() if config is None else config
        self._cfg.segment_bytes, self._cfg.block_threads = segment_bytes, block_threads
        self._cfg.collect_timing, self._cfg.window_bytes = 1 if collect_timing else 0, window_bytes
        rc = self._lib.kx_load_config(self._blob, len(self._blob), ctypes.byref(self._cfg), ctypes.byref(self._h))
        if rc:
            raise EngineError(self._err())
        self.last_stats = None

    @classmethod
    def from_file(cls, path, opt=3, **kw):
        return cls(compile_file(path, opt), **kw)

    @classmethod
    def from_source(cls, source, opt=3, **kw):
        return cls(compile_source(source, opt=opt), **kw)

    def _err(self):
        return self._lib.kx_last_error().decode("utf-8", "replace")

    def configure(self, segment_bytes=0, block_threads=0, collect_timing=False, window_bytes=0, **fields):
        """Run-time fields (kx_set_config); a load-time field in `fields` that differs from the loaded program's is refused."""
        cfg = self._cfg
        cfg.segment_bytes, cfg.block_threads = segment_bytes, block_threads
        cfg.collect_timing, cfg.window_bytes = 1 if collect_timing else 0, window_bytes
        for k, v in fields.items():
            setattr(cfg, k, v)
        if self._lib.kx_set_config(self._h, ctypes.byref(cfg)):
            raise EngineError(self._err())

    def reset_delayed_form(self, stage=0):
        self._lib.kx_stage_reset_delayed_form(self._h, stage)

    @property
    def num_stages(self):
        return self._lib.kx_num_stages(self._h)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.kx_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, stats):
        self.last_stats = stats
        if rc == 1:
            raise MatchError(stats.fail_pos, stats.fail_stage)
        if rc:
            raise EngineError(self._err())

    def run_host(self, data):
        """bytes → bytes through H2D / engine / D2H."""
        data = bytes(data)
        out = ctypes.c_void_p()
        n = ctypes.c_size_t()
        stats = KxStats()
        rc = self._lib.kx_run_host(self._h, data, len(data), ctypes.byref(out), ctypes.byref(n), ctypes.byref(stats))
        try:
            self._check(rc, stats)
            return ctypes.string_at(out, n.value)
        finally:
            if out.value:
                self._lib.kx_host_free(out)

    def run_device(self, d_in, n, d_out, cap, stream=None):
        """Raw device pointers (ints).  Returns the output length; raises MatchError on rejection."""
        ol = ctypes.c_size_t()
        stats = KxStats()
        rc = self._lib.kx_run_device(self._h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out), cap,
                                     ctypes.byref(ol), ctypes.byref(stats), ctypes.c_void_p(stream or 0))
        if rc == -3:
            self.last_stats = stats
            raise EngineError("output buffer too small: need %d bytes" % ol.value)
        self._check(rc, stats)
        return ol.value

    def run_tensor(self, t, out=None):
        """torch uint8 CUDA tensor → torch uint8 CUDA tensor (device-resident both ends).
        out=: the caller's buffer (include/kxhip.h, kx_run_device).  Its address is 16-byte aligned (EngineError otherwise; a program whose
        last stage has register actions takes any address); nothing outside out[0, result length) is written, whatever out.numel() is;
        on a MatchError and on "output buffer too small" `out` is untouched.  `t` may have any alignment, is never written, and no byte
        outside t[0, n) influences the result."""
        import torch
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
        n = t.numel()
        if out is None:
            out = torch.empty(self.out_capacity(n), dtype=torch.uint8, device=t.device)
        stream = torch.cuda.current_stream(t.device).cuda_stream
        ol = self.run_device(t.data_ptr(), n, out.data_ptr(), out.numel(), stream)
        return out[:ol]

    def run_batch_tensor(self, values, offsets, out=None, trim=0, last_whole=False, suffix=b""):
        """Batched run (kx_run_batch): document i is values[offsets[i]:offsets[i+1]], each a whole input of the program.
        values: CUDA uint8 tensor (any start address); offsets: int64 tensor of n_docs + 1 non-decreasing entries (on the
        device; a host tensor is checked here and copied).  Runs on the current stream; without `out` the output is sized
        by the capacity query (one more pass of everything but the placing).  Returns the device tensors
        (out_values, out_offsets, status, fail_pos, fail_stage): document i's output is out_values[out_offsets[i]:out_offsets[i+1]]
        where status[i] == 0; status 1 = rejected at stage fail_stage[i], symbol fail_pos[i] (its range is empty).
        With `trim`, `last_whole` or `suffix` the batch is framed (kx_run_batch_framed): document i is
        values[offsets[i]:offsets[i+1] - trim] (the last one whole with last_whole), and the 0 to 8 `suffix` bytes end the output
        range of every accepted document (chomp_records_model)."""
        _check_batch_args(values, offsets)
        trim = _check_trim(trim)
        if not isinstance(last_whole, bool):
            raise TypeError("run_batch_tensor: last_whole must be True or False, not %s" % type(last_whole).__name__)
        if not isinstance(suffix, (bytes, bytearray)):
            raise TypeError("run_batch_tensor: suffix must be bytes of length 0 to 8, not %s" % type(suffix).__name__)
        if len(suffix) > 8:
            raise ValueError("run_batch_tensor: suffix must be 0 to 8 bytes, not %d" % len(suffix))
        frame = None
        if trim or last_whole or suffix:
            frame = KxBatchFrame(trim=trim, last_whole=1 if last_whole else 0, suffix_len=len(suffix))
            frame.suffix[:len(suffix)] = bytes(suffix)
        return self._run_batch_call("run_batch_tensor", values, offsets, out, frame, None)

    def _run_batch_call(self, what, values, offsets, out, frame, fields, codec=None, words=False, proj=None, identity=False, keys=None):
        """The device part of run_batch_tensor (`frame`: a KxBatchFrame or None), run_batch_fields_tensor (`fields`: a
        KxBatchFields), run_batch_field_list_tensor (`fields`: a KxBatchFieldList, which adds the fail_field tensor to the
        result), run_batch_field_values_tensor (the same with `codec`: a KxFieldCodec) and run_batch_field_words_tensor (`words`;
        `codec` a KxFieldCodec or None) and run_batch_field_project_tensor (`proj`: a KxFieldProject, whose flags say whether the
        fields are words; with `identity` kx_run_batch_field_header) and run_batch_field_keys_tensor (`keys`: a KxFieldKeys; `codec`
        and `proj` or None): the checks that need the tensors' device, the buffers, the size query and the call."""
        import torch
        if not values.is_cuda:
            raise EngineError("%s: values must be on a HIP device (there is no CPU fallback)" % what)
        dev = values.device
        if not offsets.is_cuda:
            offsets = offsets.to(dev)
        elif offsets.numel() > 1:
            lo, hi = offsets[[0, -1]].tolist()    # the order is checked by the engine, on the device; the range here
            if lo < 0 or hi > values.numel():
                raise ValueError("batch offsets: outside the values buffer [0, %d]" % values.numel())
        offsets = offsets.contiguous()
        n = offsets.numel() - 1
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        docs = torch.empty((max(n, 1), 2), dtype=torch.int64, device=dev)
        listed = isinstance(fields, KxBatchFieldList)
        ffield = torch.zeros(max(n, 1), dtype=torch.int32, device=dev) if listed else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        vptr = values.data_ptr() if values.numel() else None

        def call(buf):
            ol = ctypes.c_size_t()
            st = KxBatchStats()
            bptr = ctypes.c_void_p(buf.data_ptr() if buf is not None and buf.numel() else None)
            bcap = buf.numel() if buf is not None else 0
            if keys is not None:
                rc = self._lib.kx_run_batch_field_keys(self._h, ctypes.c_void_p(vptr), ctypes.c_void_p(offsets.data_ptr()), n,
                                                       ctypes.byref(fields), ctypes.byref(keys), ctypes.byref(codec) if codec is not None else None,
                                                       ctypes.byref(proj) if proj is not None else None, bptr, bcap,
                                                       ctypes.c_void_p(out_off.data_ptr()), ctypes.c_void_p(docs.data_ptr()),
                                                       ctypes.c_void_p(ffield.data_ptr()), ctypes.byref(ol), ctypes.byref(st),
                                                       ctypes.c_void_p(stream))
            elif proj is not None:
                entry = self._lib.kx_run_batch_field_header if identity else self._lib.kx_run_batch_field_project
                rc = entry(self._h, ctypes.c_void_p(vptr), ctypes.c_void_p(offsets.data_ptr()), n,
                           ctypes.byref(fields), ctypes.byref(codec) if codec is not None else None, ctypes.byref(proj), bptr, bcap,
                           ctypes.c_void_p(out_off.data_ptr()), ctypes.c_void_p(docs.data_ptr()), ctypes.c_void_p(ffield.data_ptr()),
                           ctypes.byref(ol), ctypes.byref(st), ctypes.c_void_p(stream))
            elif words:
                rc = self._lib.kx_run_batch_field_words(self._h, ctypes.c_void_p(vptr), ctypes.c_void_p(offsets.data_ptr()), n,
                                                        ctypes.byref(fields), ctypes.byref(codec) if codec is not None else None, bptr,
                                                        bcap, ctypes.c_void_p(out_off.data_ptr()), ctypes.c_void_p(docs.data_ptr()),
                                                        ctypes.c_void_p(ffield.data_ptr()), ctypes.byref(ol), ctypes.byref(st),
                                                        ctypes.c_void_p(stream))
            elif codec is not None:
                rc = self._lib.kx_run_batch_field_values(self._h, ctypes.c_void_p(vptr), ctypes.c_void_p(offsets.data_ptr()), n,
                                                         ctypes.byref(fields), ctypes.byref(codec), bptr, bcap,
                                                         ctypes.c_void_p(out_off.data_ptr()), ctypes.c_void_p(docs.data_ptr()),
                                                         ctypes.c_void_p(ffield.data_ptr()), ctypes.byref(ol), ctypes.byref(st),
                                                         ctypes.c_void_p(stream))
            elif listed:
                rc = self._lib.kx_run_batch_field_list(self._h, ctypes.c_void_p(vptr), ctypes.c_void_p(offsets.data_ptr()), n,
                                                       ctypes.byref(fields), bptr, bcap, ctypes.c_void_p(out_off.data_ptr()),
                                                       ctypes.c_void_p(docs.data_ptr()), ctypes.c_void_p(ffield.data_ptr()),
                                                       ctypes.byref(ol), ctypes.byref(st), ctypes.c_void_p(stream))
            elif fields is not None:
                rc = self._lib.kx_run_batch_fields(self._h, ctypes.c_void_p(vptr), ctypes.c_void_p(offsets.data_ptr()), n,
                                                   ctypes.byref(fields), bptr, bcap, ctypes.c_void_p(out_off.data_ptr()),
                                                   ctypes.c_void_p(docs.data_ptr()), ctypes.byref(ol), ctypes.byref(st),
                                                   ctypes.c_void_p(stream))
            elif frame is None:
                rc = self._lib.kx_run_batch(self._h, ctypes.c_void_p(vptr), ctypes.c_void_p(offsets.data_ptr()), n, bptr, bcap,
                                            ctypes.c_void_p(out_off.data_ptr()), ctypes.c_void_p(docs.data_ptr()), ctypes.byref(ol),
                                            ctypes.byref(st), ctypes.c_void_p(stream))
            else:
                rc = self._lib.kx_run_batch_framed(self._h, ctypes.c_void_p(vptr), ctypes.c_void_p(offsets.data_ptr()), n,
                                                   ctypes.byref(frame), bptr, bcap, ctypes.c_void_p(out_off.data_ptr()),
                                                   ctypes.c_void_p(docs.data_ptr()), ctypes.byref(ol), ctypes.byref(st),
                                                   ctypes.c_void_p(stream))
            self.last_batch_stats = st
            return rc, ol.value

        if out is None:
            rc, need = call(None)
            if rc == -3:
                out = torch.empty(need, dtype=torch.uint8, device=dev)
                rc, need = call(out)
            elif rc in (0, 1):
                out = torch.empty(0, dtype=torch.uint8, device=dev)
        else:
            if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()):
                raise TypeError("%s: out must be a contiguous CUDA uint8 tensor" % what)
            rc, need = call(out)
        if rc == -3:
            raise EngineError("output buffer too small: need %d bytes" % need)
        if rc not in (0, 1):
            raise EngineError(self._err())
        d = docs[:n]
        res = out[:need], out_off, (d[:, 1] & 0xFFFFFFFF).to(torch.int32), d[:, 0], (d[:, 1] >> 32).to(torch.int32)
        return res + ((ffield[:n].to(torch.int64) & 0xFFFFFFFF),) if listed else res

    def run_batch_fields_tensor(self, values, offsets, field, fs=b"\t", quote=None, escape=None, sep_len=0, last_whole=False,
                                keep_sep=True, suffix=b"", out=None):
        """Field mode (kx_run_batch_fields): run_batch_tensor where the program runs on field `field` (from 1) of record i =
        values[offsets[i]:offsets[i+1]] and the rest of the record is copied around its output (field_records_model): an accepted
        record's output is prefix + program output + rest, then its separator (its last `sep_len` bytes; the last record has none
        with `last_whole`) if `keep_sep`, then the 0 to 8 `suffix` bytes.  Returns the five tensors of run_batch_tensor; status 2 =
        the record has fewer fields, fail_pos[i] of them."""
        _check_batch_args(values, offsets)
        field, sep_len = _check_field(field), _check_sep_len(sep_len)
        f = _check_fs(fs, quote, escape)
        q = -1 if quote is None else _one_byte(quote, "quote character")
        e = -1 if escape is None else _one_byte(escape, "escape character")
        if q >= 0 and q == e:
            raise ValueError("escape character: %r is also the quote character" % bytes([e]))
        for name, v in (("last_whole", last_whole), ("keep_sep", keep_sep)):
            if not isinstance(v, bool):
                raise TypeError("run_batch_fields_tensor: %s must be True or False, not %s" % (name, type(v).__name__))
        if not isinstance(suffix, (bytes, bytearray)):
            raise TypeError("run_batch_fields_tensor: suffix must be bytes of length 0 to 8, not %s" % type(suffix).__name__)
        if len(suffix) > 8:
            raise ValueError("run_batch_fields_tensor: suffix must be 0 to 8 bytes, not %d" % len(suffix))
        spec = KxBatchFields(size=ctypes.sizeof(KxBatchFields), field=field, fs=f, quote=q, escape=e, sep_len=sep_len,
                             last_whole=1 if last_whole else 0, keep_sep=1 if keep_sep else 0, suffix_len=len(suffix))
        spec.suffix[:len(suffix)] = bytes(suffix)
        return self._run_batch_call("run_batch_fields_tensor", values, offsets, out, None, spec)

    def run_batch_field_list_tensor(self, values, offsets, ranges, fs=b"\t", quote=None, escape=None, sep_len=0, last_whole=False,
                                    keep_sep=True, suffix=b"", out=None):
        """Field mode with a list (kx_run_batch_field_list): run_batch_fields_tensor where the program runs on every field of
        `ranges` (a parse_field_list result, or a sequence of ints and (lo, hi) pairs), each a whole input of its own
        (field_list_records_model).  A record with all its selected fields accepted writes its body with every one replaced by the
        program's output, then separator and suffix as there.  Returns (out, out_off, status, fail_pos, fail_stage, fail_field):
        status 1 = a field was rejected, fail_field[i] the lowest such and fail_pos[i] counted inside it; status 2 = the record
        has too few fields, fail_pos[i] of them, and fail_field[i] is the first one it lacks; fail_field 0 = accepted."""
        _check_batch_args(values, offsets)
        ranges, sep_len = _check_field_ranges(ranges), _check_sep_len(sep_len)
        f = _check_fs(fs, quote, escape)
        q = -1 if quote is None else _one_byte(quote, "quote character")
        e = -1 if escape is None else _one_byte(escape, "escape character")
        if q >= 0 and q == e:
            raise ValueError("escape character: %r is also the quote character" % bytes([e]))
        for name, v in (("last_whole", last_whole), ("keep_sep", keep_sep)):
            if not isinstance(v, bool):
                raise TypeError("run_batch_field_list_tensor: %s must be True or False, not %s" % (name, type(v).__name__))
        if not isinstance(suffix, (bytes, bytearray)):
            raise TypeError("run_batch_field_list_tensor: suffix must be bytes of length 0 to 8, not %s" % type(suffix).__name__)
        if len(suffix) > 8:
            raise ValueError("run_batch_field_list_tensor: suffix must be 0 to 8 bytes, not %d" % len(suffix))
        arr, nr = _field_range_array(ranges)
        spec = KxBatchFieldList(size=ctypes.sizeof(KxBatchFieldList), n_ranges=nr, ranges=arr, fs=f, quote=q, escape=e, sep_len=sep_len,
                                last_whole=1 if last_whole else 0, keep_sep=1 if keep_sep else 0, suffix_len=len(suffix))
        spec.suffix[:len(suffix)] = bytes(suffix)
        return self._run_batch_call("run_batch_field_list_tensor", values, offsets, out, None, spec)

    def run_batch_field_values_tensor(self, values, offsets, ranges, fs=b"\t", quote=None, escape=None, special=b"\n", sep_len=0,
                                      last_whole=False, keep_sep=True, suffix=b"", out=None):
        """Field mode on unquoted values (kx_run_batch_field_values): run_batch_field_list_tensor where the program runs on the
        VALUE of every selected field (unquote_field_model) and the field is replaced by the spelling of the program's output
        (requote_field_model, with the 0 to 8 `special` bytes).  Needs a `quote` or an `escape` byte.  Returns the six tensors of
        run_batch_field_list_tensor; fail_pos counts inside the value."""
        _check_batch_args(values, offsets)
        ranges, sep_len = _check_field_ranges(ranges), _check_sep_len(sep_len)
        f = _check_fs(fs, quote, escape)
        q, e, special = _check_codec("run_batch_field_values_tensor", quote, escape, special)
        for name, v in (("last_whole", last_whole), ("keep_sep", keep_sep)):
            if not isinstance(v, bool):
                raise TypeError("run_batch_field_values_tensor: %s must be True or False, not %s" % (name, type(v).__name__))
        if not isinstance(suffix, (bytes, bytearray)):
            raise TypeError("run_batch_field_values_tensor: suffix must be bytes of length 0 to 8, not %s" % type(suffix).__name__)
        if len(suffix) > 8:
            raise ValueError("run_batch_field_values_tensor: suffix must be 0 to 8 bytes, not %d" % len(suffix))
        arr, nr = _field_range_array(ranges)
        spec = KxBatchFieldList(size=ctypes.sizeof(KxBatchFieldList), n_ranges=nr, ranges=arr, fs=f, quote=-1 if q is None else q,
                                escape=-1 if e is None else e, sep_len=sep_len, last_whole=1 if last_whole else 0,
                                keep_sep=1 if keep_sep else 0, suffix_len=len(suffix))
        spec.suffix[:len(suffix)] = bytes(suffix)
        codec = KxFieldCodec(size=ctypes.sizeof(KxFieldCodec), n_special=len(special))
        codec.special[:len(special)] = special
        return self._run_batch_call("run_batch_field_values_tensor", values, offsets, out, None, spec, codec)

    def run_batch_field_words_tensor(self, values, offsets, ranges, quote=None, escape=None, unquote=False, special=b"\n", sep_len=0,
                                     last_whole=False, keep_sep=True, suffix=b"", out=None):
        """Field mode on words (kx_run_batch_field_words): run_batch_field_list_tensor where the fields of a record are the words
        between its live blanks — spaces and tabs — as blank_field_list_records_model has them; every blank is copied as it is.
        With `unquote` (needs a `quote` or an `escape` byte) the program runs on the VALUE of every selected word and the word is
        replaced by the spelling of the program's output: requote_field_model with fs = the space and the 0 to 7 `special` bytes
        plus the tab.  Returns the six tensors of run_batch_field_list_tensor; status 2 = the record has too few words,
        fail_pos[i] of them (0 for a record without any)."""
        what = "run_batch_field_words_tensor"
        _check_batch_args(values, offsets)
        ranges, sep_len = _check_field_ranges(ranges), _check_sep_len(sep_len)
        if not isinstance(unquote, bool):
            raise TypeError("%s: unquote must be True or False, not %s" % (what, type(unquote).__name__))
        codec = None
        if unquote:
            q, e, special = _check_codec(what, quote, escape, special)
            if len(special) > 7:
                raise ValueError("%s: special must be 0 to 7 bytes (the tab is added), not %d" % (what, len(special)))
            _check_not_blank(quote, escape, special=special)
            codec = KxFieldCodec(size=ctypes.sizeof(KxFieldCodec), n_special=len(special))
            codec.special[:len(special)] = special
        else:
            _check_not_blank(quote, escape)
            q = None if quote is None else _one_byte(quote, "quote character")
            e = None if escape is None else _one_byte(escape, "escape character")
            if q is not None and q == e:
                raise ValueError("escape character: %r is also the quote character" % bytes([e]))
        for name, v in (("last_whole", last_whole), ("keep_sep", keep_sep)):
            if not isinstance(v, bool):
                raise TypeError("%s: %s must be True or False, not %s" % (what, name, type(v).__name__))
        if not isinstance(suffix, (bytes, bytearray)):
            raise TypeError("%s: suffix must be bytes of length 0 to 8, not %s" % (what, type(suffix).__name__))
        if len(suffix) > 8:
            raise ValueError("%s: suffix must be 0 to 8 bytes, not %d" % (what, len(suffix)))
        arr, nr = _field_range_array(ranges)
        spec = KxBatchFieldList(size=ctypes.sizeof(KxBatchFieldList), n_ranges=nr, ranges=arr, fs=0, quote=-1 if q is None else q,
                                escape=-1 if e is None else e, sep_len=sep_len, last_whole=1 if last_whole else 0,
                                keep_sep=1 if keep_sep else 0, suffix_len=len(suffix))
        spec.suffix[:len(suffix)] = bytes(suffix)
        return self._run_batch_call(what, values, offsets, out, None, spec, codec, words=True)

    def run_batch_field_header_tensor(self, values, offsets, items, ofs, fs=b"\t", blanks=False, quote=None, escape=None, unquote=False,
                                      special=b"\n", sep_len=0, last_whole=False, keep_sep=True, suffix=b"", out=None):
        """run_batch_field_project_tensor with the identity in the program's place (kx_run_batch_field_header): the route of a
        header record under `only=`.  Every record with enough fields writes its selected fields themselves — with `unquote` the
        spelling of each one's value, requote_field_model(unquote_field_model(cell), …) — in the written order; no record is
        rejected by the program."""
        return self.run_batch_field_project_tensor(values, offsets, items, ofs, fs, blanks, quote, escape, unquote, special, sep_len,
                                                   last_whole, keep_sep, suffix, out, _identity=True)

    def run_batch_field_project_tensor(self, values, offsets, items, ofs, fs=b"\t", blanks=False, quote=None, escape=None, unquote=False,
                                       special=b"\n", sep_len=0, last_whole=False, keep_sep=True, suffix=b"", out=None, _identity=False):
        """Field mode, projected (kx_run_batch_field_project, project_records_model): the program runs once on every field of the
        union of `items` (a parse_field_order result, or 1 to 16 ints and (lo, hi) pairs in any order), as
        run_batch_field_list_tensor runs it — with `blanks` on the words, as run_batch_field_words_tensor (`fs` is then not used);
        with `unquote` on the values, as run_batch_field_values_tensor — and an accepted record writes only the outputs (with
        `unquote` their spellings, which protect the one byte of `ofs` in place of `fs`), item by item in the written order, joined
        by the 0 to 8 bytes `ofs`, then separator and suffix as there.  Returns the six tensors of run_batch_field_list_tensor;
        fail_field is the lowest rejected field number whatever the order."""
        what = "run_batch_field_header_tensor" if _identity else "run_batch_field_project_tensor"
        _check_batch_args(values, offsets)
        (items, ranges), sep_len, ofs = _check_field_items(items), _check_sep_len(sep_len), _check_ofs(ofs)
        for name, v in (("blanks", blanks), ("unquote", unquote), ("last_whole", last_whole), ("keep_sep", keep_sep)):
            if not isinstance(v, bool):
                raise TypeError("%s: %s must be True or False, not %s" % (what, name, type(v).__name__))
        f = 0 if blanks else _check_fs(fs, quote, escape)
        codec = None
        if unquote:
            q, e, special = _check_codec(what, quote, escape, special)
            if blanks and len(special) > 7:
                raise ValueError("%s: special must be 0 to 7 bytes (the tab is added), not %d" % (what, len(special)))
            _check_ofs_codec(what, ofs, q, e, special + (b"\t" if blanks else b""))
            codec = KxFieldCodec(size=ctypes.sizeof(KxFieldCodec), n_special=len(special))
            codec.special[:len(special)] = special
        else:
            q = None if quote is None else _one_byte(quote, "quote character")
            e = None if escape is None else _one_byte(escape, "escape character")
            if q is not None and q == e:
                raise ValueError("escape character: %r is also the quote character" % bytes([e]))
        if blanks:
            _check_not_blank(quote, escape, special=special if unquote else b"")
        if not isinstance(suffix, (bytes, bytearray)):
            raise TypeError("%s: suffix must be bytes of length 0 to 8, not %s" % (what, type(suffix).__name__))
        if len(suffix) > 8:
            raise ValueError("%s: suffix must be 0 to 8 bytes, not %d" % (what, len(suffix)))
        arr, nr = _field_range_array(ranges)
        spec = KxBatchFieldList(size=ctypes.sizeof(KxBatchFieldList), n_ranges=nr, ranges=arr, fs=f, quote=-1 if q is None else q,
                                escape=-1 if e is None else e, sep_len=sep_len, last_whole=1 if last_whole else 0,
                                keep_sep=1 if keep_sep else 0, suffix_len=len(suffix))
        spec.suffix[:len(suffix)] = bytes(suffix)
        iarr, ni = _field_item_array(items)
        proj = KxFieldProject(size=ctypes.sizeof(KxFieldProject), n_items=ni, items=iarr, ofs_len=len(ofs),
                              flags=KX_PROJECT_WORDS if blanks else 0)
        proj.ofs[:len(ofs)] = ofs
        return self._run_batch_call(what, values, offsets, out, None, spec, codec, proj=proj, identity=_identity)

    def run_batch_field_keys_tensor(self, values, offsets, names, kv=b"=", fs=b"\t", blanks=False, quote=None, escape=None, optional=(),
                                    unquote=False, special=b"\n", only=None, ofs=None, sep_len=0, last_whole=False, keep_sep=True, suffix=b"",
                                    out=None):
        """Field mode by key (kx_run_batch_field_keys, keyed_records_model): the fields of record i — cut by the live `fs` bytes, or
        with `blanks` into words — are key `kv` value pairs, and the program runs on the value of the first field whose key is each
        of the bytes `names` (distinct, 1 to 16), each a whole input of its own; with `unquote` on its unquote_field_model value,
        and the spelling of the output is spliced (requote_field_model with the `special` bytes).  A record that lacks a name not in
        `optional` has status 2, fail_pos[i] = the mask of the names it has and fail_field[i] = 1 + the index of the first name it
        lacks; a rejected value gives status 1 and fail_field[i] = 1 + the index of its name.  An accepted record writes its body with
        every selected value replaced, then separator and suffix as run_batch_field_list_tensor; with `only` (a sequence of indices
        into names, 1 to 16, in any order, repeats allowed) it writes the outputs of those names alone, joined by the 0 to 8 bytes
        `ofs` — a name the record lacks writes nothing.  Returns the six tensors of run_batch_field_list_tensor."""
        what = "run_batch_field_keys_tensor"
        _check_batch_args(values, offsets)
        for name, v in (("blanks", blanks), ("unquote", unquote), ("last_whole", last_whole), ("keep_sep", keep_sep)):
            if not isinstance(v, bool):
                raise TypeError("%s: %s must be True or False, not %s" % (what, name, type(v).__name__))
        sep_len = _check_sep_len(sep_len)
        given = list(names)
        names, mask, _, c = _check_field_keys(what, given, optional, kv, None if blanks else fs, blanks, quote, escape)
        if len(names) != len(given):
            raise ValueError("%s: names are distinct" % what)
        f = 0 if blanks else _check_fs(fs, quote, escape)
        codec = proj = None
        if only is not None:
            only = [int(t) for t in only]
            if not 1 <= len(only) <= FIELD_ITEMS_MAX or not all(0 <= t < len(names) for t in only):
                raise ValueError("%s: only: 1 to %d indices into names" % (what, FIELD_ITEMS_MAX))
            ofs = _check_ofs((b" " if blanks else bytes([f])) if ofs is None else ofs)
        elif ofs is not None:
            raise ValueError("%s: ofs= needs only=" % what)
        if unquote:
            q, e, special = _check_codec(what, quote, escape, special)
            if blanks and len(special) > 7:
                raise ValueError("%s: special must be 0 to 7 bytes (the tab is added), not %d" % (what, len(special)))
            if only is not None:
                _check_ofs_codec(what, ofs, q, e, special + (b"\t" if blanks else b""))
            codec = KxFieldCodec(size=ctypes.sizeof(KxFieldCodec), n_special=len(special))
            codec.special[:len(special)] = special
        else:
            q = None if quote is None else _one_byte(quote, "quote character")
            e = None if escape is None else _one_byte(escape, "escape character")
            if q is not None and q == e:
                raise ValueError("escape character: %r is also the quote character" % bytes([e]))
        if blanks:
            _check_not_blank(quote, escape, special=special if unquote else b"")
        if not isinstance(suffix, (bytes, bytearray)):
            raise TypeError("%s: suffix must be bytes of length 0 to 8, not %s" % (what, type(suffix).__name__))
        if len(suffix) > 8:
            raise ValueError("%s: suffix must be 0 to 8 bytes, not %d" % (what, len(suffix)))
        spec = KxBatchFieldList(size=ctypes.sizeof(KxBatchFieldList), n_ranges=0, fs=f, quote=-1 if q is None else q,
                                escape=-1 if e is None else e, sep_len=sep_len, last_whole=1 if last_whole else 0,
                                keep_sep=1 if keep_sep else 0, suffix_len=len(suffix))
        spec.suffix[:len(suffix)] = bytes(suffix)
        keys = field_keys_struct(names, mask, c, KX_KEYS_WORDS if blanks else 0)
        if only is not None:
            iarr, ni = _field_item_array([(0, t) for t in only])
            proj = KxFieldProject(size=ctypes.sizeof(KxFieldProject), n_items=ni, items=iarr, ofs_len=len(ofs),
                                  flags=KX_PROJECT_WORDS if blanks else 0)
            proj.ofs[:len(ofs)] = ofs
        return self._run_batch_call(what, values, offsets, out, None, spec, codec, proj=proj, keys=keys)

    def fields_kernel_stats(self):
        """kx_fields_stats: HIP-event times of field mode's own kernels, summed over this program's calls (collect_timing)."""
        st = KxFieldsKernelStats()
        if self._lib.kx_fields_stats(self._h, ctypes.byref(st)):
            raise EngineError(self._err())
        return st.as_dict()

    def run_batch(self, docs, device=None):
        """Convenience form of run_batch_tensor: a list of bytes → a list holding, per document, its output bytes or a
        MatchError (pos, stage)."""
        import torch
        values, offs = pack_batch(docs)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        v = torch.frombuffer(bytearray(values), dtype=torch.uint8).to(dev) if values else torch.empty(0, dtype=torch.uint8, device=dev)
        o = torch.tensor(offs, dtype=torch.int64).to(dev)
        out, ooff, status, fpos, fstage = self.run_batch_tensor(v, o)
        torch.cuda.synchronize(dev)
        ob = out.cpu().numpy().tobytes()
        ooff, status, fpos, fstage = ooff.tolist(), status.tolist(), fpos.tolist(), fstage.tolist()
        res = []
        for i in range(len(offs) - 1):
            res.append(MatchError(fpos[i], fstage[i]) if status[i] else ob[ooff[i]:ooff[i + 1]])
        return res

    @contextlib.contextmanager
    def _batch_actions_for_call(self, batch_actions):
        """kx_config::batch_actions for one call of record mode, as the produced binary sets it for --records: True turns the
        batch replay on unless the program's configuration says 1 (the route) explicitly; False asks for the route."""
        old = self._cfg.batch_actions
        new = (old or 2) if batch_actions else 1
        if new != old:
            self._cfg.batch_actions = new
            if self._lib.kx_set_config(self._h, ctypes.byref(self._cfg)):
                self._cfg.batch_actions = old
                raise EngineError(self._err())
        try:
            yield
        finally:
            if new != old:
                self._cfg.batch_actions = old
                self._lib.kx_set_config(self._h, ctypes.byref(self._cfg))

    @staticmethod
    def _check_unquote(what, unquote, field, fields, quote, escape):
        """The `unquote=` keyword of record mode: with `field` or `fields`, and with a `quote` or an `escape` → (field, fields),
        where with `unquote` a `field=K` has become the list K-K."""
        if not isinstance(unquote, bool):
            raise TypeError("%s: unquote must be True or False, not %s" % (what, type(unquote).__name__))
        if not unquote:
            return field, fields
        if field is None and fields is None:
            raise ValueError("%s: unquote= needs field= or fields=" % what)
        if quote is None and escape is None:
            raise ValueError("%s: unquote= needs quote= or escape=" % what)
        if field is not None and fields is None:
            return None, [_check_field(field)]
        return field, fields

    @staticmethod
    def _check_blanks(what, blanks, field, fields, fs, sep, quote, escape, rs):
        """The `blanks=` keyword of record mode: with `field` or `fields`, without an `fs`, and with a one-byte record separator,
        a quote and an escape byte that are no blanks → (field, fields, fs), where with `blanks` a `field=K` has become the list
        K-K; without it `fs` has its default, a tab."""
        if not isinstance(blanks, bool):
            raise TypeError("%s: blanks must be True or False, not %s" % (what, type(blanks).__name__))
        if not blanks:
            return field, fields, b"\t" if fs is None else fs
        if fs is not None:
            raise ValueError("%s: blanks= cannot be combined with fs=" % what)
        if field is None and fields is None:
            raise ValueError("%s: blanks= needs field= or fields=" % what)
        one = isinstance(rs, (bytes, bytearray)) and len(rs) == 1
        _check_not_blank(quote, escape, sep if rs is None else bytes(rs) if one else None)
        if field is not None and fields is None:
            return None, [_check_field(field)], None
        return field, fields, None

    @staticmethod
    def _check_only(what, only, ofs, field, fields, fs, blanks):
        """The `only=` and `ofs=` keywords of record mode: `only` with `field` or `fields`, `ofs` with `only` → (items, ofs): the
        list as written (a `field=K` is the list K-K) and the output field separator, whose default is `fs` — a tab if that is
        not given — or one space with `blanks`; (None, None) without `only`."""
        if not isinstance(only, bool):
            raise TypeError("%s: only must be True or False, not %s" % (what, type(only).__name__))
        if not only:
            if ofs is not None:
                raise ValueError("%s: ofs= needs only=" % what)
            return None, None
        if field is None and fields is None:
            raise ValueError("%s: only= needs field= or fields=" % what)
        if field is not None and fields is not None:
            raise ValueError("%s: field= and fields= exclude each other" % what)
        items, _ = _check_field_items([_check_field(field)] if fields is None else fields)
        if ofs is None:
            ofs = b" " if blanks else b"\t" if fs is None else bytes([_one_byte(fs, "field separator")])
        return items, _check_ofs(ofs)

    @staticmethod
    def _check_keys(what, keys, optional, field, fields, fs, blanks, quote, escape, sep, rs, header):
        """The `keys=` and `optional=` keywords of record mode: `keys` with `fields` (bytes names), not with `field` or `header` →
        None, or (the distinct names, optional_mask, the items as indices, C): _check_field_keys's result."""
        if keys is None:
            if optional:
                raise ValueError("%s: optional= needs keys=" % what)
            return None
        if header:
            raise ValueError("%s: keys= cannot be combined with header=" % what)
        if field is not None or fields is None:
            raise ValueError("%s: keys= needs fields=, a sequence of bytes names" % what)
        if not isinstance(blanks, bool):
            raise TypeError("%s: blanks must be True or False, not %s" % (what, type(blanks).__name__))
        if blanks and fs is not None:
            raise ValueError("%s: blanks= cannot be combined with fs=" % what)
        one = isinstance(rs, (bytes, bytearray)) and len(rs) == 1
        return _check_field_keys(what, fields, optional, keys, None if blanks else b"\t" if fs is None else fs, blanks, quote, escape,
                                 sep if rs is None else bytes(rs) if one else None)

    @staticmethod
    def _check_rs_alone(rs, sep, quote, escape, what):
        """The `rs=` keyword of record mode: 1 to 8 bytes, with the default `sep` and neither `quote` nor `escape`."""
        rs = _check_rs(rs)
        if _check_sep(sep) != 0x0A:
            raise ValueError("%s: rs= cannot be combined with sep=" % what)
        if quote is not None or escape is not None:
            raise ValueError("%s: rs= cannot be combined with quote= or escape=" % what)
        return rs

    def run_records(self, data, sep=b"\n", device=None, quote=None, escape=None, batch_actions=True, rs=None, chomp=False, ors=b"",
                    field=None, fs=None, fields=None, unquote=False, blanks=False, only=False, ofs=None, header=0, keys=None, optional=()):
        """Record mode on bytes: every record of `data` (split after each `sep` byte, kx_split_records on the device) is a
        whole input.  Returns a list holding, per record, its output bytes or a MatchError (pos, stage).  With a `quote` byte
        a separator inside quotes ends no record (kx_split_records_quoted from parity 0).  With an `escape` byte an escaped
        byte is only data (kx_split_records_escaped from state 0).  `batch_actions`: stages with register actions are replayed
        by the batch kernels (kx_config::batch_actions = 2 for this call) instead of routing every record.  With `rs` (1 to 8
        bytes; not with a `sep`, `quote` or `escape`) records end after the leftmost, non-overlapping copies of rs
        (kx_split_records_rs from an empty context).  With `chomp` every record is run without its separator (a tail, which
        has no valid one, whole) and the 0 to 8 bytes `ors` end the output of every accepted record (kx_run_batch_framed,
        chomp_records_model).  With `field` (from 1) the program runs on that field of every record — the fields lie between the
        live `fs` bytes — and the rest of the record is copied around its output (kx_run_batch_fields, field_records_model): the
        separator is never part of the body, and follows the output unless `chomp`; a record with fewer fields gives a
        NoFieldError.  With `fields` (a parse_field_list result, or a sequence of ints and (lo, hi) pairs; not with `field`) the
        program runs on every field of the list (kx_run_batch_field_list, field_list_records_model): a record with a rejected
        field gives a MatchError whose `field` is the lowest rejected field and whose `pos` counts inside it.  With `unquote`
        (with `field` or `fields`, and a `quote` or an `escape`) the program runs on the VALUE of every selected field and the
        field is replaced by the spelling of its output (kx_run_batch_field_values with the separator as the special byte,
        unquote_field_model, requote_field_model); `field=K` is then the list K-K, and `pos` counts inside the value.  With
        `blanks` (with `field` or `fields`, not with `fs`, whose default is a tab) the fields are the words between the record's
        live spaces and tabs and every blank is copied as it is (kx_run_batch_field_words, blank_field_list_records_model);
        `field=K` is then the list K-K, and a record without any word gives NoFieldError(0).  With `only` (with `field` or `fields`)
        an accepted record gives the outputs of its selected fields alone, in the order the `fields` sequence has them — items
        may overlap and repeat — joined by the 0 to 8 bytes `ofs` (default `fs`, or one space with `blanks`), then separator and
        `ors` as ever (kx_run_batch_field_project, project_records_model); with `unquote` the spellings protect `ofs`, one byte.
        With `header` = N the first N records are header records: the program never runs on them, and the list holds their bytes
        in their places — body, separator unless `chomp`, `ors`; with `only` their projection (kx_run_batch_field_header), or a
        NoFieldError.  `fields` may then hold bytes NAMES, resolved against the cells of record N (header_names_model,
        resolve_field_names): a name no cell has raises HeaderError; data with fewer than N records resolves nothing (under `only`
        with names its records then give b"").  With `keys` (the key separator C, one byte; with `fields`, a sequence of bytes
        NAMES; not with `header`) the fields are key C value pairs and the program runs on the value of the first field that has each
        name for a key (kx_run_batch_field_keys, keyed_records_model): a record that lacks a name not in `optional` gives a
        NoFieldError whose `field` is the first such name, a rejected value a MatchError whose `field` is its name; with `only` the
        outputs come in the order of `fields`, and a name the record lacks gives nothing."""
        if not isinstance(data, (bytes, bytearray, memoryview)):
            raise TypeError("run_records: data must be bytes, not %s" % type(data).__name__)
        keyed = self._check_keys("run_records", keys, optional, field, fields, fs, blanks, quote, escape, sep, rs, header)
        if keyed is not None:
            fields = [1] * len(keyed[2])                 # (a placeholder for the checks: the names select the fields)
        header, named = _check_header("run_records", header, fields)
        written = list(fields) if named else None
        if named:                                        # (a placeholder for the checks; the numbers come with record N)
            fields = [1 if isinstance(it, (bytes, bytearray)) else it for it in fields]
        chomp, ors = _check_chomp(chomp), _check_ors(ors)
        items, ofs = self._check_only("run_records", only, ofs, field, fields, fs, blanks)
        if items is not None:
            field, fields = None, list(items)
        field, fields = self._check_unquote("run_records", unquote, field, fields, quote, escape)
        field, fields, fs = self._check_blanks("run_records", blanks, field, fields, fs, sep, quote, escape, rs)
        if field is not None and fields is not None:
            raise ValueError("run_records: field= and fields= exclude each other")
        if field is not None:
            field = _check_field(field)
        if fields is not None:
            fields = _check_field_ranges(fields)
        if (field is not None or fields is not None) and not blanks:
            _check_fs(fs, quote, escape, sep if rs is None else rs if len(rs) == 1 else None)
        if rs is not None:
            rs = self._check_rs_alone(rs, sep, quote, escape, "run_records")
        sep_byte = bytes([_check_sep(sep)])              # (`sep` itself may be an int)
        if quote is not None:
            _check_quote(quote, sep)
        if escape is not None:
            _check_escape(escape, sep, quote)
        import torch
        data = bytes(data)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        v = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev) if data else torch.empty(0, dtype=torch.uint8, device=dev)
        mode = _records_mode(quote, escape, rs)
        if mode == KX_RECORDS_RS:
            offs, (_, tail_len) = split_rs_records_tensor(v, rs)
            tail = tail_len > 0                          # (the splitter's own report)
        else:
            if mode == KX_RECORDS_ESCAPED:
                offs, _ = split_escaped_records_tensor(v, sep, quote, escape)
                model = lambda d: split_escaped_records_model(d, sep, quote, escape)[0]   # noqa: E731
            elif mode == KX_RECORDS_QUOTED:
                offs, _ = split_quoted_records_tensor(v, sep, quote)
                model = lambda d: split_records_model(d, sep, quote)                      # noqa: E731
            else:
                offs = split_records_tensor(v, sep)
                model = lambda d: split_records_model(d, sep)                             # noqa: E731
            # tail: the last record has no valid separator.  The record starts at a boundary, where the split's state is 0, so
            # the split model says it: with one more byte behind the record, its end is a boundary iff a separator ends it.
            # (`data` is bytes here, whatever came in; reading offs[-2] waits for the split, as the batch's size query would.)
            last = data[int(offs[-2]):] if (chomp or field is not None or fields is not None) and offs.numel() > 1 else b""
            tail = bool(last) and len(last) not in model(last + b"\0")[:-1]
        trim = (len(rs) if rs is not None else 1) if chomp else 0

        def unpack(res):
            out, ooff, status, fpos, fstage = res[:5]
            torch.cuda.synchronize(dev)
            ob = out.cpu().numpy().tobytes()
            ooff, status, fpos, fstage = ooff.tolist(), status.tolist(), fpos.tolist(), fstage.tolist()
            ffield = [None] * len(status) if len(res) < 6 else res[5].tolist()
            if keyed is not None:
                name = lambda i: keyed[0][ffield[i] - 1]                                  # noqa: E731
                return [NoFieldError(fpos[i], name(i)) if status[i] == 2 else MatchError(fpos[i], fstage[i], name(i)) if status[i]
                        else ob[ooff[i]:ooff[i + 1]] for i in range(len(status))]
            return [NoFieldError(fpos[i]) if status[i] == 2 else MatchError(fpos[i], fstage[i], ffield[i]) if status[i] else ob[ooff[i]:ooff[i + 1]]
                    for i in range(len(status))]

        head, nrec, sep_len = [], offs.numel() - 1, len(rs) if rs is not None else 1
        nh = min(header, nrec)
        if nh:                                           # the header records
            ho = offs[:nh + 1].tolist()
            if named and nrec >= header:
                cut = 0 if tail and header == nrec else sep_len
                cells = header_names_model(data[ho[-2]:ho[-1] - cut], fs, quote, escape, blanks, header == 1)
                resolved = resolve_field_names(written, cells)
                try:
                    if items is not None:
                        items, fields = _check_field_items(resolved)
                    else:
                        fields = _check_field_ranges(resolved)
                except ValueError as ex:
                    raise HeaderError(None, str(ex))
            if items is not None and named and nrec < header:
                head = [b""] * nh
            elif items is not None:
                head = unpack(self.run_batch_field_header_tensor(
                    v, offs[:nh + 1], items, ofs, fs, blanks, quote, escape, unquote=unquote, special=sep_byte, sep_len=sep_len,
                    last_whole=bool(tail and nh == nrec), keep_sep=not chomp, suffix=ors))
            else:
                for i in range(nh):
                    cut = 0 if tail and i == nrec - 1 else sep_len
                    head.append(data[ho[i]:ho[i + 1] - cut] + (b"" if chomp else data[ho[i + 1] - cut:ho[i + 1]]) + ors)
            if nh == nrec:
                return head
            offs = offs[nh:]
        with self._batch_actions_for_call(batch_actions):
            if keyed is not None:
                res = self.run_batch_field_keys_tensor(
                    v, offs, keyed[0], keys, fs, blanks, quote, escape, optional, unquote=unquote, special=sep_byte,
                    only=keyed[2] if items is not None else None, ofs=ofs, sep_len=len(rs) if rs is not None else 1,
                    last_whole=bool(tail and data), keep_sep=not chomp, suffix=ors)
            elif items is not None:
                res = self.run_batch_field_project_tensor(
                    v, offs, items, ofs, fs, blanks, quote, escape, unquote=unquote, special=sep_byte,
                    sep_len=len(rs) if rs is not None else 1, last_whole=bool(tail and data), keep_sep=not chomp, suffix=ors)
            elif blanks:
                res = self.run_batch_field_words_tensor(
                    v, offs, fields, quote, escape, unquote=unquote, special=sep_byte, sep_len=len(rs) if rs is not None else 1,
                    last_whole=bool(tail and data), keep_sep=not chomp, suffix=ors)
            elif unquote:
                res = self.run_batch_field_values_tensor(
                    v, offs, fields, fs, quote, escape, special=sep_byte, sep_len=1, last_whole=bool(tail and data), keep_sep=not chomp,
                    suffix=ors)
            elif fields is not None:
                res = self.run_batch_field_list_tensor(
                    v, offs, fields, fs, quote, escape, sep_len=len(rs) if rs is not None else 1, last_whole=bool(tail and data),
                    keep_sep=not chomp, suffix=ors)
            elif field is not None:
                res = self.run_batch_fields_tensor(
                    v, offs, field, fs, quote, escape, sep_len=len(rs) if rs is not None else 1, last_whole=bool(tail and data),
                    keep_sep=not chomp, suffix=ors)
            else:
                res = self.run_batch_tensor(v, offs, trim=trim, last_whole=bool(trim and tail and data), suffix=ors)
        return head + unpack(res)

    def run_records_fd(self, in_fd, out_fd, sep=b"\n", report_fd=-1, quote=None, escape=None, batch_actions=True, rs=None, chomp=False,
                       ors=b"", field=None, fs=None, fields=None, unquote=False, blanks=False, only=False, ofs=None, header=0, keys=None,
                       optional=()):
        """kx_run_records_fd: the stream on in_fd in record mode, outputs to out_fd, one line per rejected record to report_fd
        (-1: none).  Returns kx_records_stats as a dict, with "rejected" = whether some record was rejected.  With a `quote`
        byte, kx_run_records_fd_quoted: a separator inside quotes ends no record.  With an `escape` byte,
        kx_run_records_fd_escaped: an escaped byte is only data (with or without a quote).  With `rs` (1 to 8 bytes),
        kx_run_records_fd_rs: records end after the leftmost, non-overlapping copies of rs.  `batch_actions` as in run_records.  With
        `chomp` or a non-empty `ors`, kx_run_records_fd_opts: records run without their separator, `ors` after every accepted
        record's output.  With `field`, kx_run_records_fd_fields: the program runs on field `field` of every record (fields end at
        the live `fs` bytes), the rest of the record is copied; a record with fewer fields is reported and counts as rejected.
        With `fields` (as in run_records; not with `field`), kx_run_records_fd_field_list: the program runs on every field of the
        list, and a record with a rejected field is reported once, with the field's number.  With `unquote` (as in run_records),
        kx_run_records_fd_field_values: the program runs on the values of the selected fields, which are spelled again behind it.
        With `blanks` (as in run_records), kx_run_records_fd_field_words: the fields are the words between live spaces and tabs.
        With `only` and `ofs` (as in run_records), kx_run_records_fd_field_project: only the selected fields' outputs are written.
        With `header` = N >= 1, kx_run_records_fd_table: the first N records are header records, and `fields` may hold bytes names of
        the cells of record N; a name no cell has raises EngineError (KX_E_HEADER) with the library's message.  With `keys` and
        `optional` (as in run_records), kx_run_records_fd_field_keys: the report lines name the field by its key."""
        keyed = self._check_keys("run_records_fd", keys, optional, field, fields, fs, blanks, quote, escape, sep, rs, header)
        if keyed is not None:
            fields = [1] * len(keyed[2])                 # (a placeholder for the checks: the names select the fields)
        header, named = _check_header("run_records_fd", header, fields)
        written = list(fields) if named else None
        if named:                                        # (a placeholder for the checks; the library resolves the names)
            fields = [1 if isinstance(it, (bytes, bytearray)) else it for it in fields]
        items, ofs = self._check_only("run_records_fd", only, ofs, field, fields, fs, blanks)
        if items is not None:
            field, fields = None, list(items)
        field, fields = self._check_unquote("run_records_fd", unquote, field, fields, quote, escape)
        field, fields, fs = self._check_blanks("run_records_fd", blanks, field, fields, fs, sep, quote, escape, rs)
        for name, fd in (("in_fd", in_fd), ("out_fd", out_fd), ("report_fd", report_fd)):
            if isinstance(fd, bool) or not isinstance(fd, int):
                raise TypeError("run_records_fd: %s must be an int file descriptor, not %s" % (name, type(fd).__name__))
        if rs is not None:
            rs = self._check_rs_alone(rs, sep, quote, escape, "run_records_fd")
        s = _check_sep(sep)
        q = None if quote is None else _check_quote(quote, sep)
        e = None if escape is None else _check_escape(escape, sep, quote)
        chomp, ors = _check_chomp(chomp), _check_ors(ors)
        mode, qi = _records_mode(q, e, rs), -1 if q is None else q
        if field is not None and fields is not None:
            raise ValueError("run_records_fd: field= and fields= exclude each other")
        if field is not None:
            field = _check_field(field)
        if fields is not None:
            fields = _check_field_ranges(fields)
        f = 0                                            # (with blanks= there is no field separator)
        if (field is not None or fields is not None) and not blanks:
            f = _check_fs(fs, quote, escape, sep if rs is None else rs if len(rs) == 1 else None)
        st = KxRecordsStats()
        with self._batch_actions_for_call(batch_actions):
            if chomp or ors or field is not None or fields is not None or header:   # the framing: only kx_run_records_fd_opts (and _fields, _field_list) has it
                o = KxRecordsOpts(size=ctypes.sizeof(KxRecordsOpts), mode=mode, sep=s, quote=qi, escape=-1 if e is None else e,
                                  rs_len=len(rs or b""), chomp=1 if chomp else 0, ors_len=len(ors))
                o.rs[:o.rs_len] = rs or b""
                o.ors[:len(ors)] = ors
                name, args = "kx_run_records_fd_opts", (ctypes.byref(o),)
                if field is not None:
                    name, args = "kx_run_records_fd_fields", (ctypes.byref(o), field, f)
                if fields is not None:
                    arr, nr = _field_range_array(fields)
                    name, args = "kx_run_records_fd_field_values" if unquote else "kx_run_records_fd_field_list", (ctypes.byref(o), arr, nr, f)
                    if blanks:
                        name, args = "kx_run_records_fd_field_words", (ctypes.byref(o), arr, nr, 1 if unquote else 0)
                    if items is not None:
                        if unquote:
                            _check_ofs_codec("run_records_fd", ofs, q, e, bytes([s]) + (b"\t" if blanks else b""))
                        iarr, ni = _field_item_array(items)
                        name, args = "kx_run_records_fd_field_project", (ctypes.byref(o), iarr, ni, f, ofs, len(ofs),
                                                                         (KX_PROJECT_WORDS if blanks else 0) | (KX_PROJECT_UNQUOTE if unquote else 0))
                if keyed is not None:
                    kk = field_keys_struct(keyed[0], keyed[1], keyed[3], (KX_KEYS_WORDS if blanks else 0) | (KX_KEYS_UNQUOTE if unquote else 0) |
                                           (KX_KEYS_ONLY if items is not None else 0))
                    karr = (ctypes.c_uint32 * 16)(*keyed[2])
                    name, args = "kx_run_records_fd_field_keys", (ctypes.byref(o), ctypes.byref(kk), f, karr, len(keyed[2]), ofs or b"", len(ofs or b""))
                if header:                               # one entry point for every combination
                    tflags = (KX_TABLE_WORDS if blanks else 0) | (KX_TABLE_UNQUOTE if unquote else 0) | (KX_TABLE_ONLY if items is not None else 0)
                    titems = written if named else items if items is not None else fields if fields is not None else []
                    if field is not None:
                        titems, tflags = [field], KX_TABLE_SINGLE
                    table = records_table(header, list(titems), tflags, f, ofs or b"")
                    name, args = "kx_run_records_fd_table", (ctypes.byref(o), ctypes.byref(table))
            else:                                        # the mode's own entry point
                name, args = (("kx_run_records_fd", (s,)), ("kx_run_records_fd_quoted", (s, q)), ("kx_run_records_fd_escaped", (s, qi, e)),
                              ("kx_run_records_fd_rs", (rs, len(rs or b""))))[mode]
            rc = getattr(self._lib, name)(self._h, in_fd, out_fd, *args, report_fd, ctypes.byref(st))
        self.last_records_stats = st
        if rc not in (0, 1):
            raise EngineError(self._err())
        d = st.as_dict()
        d["rejected"] = rc == 1
        return d

    def out_capacity(self, n, factor=None):
        """A generous output allocation for n input bytes (callers may also size exactly via shards)."""
        f = factor if factor is not None else 8
        return int(n * f) + 65536

    # sharded protocol (one shard per rank); thin wrappers, see include/kxhip.h
    def stage_has_actions(self, stage):
        return bool(self._lib.kx_stage_has_actions(self._h, stage))

    def stage_delayed_form(self, stage=0):
        """0: the stage has no delayed form; 1: it runs on it; 2: a shard gave it up (an undecided context), later shards run the general engine."""
        return int(self._lib.kx_stage_delayed_form(self._h, stage))

    def run_sharded(self, rank, world, gather, d_in, n, d_out, cap, stream=None):
        """kx_run_sharded: this rank's shard through every stage, the boundary hand-off done by the library through `gather`
        (a Comm, a GroupMember, or None when world == 1).  Returns the KxShardedResult; raises MatchError (global position)."""
        res = KxShardedResult()
        fn, ctx = (None, None) if gather is None else gather.callback()
        rc = self._lib.kx_run_sharded(self._h, rank, world, fn, ctx, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out), cap,
                                      ctypes.byref(res), ctypes.c_void_p(stream or 0))
        if rc == -3:
            self.last_stats = res.stats
            raise EngineError("output buffer too small: need %d bytes" % res.out_len)
        self._check(rc, res.stats)
        return res

    def shard_begin(self, stage, d_in, n, is_first, is_last, stream=None):
        if self.stage_has_actions(stage):
            raise EngineError("stage %d uses register actions: their replay is sequential over the whole stream, "
                              "run the program unsharded (kx_run_device / kx_run_fd)" % stage)
        return Shard(self, stage, d_in, n, is_first, is_last, stream)


class Comm:
    """The library's own RCCL communicator (kx_comm_*): rank 0 makes the 128-byte id, the launcher distributes it."""

    def __init__(self, rank, world, unique_id=None):
        self._lib = load_engine()
        self._h = ctypes.c_void_p()
        rc = self._lib.kx_comm_init(ctypes.byref(self._h), rank, world, unique_id)
        if rc:
            raise EngineError(self._lib.kx_last_error().decode("utf-8", "replace"))

    @staticmethod
    def unique_id():
        lib = load_engine()
        buf = ctypes.create_string_buffer(128)
        if lib.kx_comm_unique_id(buf):
            raise EngineError(lib.kx_last_error().decode("utf-8", "replace"))
        return buf.raw

    def callback(self):
        return ctypes.cast(self._lib.kx_comm_allgather, ctypes.c_void_p), self._h

    def close(self):
        if self._h:
            self._lib.kx_comm_free(self._h)
            self._h = ctypes.c_void_p()


class Group:
    """Ranks = threads of this process (kx_group_*): what the produced binary's `--gpus N` uses."""

    def __init__(self, world):
        self._lib = load_engine()
        self._h = ctypes.c_void_p(self._lib.kx_group_create(world))
        self.world = world

    def member(self, rank):
        return GroupMember(self, rank)

    def close(self):
        if self._h:
            self._lib.kx_group_free(self._h)
            self._h = ctypes.c_void_p()


class GroupMember:
    def __init__(self, group, rank):
        self._lib = group._lib
        self._h = ctypes.c_void_p(self._lib.kx_group_join(group._h, rank))

    def callback(self):
        return ctypes.cast(self._lib.kx_group_allgather, ctypes.c_void_p), self._h

    def close(self):
        if self._h:
            self._lib.kx_group_leave(self._h)
            self._h = ctypes.c_void_p()


class Shard:
    def __init__(self, prog, stage, d_in, n, is_first, is_last, stream=None):
        self._p = prog
        self._lib = prog._lib
        self._h = ctypes.c_void_p()
        rc = self._lib.kx_shard_begin(prog._h, stage, ctypes.c_void_p(d_in), n, int(is_first), int(is_last),
                                      ctypes.c_void_p(stream or 0), ctypes.byref(self._h))
        if rc:
            raise EngineError(prog._err())

    def _ck(self, rc):
        if rc:
            raise EngineError(self._p._err())

    def forward(self):
        s = KxFwdSummary()
        self._ck(self._lib.kx_shard_forward(self._h, ctypes.byref(s)))
        return s

    def fix_head(self, incoming_state):
        s = KxFwdSummary()
        self._ck(self._lib.kx_shard_fix_head(self._h, incoming_state, ctypes.byref(s)))
        return s

    def backward(self):
        s = KxBwdSummary()
        self._ck(self._lib.kx_shard_backward(self._h, ctypes.byref(s)))
        return s

    def resolve(self, end_leaf):
        n = ctypes.c_uint64()
        self._ck(self._lib.kx_shard_resolve(self._h, end_leaf, ctypes.byref(n)))
        return n.value

    def emit(self, d_out, cap):
        self._ck(self._lib.kx_shard_emit(self._h, ctypes.c_void_p(d_out), cap))

    def stats(self):
        s = KxStats()
        self._lib.kx_shard_stats(self._h, ctypes.byref(s))
        return s

    def end(self):
        if self._h.value:
            self._lib.kx_shard_end(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.end()
        except Exception:
            pass
