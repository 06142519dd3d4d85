"""CPU: the batch replay of register-action stages (kx_config::batch_actions, kx_batch_actions.inc) — the ABI of the switch and
of the new statistics, and the MEASURE rule (k_bact_measure: the replay with lengths only) against a full replay stated in
Python after Actions.hs:28-38.  No device needed."""
import ctypes
import random

from kleenexlang_amd import host

ESC, PUSH, POP, WRITE = 0xFF, 0x00, 0x01, 0x02      # include/kxp_format.h


def test_the_switch_and_the_statistics_without_changing_a_struct_size():
    names = [f[0] for f in host.KxConfig._fields_]
    assert "batch_actions" in names
    assert ctypes.sizeof(host.KxConfig) == 112          # the parent commit's size
    assert ctypes.sizeof(host.KxBatchStats) == 80        # the parent commit's size
    assert host.config_from_env({}).batch_actions == 0
    assert host.config_from_env({"KX_BATCH_ACTIONS": "1"}).batch_actions == 2
    assert host.config_from_env({"KX_BATCH_ACTIONS": "0"}).batch_actions == 1
    snames = [f[0] for f in host.KxBatchStats._fields_]
    assert "docs_replayed" in snames and "actions_ms" in snames
    assert host.KxBatchStats.docs_replayed.size == 8 and host.KxBatchStats.actions_ms.size == 4
    d = host.KxBatchStats().as_dict()
    assert d["docs_replayed"] == 0 and d["actions_ms"] == 0.0 and d["docs_routed"] == 0


# ------------------------------------------------------------------------------------------------- token streams by hand
def lit(b):
    return bytes(b).replace(b"\xff", b"\xff\xff")


def push():
    return bytes([ESC, PUSH])


def pop(r):
    return bytes([ESC, POP, r])


def write(r):
    return bytes([ESC, WRITE, r])


def tokens(stream):
    """(kind, value) per token: ("lit", byte), ("push", None), ("pop", r), ("write", r); a token cut by the end ends the list."""
    i, n = 0, len(stream)
    while i < n:
        if stream[i] != ESC:
            yield "lit", stream[i]
            i += 1
            continue
        if i + 1 >= n:
            return
        t = stream[i + 1]
        if t == ESC:
            yield "lit", 0xFF
            i += 2
        elif t == PUSH:
            yield "push", None
            i += 2
        else:
            if i + 2 >= n:
                return
            yield ("pop" if t == POP else "write"), stream[i + 2]
            i += 3


def replay(stream, nregs):
    """The full replay (Actions.hs:28-38 on a stack of buffers): returns the bottom buffer.  Registers still full and frames
    still open at the end are dropped; Pop at depth 0 and registers >= nregs are ignored."""
    stack, regs = [bytearray()], {}
    for kind, v in tokens(stream):
        if kind == "lit":
            stack[-1].append(v)
        elif kind == "push":
            stack.append(bytearray())
        elif v >= nregs:
            continue
        elif kind == "pop":
            if len(stack) > 1:
                regs[v] = stack.pop()
        else:
            stack[-1] += regs.get(v, b"")
            regs[v] = bytearray()
    return bytes(stack[0])


def measure(stream, nregs):
    """k_bact_measure's rule: numbers only.  `below[k]` = length of the buffer under frame k + 1 while it is open, `cur` = length
    of the top buffer, `reg[r]` = length of register r.  Returns (replayed length, deepest nesting, highest register used)."""
    below, reg, cur, maxdepth, maxreg = [], {}, 0, 0, -1
    for kind, v in tokens(stream):
        if kind == "lit":
            cur += 1
        elif kind == "push":
            below.append(cur)
            cur = 0
            maxdepth = max(maxdepth, len(below))
        elif v >= nregs:
            continue
        elif kind == "pop":
            maxreg = max(maxreg, v)
            if below:
                reg[v] = cur
                cur = below.pop()
        else:
            maxreg = max(maxreg, v)
            cur += reg.get(v, 0)
            reg[v] = 0
    return (below[0] if below else cur), maxdepth, maxreg


CASES = {
    "empty": (b"", 2, b""),
    "plain": (lit(b"hello"), 2, b"hello"),
    "swap": (push() + lit(b"ab") + pop(0) + push() + lit(b"12") + pop(1) + write(1) + lit(b",") + write(0) + lit(b"\n"), 2, b"12,ab\n"),
    "nested frames": (push() + push() + lit(b"aa") + pop(1) + lit(b"<") + write(1) + lit(b">b") + pop(0) + write(0) + lit(b"|") + write(0)
                      + lit(b"|") + write(1), 2, b"<aa>b||"),
    "register written twice": (push() + lit(b"xyz") + pop(0) + write(0) + write(0) + lit(b"."), 1, b"xyz."),
    "pop at depth 0": (lit(b"a") + pop(0) + lit(b"b") + write(0), 1, b"ab"),
    "register beyond act_regs": (push() + lit(b"q") + pop(5) + write(5) + lit(b"r"), 2, b""),       # the Pop is ignored: the frame stays open
    "escaped FF in literals": (lit(b"\xff\xffa\xff"), 1, b"\xff\xffa\xff"),
    "escaped FF in a frame and a register": (push() + lit(b"\xffa\xff") + pop(0) + lit(b"[") + write(0) + lit(b"]"), 1, b"[\xffa\xff]"),
    "ends with registers full": (push() + lit(b"ab") + pop(0) + lit(b"1"), 1, b"1"),
    "ends with a frame open": (lit(b"k") + push() + lit(b"lost"), 1, b"k"),
    "write into a frame": (push() + lit(b"a") + pop(0) + push() + lit(b"<") + write(0) + lit(b">") + pop(1) + write(1) + write(1), 2, b"<a>"),
    "cut token": (lit(b"ab") + bytes([ESC]), 1, b"ab"),
    "cut pop": (push() + lit(b"ab") + bytes([ESC, POP]), 1, b""),
}


def test_measure_gives_the_length_of_the_full_replay_on_streams_built_by_hand():
    for name, (stream, nregs, want) in CASES.items():
        assert replay(stream, nregs) == want, name
        assert measure(stream, nregs)[0] == len(want), name
    # the classes' inputs: nesting and registers as the lane interpreter limits them (LANE_DEPTH = LANE_REGS = 8)
    deep = b"".join(push() + lit(b"x") for _ in range(9)) + b"".join(pop(0) + write(0) for _ in range(9))
    assert measure(deep, 1) == (len(replay(deep, 1)), 9, 0)
    ten = b"".join(push() + lit(b"%d" % r) + pop(r) for r in range(10)) + b"".join(write(r) for r in reversed(range(10)))
    assert replay(ten, 10) == b"9876543210" and measure(ten, 10) == (10, 1, 9)


def test_measure_agrees_with_the_full_replay_on_random_streams():
    rnd = random.Random(7)
    for _ in range(3000):
        nregs = rnd.choice([1, 2, 3, 9])
        parts = []
        for _ in range(rnd.randrange(0, 30)):
            k = rnd.random()
            if k < 0.4:
                parts.append(lit(bytes(rnd.choice(b"ab\xff") for _ in range(rnd.randrange(1, 6)))))
            elif k < 0.6:
                parts.append(push())
            elif k < 0.8:
                parts.append(pop(rnd.randrange(nregs + 1)))
            else:
                parts.append(write(rnd.randrange(nregs + 1)))
        stream = b"".join(parts)
        if rnd.random() < 0.2:
            stream = stream[:rnd.randrange(len(stream) + 1)]      # (possibly inside a token: the replay ends there)
        got = measure(stream, nregs)[0]
        assert got == len(replay(stream, nregs)), stream
