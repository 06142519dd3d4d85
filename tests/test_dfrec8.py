"""The delayed form's 8-byte piece records and wave-local output offsets (kx_dfkernels.inc: DfRec, the wave base array).

A piece record no longer says where the piece's output starts: k_demit adds up the lengths of the pieces in front of it in its
wave-iteration, from one absolute offset per iteration (one base word per 32 pieces).  The cases are the smallest shapes at which
that can go wrong: every field of the record at its bound, a wave-iteration whose first piece lies on and off a block boundary and
in an own and in a spill part, iterations of half pieces, a class table of indices, pieces resolved on the slow path (hole records)
that begin on and next to a base word's piece, windows and shards.  Every output is compared byte for byte with the oracle."""
import os
import random
import subprocess

import pytest
from conftest import blob_of
from test_delayed_form import expect, many_classes_program

from kleenexlang_amd import MatchError, Program, host, workloads

PIECE = 64
SEGMENTS = (64, 4096, 0)          # a block of one piece, of 64 pieces (one wave-iteration), the engine's own choice


def run(p, data):
    try:
        return p.run_host(data)
    except MatchError as e:
        return ("fail", e.pos)


def check(blob, datas, segments=SEGMENTS, on_form=True):
    """every input on the delayed form at every segment size, against the oracle (computed once per input)"""
    wants = [expect(blob, d) for d in datas]
    for seg in segments:
        p = Program(blob, segment_bytes=seg)
        try:
            for d, want in zip(datas, wants):
                assert run(p, d) == want, (seg, len(d))
                if on_form and not isinstance(want, tuple) and len(d):
                    assert p.stage_delayed_form(0) == 1, (seg, len(d), "the run left the delayed form")
                p.reset_delayed_form(0)
        finally:
            p.close()


def stretch(line, shape, k):
    """the line, k bytes longer, still of its shape"""
    if shape == "apache_log":
        return line[:-2] + b"x" * k + line[-2:]          # (inside the quoted agent field)
    if shape == "csv":
        f = line.split(b",")
        f[1] += b"x" * k
        return b",".join(f)
    raise ValueError(shape)


def exactly(shape, n, seed):
    """n bytes of whole lines of the shape (the last one stretched to fit); where n is too short for one line, the first n bytes
    of one — the engine then has to reject it where the oracle does"""
    lines = workloads.generate(shape, n + 4096, seed).split(b"\n")[:-1]
    out = b""
    for i, ln in enumerate(lines):
        nxt = lines[i + 1]
        if len(out) + len(ln) + 1 + len(nxt) + 1 > n:     # ln is the last line that fits with room to spare: stretch it
            room = n - len(out) - len(ln) - 1
            if room < 0 and shape == "csv" and n >= 14:
                return b"1," + b"x" * (n - 14) + b",,,,1.1.1.1\n"      # (the shortest row there is, its first name stretched)
            if room < 0:
                return (out + ln + b"\n")[:n]
            return out + stretch(ln, shape, room) + b"\n"
        out += ln + b"\n"
    raise AssertionError("not enough lines")


def test_exactly_gives_whole_lines_of_the_asked_length():
    for shape in ("apache_log", "csv"):
        for n in (2047, 2048, 2049, 4096 * 3 + 1, 64 * 64 * 2 + 17):
            d = exactly(shape, n, 5)
            assert len(d) == n and d.endswith(b"\n")
    for n in (63, 64, 65):
        d = exactly("csv", n, 5)
        assert len(d) == n and not isinstance(expect(blob_of("csv2json"), d), tuple)
    assert len(exactly("apache_log", 63, 5)) == 63 and len(exactly("csv", 1, 5)) == 1


# ------------------------------------------------------------------------------------------------------------ field maxima
LONGEST = "Q" * 125      # the longest constant a step may append (kx_delayed.h: copy + constant <= 126 bytes)


def maxima_programs():
    return {"long": 'main := (/[a-z]/ "%s")*\n' % LONGEST,        # every step: 126 bytes: len = 64 * 126, lenA = 32 * 126
            "short": 'main := (/[a-z]/ "ab")*\n'}                   # every step a constant: kA = kB = 32


def test_field_maxima_programs_have_a_delayed_form():
    for name, src in maxima_programs().items():
        info, _ = host.df_describe(blob_of(src))
        assert info.available == 1 and info.escapes == 0, (name, info.reason)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["long", "short"])
def test_field_maxima(name):
    """len and lenA at their bounds with pieces of 8 064 output bytes; 32 constants in either half of every piece (a round may
    overflow its job slots: the output must still match)"""
    blob = blob_of(maxima_programs()[name])
    r = random.Random(3)
    datas = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(n)) for n in (64, 65, 4096, 4097)]
    per = 126 if name == "long" else 3
    assert [len(expect(blob, d)) for d in datas] == [per * len(d) for d in datas]
    check(blob, datas)


# ------------------------------------------------------------------------------------- the base array and the wave prefix
LENGTHS = (1, 63, 64, 65, 2047, 2048, 2049, 4096 * 3 + 1, 64 * 64 * 2 + 17)


@pytest.mark.gpu
@pytest.mark.parametrize("prog,shape", [("apache_log", "apache_log"), ("csv2json", "csv")])
def test_wave_base_and_prefix_across_block_boundaries(prog, shape):
    """a wave-iteration's first piece on a block boundary (segments of 64 pieces: every iteration; of one piece: every piece is a
    block) and off it (the default segment size), in an own part and in a spill part (a lane's own part starts K + J symbols behind
    its synchronisation point: the pieces before belong to the lane in front).  An apache_log line is longer than 65 bytes: at 1, 63, 64
    and 65 bytes its input is the start of one line, and the case checks only that the engine rejects it where the oracle does —
    at those sizes only csv2json (whose shortest row is 14 bytes) produces output and exercises the offsets."""
    blob = blob_of(prog)
    datas = [exactly(shape, n, 100 + n) for n in LENGTHS]
    check(blob, datas)


@pytest.mark.gpu
def test_half_piece_iterations():
    """iso_datetime_to_json: a lane takes half a piece, a wave-iteration is 32 pieces = one base word; 31, 32, 33 and 65 pieces"""
    blob = blob_of("iso_datetime_to_json")
    lines = workloads.generate("datetime", 8192, 9).split(b"\n")[:-1]
    datas = []
    for pieces in (31, 32, 33, 65):
        d = b""
        for ln in lines:
            if len(d) + len(ln) + 1 > pieces * PIECE:
                break
            d += ln + b"\n"
        assert (len(d) + PIECE - 1) // PIECE == pieces, (pieces, len(d))
        datas.append(d)
    check(blob, datas, segments=(64, 4096))


@pytest.mark.gpu
def test_more_than_31_byte_classes_at_4k_plus_1():
    r = random.Random(13)
    for width in (2, 8):
        src, letters = many_classes_program(width)
        data = bytes(r.choice((letters + "0123456789 ").encode()) for _ in range(4096 + 1))
        check(blob_of(src), [data])


# -------------------------------------------------------------------------------------------------------------------- holes
def with_context_at(lines, k, where):
    """the log lines with an undecided context (an escaped quote in the request field) in line k, its backslash at a position
    congruent to `where` modulo 32 pieces: the line before is stretched"""
    lines = list(lines)
    lines[k] = lines[k].replace(b' HTTP/', b'\\"   5x HTTP/', 1)
    at = sum(len(ln) + 1 for ln in lines[:k]) + lines[k].index(b'\\"')
    lines[k - 1] = stretch(lines[k - 1], "apache_log", (where - at) % (32 * PIECE))
    data = b"\n".join(lines) + b"\n"
    assert data.index(b'\\"') % (32 * PIECE) == where
    return data


@pytest.mark.gpu
def test_holes_on_and_next_to_a_base_word():
    """a stretch that the forward pass resolves itself begins in the piece that holds the context: at a piece whose index is a multiple
    of 32 (its record is a hole AND it writes the base word), one piece before that (the base word's piece lies inside the stretch),
    and in the input's last line (the stretch runs to the end of the input)"""
    blob = blob_of("apache_log")
    # (50 segments: a stage arms its slow path only where fewer than a sixteenth of the shard's lanes met such a context)
    lines = workloads.generate("apache_log", 200 * 1024, 17).split(b"\n")[:-1]
    k = len(lines) // 2
    datas = [with_context_at(lines, k, 20), with_context_at(lines, k, 31 * PIECE + 20), with_context_at(lines, len(lines) - 1, 20),
             with_context_at(lines, len(lines) - 1, 31 * PIECE + 20)]
    wants = [expect(blob, d) for d in datas]
    assert not any(isinstance(w, tuple) for w in wants)
    general = Program(blob, config=host.config_from_env({"KX_DF": "0"}), segment_bytes=4096)
    p = Program(blob, segment_bytes=4096)
    try:
        for d, want in zip(datas, wants):
            assert general.run_host(d) == want and general.stage_delayed_form(0) == 0
            assert p.run_host(d) == want, len(d)
            assert p.stage_delayed_form(0) == 1, "the shard fell back instead of resolving the stretch"
    finally:
        p.close()
        general.close()


# ------------------------------------------------------------------------------------------------------ windows and shards
@pytest.mark.gpu
def test_windows_and_two_shards(tmp_path):
    """later windows and shards take their head from k_dhead, which writes records and base words of its own"""
    from kleenexlang_amd import build, program_path
    exe = tmp_path / "apache_log"
    assert subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("apache_log"), "--out", str(exe)]).returncode == 0
    data = workloads.generate("apache_log", 256 * 1024, 23)
    want = expect(blob_of("apache_log"), data)
    r = subprocess.run([str(exe)], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, KX_WINDOW_BYTES="50000", KX_DEBUG="1"))
    assert r.returncode == 0 and r.stdout == want
    assert b"delayed form" in r.stderr and b"falls back" not in r.stderr
    src = tmp_path / "apache_log.in"
    src.write_bytes(data)
    with open(src, "rb") as fin:
        r = subprocess.run([str(exe), "--gpus", "2"], stdin=fin, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(os.environ, KX_DEBUG="1", KX_SHARD_SAME_DEVICE="1"))
    assert r.returncode == 0 and r.stdout == want, r.stderr[-300:]
    assert b"falls back" not in r.stderr, "a shard left the delayed form: " + r.stderr[-300:].decode(errors="replace")
