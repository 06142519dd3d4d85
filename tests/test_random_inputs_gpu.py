"""GPU: generated programs on long ACCEPTED inputs (test_random_inputs.py: sampled from the program's own transducer, with the rejected
variants derived from them), on every route of the engine.  Every result is compared byte for byte with the CPU oracle on the same
blob — or ("fail", pos) with its position; nothing is compared with another run of the engine.  Which engine ran is asserted, not
assumed: kx_stage_delayed_form and the lines the library prints under KX_DEBUG (the regexes of test_instances_gpu.py).

  a. both single-document engines at piece, wave-iteration, block and segment edges     test_engines_*
  b. the delayed form leaving the form in mid-run (in-lane resolve, shard fall-back, back-off) test_leaving_the_form_*
  c. the chunk-parallel replay of register actions                                         test_action_replay_*
  d. the batch route                                                                       test_batch_*

A program is left out only by a counted rule: it does not compile or its path tree is too large (test_random_programs._usable), or the
engine refuses to load it (table limits).  The seeds run in chunks, one test each; the chunks' counts are kept in this module, and the
*_populations tests — which run whatever chunk has not run yet — assert them against the floors of test_random_inputs.py."""
import pytest
import test_random_inputs as tr
from conftest import blob_of
from test_batch_actions_gpu import _arrays, _check_arrays
from test_batch_gpu import _check
from test_instances_gpu import demit_lines, emit_lines, log  # noqa: F401  (log: the fixture)

from kleenexlang_amd import EngineError, Program, host

pytestmark = pytest.mark.gpu

TARGETS = tr.EDGE_TARGETS + (tr.FAR,)
NCHUNK = 8
CHUNKS = [range(c, tr.NPROG, NCHUNK) for c in range(NCHUNK)]
SMALL_BLOCK = 64                                   # (the small legal workgroup of test_instances_gpu.test_block_threads)
# (segment_bytes, block_threads): blocks of one piece, of one wave-iteration, the engine's own choice (the delayed form's SEGMENTS), and
# one-piece segments in workgroups of 64 lanes: the 8 209-byte input's 129 segments span three workgroups
CONFIGS = {"delayed": ((64, 0), (4096, 0), (0, 0), (64, SMALL_BLOCK)), "general": ((64, 0), (4096, 0), (64, SMALL_BLOCK))}
MODE_ENV = {"delayed": {}, "general": {"KX_DF": "0"}}


def load(src, env=None, **fields):
    """the configuration goes through config_from_env; None where the engine refuses the tables"""
    try:
        return Program(blob_of(src, 3), config=host.config_from_env(env or {}, **fields))
    except EngineError:
        return None


def inputs_of(kind, seed):
    """every distinct sample with its variants, once"""
    seen, out = set(), []
    for t in TARGETS:
        for d in (tr.sample(kind, seed, t),) + tr.variants(kind, seed, t):
            if d not in seen:
                seen.add(d)
                out.append(d)
    return out


def reset(p):
    for s in range(p.num_stages):
        p.reset_delayed_form(s)


_FAULT = []


def run(log, p, data):
    """log(p, data); after an engine error in a run (a refused load is none) no test of this file starts anything on the GPU again"""
    assert not _FAULT, ("an earlier run ended in an engine error: nothing more is started on the GPU", _FAULT)
    try:
        return log(p, data)
    except EngineError as e:
        _FAULT.append(str(e))
        raise


# ------------------------------------------------------------------------------------------------ a. both engines, edges
_ENGINES = {}


def engines_chunk(log, kind, mode, chunk):
    """-> per seed of the chunk: None (refused by the engine) or {"long", "on_form", "escaped", "runs"}"""
    key = (kind, mode, chunk)
    if key in _ENGINES:
        return _ENGINES[key]
    res, bad = {}, []
    for seed in CHUNKS[chunk]:
        src = tr.source(kind, seed)
        if src is None:
            continue
        p = load(src, MODE_ENV[mode])
        if p is None:
            res[seed] = None
            continue
        datas = inputs_of(kind, seed)
        wants = [tr.expect(kind, seed, d) for d in datas]
        samples = {tr.sample(kind, seed, t) for t in TARGETS}      # (the table is simulated on the samples only: Python)
        forms = [tr.on_the_form(kind, seed, d) if mode == "delayed" and d in samples else None for d in datas]
        assert all(isinstance(w, bytes) for d, w in zip(datas, wants) if d in samples), (kind, seed, src, "the oracle rejects a sample")
        long_sample = tr.sample(kind, seed, tr.LONG)
        c = {"long": len(long_sample) >= tr.LONG_MIN, "on_form": 0, "escaped": 0, "runs": 0,
             "form_of_long": tr.on_the_form(kind, seed, long_sample) if mode == "delayed" else None}
        try:
            single = p.num_stages == 1
            for seg, bt in CONFIGS[mode]:
                p.configure(segment_bytes=seg, block_threads=bt)
                for d, want, form in zip(datas, wants, forms):
                    got, err = run(log, p, d)
                    where = (kind, mode, seed, src, seg, bt, len(d))
                    c["runs"] += 1
                    if got != want:
                        bad.append(where + ("other bytes" if isinstance(got, bytes) else got, want if isinstance(want, tuple) else len(want), err[-300:]))
                    elif mode == "general":
                        if p.stage_delayed_form(0) != 0 or demit_lines(err):
                            bad.append(where + ("the general engine was asked for", err[-300:]))
                    elif isinstance(want, bytes) and len(d):
                        if form:
                            # the simulated table stayed on the form: so did the engine, and k_demit wrote the output
                            lines = demit_lines(err)
                            if p.stage_delayed_form(0) != 1:
                                bad.append(where + ("the run left the delayed form", p.stage_delayed_form(0), err[-300:]))
                            elif not ((len(lines) == 1 and not emit_lines(err)) if single else lines):
                                bad.append(where + ("not one delayed-form emit line", err[-300:]))
                            c["on_form"] += 1
                        elif form is False:
                            c["escaped"] += 1
                    reset(p)
        finally:
            p.close()
        res[seed] = c
    _ENGINES[key] = res
    assert not bad, (len(bad), bad[:6])
    return res


@pytest.mark.parametrize("chunk", range(NCHUNK))
@pytest.mark.parametrize("mode", ["delayed", "general"])
@pytest.mark.parametrize("kind", ["plain", "wide"])
def test_engines_on_sampled_inputs(log, kind, mode, chunk):
    """Accepted inputs of 65, 4 031, 4 097, 8 209 and about 20 500 bytes and their rejected variants (a byte overwritten, the input cut:
    at 63, 64, 4 095, 4 096, the last byte and a random one), in segments of 64 and 4 096 bytes and the engine's own, and in
    workgroups of 64 lanes — on the general engine (KX_DF=0: no delayed-form line, kx_stage_delayed_form 0) and by default, where an
    input on which the simulated table stays on the form must run on the form (state 1, one `emit (delayed form` line, no general
    `emit:` line; a second stage prints its own) and an input on which it escapes must still give the oracle's bytes."""
    res = engines_chunk(log, kind, mode, chunk)
    assert any(c and c["runs"] for c in res.values())


@pytest.mark.parametrize("kind", ["plain", "wide"])
def test_engines_populations(log, kind):
    """Programs run (not refused by the engine), over all chunks, against the floors of test_random_inputs.FLOORS: with a long input;
    whose long input ran on the form; whose long input escapes in the simulation (and gave the oracle's bytes all the same).
    Measured on an MI355X — plain: 119 run, 0 refused, 87 long, 70 on the form, 13 escaping; wide: 120 run, 0 refused, 93 long, 83 on
    the form, 5 escaping (the line this test prints)."""
    tot = {"run": 0, "refused": 0, "long": 0, "on_form": 0, "escaped": 0, "long_general": 0}
    for chunk in range(NCHUNK):
        for c in engines_chunk(log, kind, "delayed", chunk).values():
            tot["refused" if c is None else "run"] += 1
            if c and c["long"]:
                tot["long"] += 1
                tot["on_form"] += c["form_of_long"] is True and c["on_form"] > 0
                tot["escaped"] += c["form_of_long"] is False and c["escaped"] > 0
        tot["long_general"] += sum(c is not None and c["long"] for c in engines_chunk(log, kind, "general", chunk).values())
    print("engines", kind, tot)
    floors = tr.FLOORS[kind]
    assert min(tot["long"], tot["long_general"]) >= floors["long"] and tot["on_form"] >= floors["on_form"] and tot["escaped"] >= floors["escape"], (kind, tot)


# --------------------------------------------------------------------------------------- b. leaving the form in mid-run
LEAVE_AT = 4096


def leaving_inputs(kind, seed):
    """Accepted inputs of about 2 and 3 * 4 096 bytes on which the simulated table escapes, but not before byte 4 096 — behind a head on
    which the table stays on the form.  Most of these programs escape in nearly every round of their star, so the head is put together
    from short accepted inputs, each kept only if the table takes it from where the head left it.  Behind the head:
      dense    the program's escaping 8 KiB sample (escapes in most segments: the shard falls back);
      sparse   ONE short accepted input on which the table escapes from where the head left it, and the head once more (a few
               escaping lanes among the 130 of one-piece segments: fewer than a sixteenth, so the stage arms its slow path).
    [] where no such head is found or no concatenation is accepted (`main` is no star): counted by the caller."""
    import random
    import struct
    info, img = tr.table(kind, seed)
    csh = 3 if info.nclasses > 31 else 0
    fst, alphabet = tr.transducers(kind, seed)[0], tr.KINDS[kind][1]
    r = random.Random(seed * 77 + 1)
    head, h, escaping = b"", info.start_handle, None
    for _ in range(8000):
        if len(head) >= LEAVE_AT + 40 and escaping:
            break
        unit = tr.randprog.accepted_input(fst, r, r.randint(1, 16), alphabet)
        h2 = h
        for b in unit:
            h2 = struct.unpack_from("<I", img, h2 + (img[b] << csh))[0] & 0xFFFF
            if h2 in (info.dead_handle, info.escape_handle):
                break
        else:
            if len(head) < LEAVE_AT + 40:
                head, h, escaping = head + unit, h2, None
            continue
        if h2 == info.escape_handle and len(head) >= LEAVE_AT + 40:
            escaping = unit
    if len(head) < LEAVE_AT + 40:
        return []
    out = []
    for data in (head + tr.sample(kind, seed, tr.LONG),) + ((head + escaping + head,) if escaping else ()):
        if isinstance(tr.expect(kind, seed, data), bytes) and _first_escape(kind, seed, data) > LEAVE_AT:
            out.append(data)
    return out


def _first_escape(kind, seed, data):
    from test_delayed_form import Escape, simulate
    info, img = tr.table(kind, seed)
    try:
        simulate(blob_of(tr.randprog.first_stage(tr.source(kind, seed)), 3), info, img, data, info.delay)
    except Escape as e:
        return e.args[0]
    return -1


def escaping_seeds(kind):
    return [s for s in tr.long_seeds(kind) if tr.on_the_form(kind, s, tr.sample(kind, s, tr.LONG)) is False]


def test_leaving_the_form_in_mid_run(log):
    """The programs whose 8 KiB sample escapes in the simulation, on an input whose first escape lies behind byte 4 096: with the slow
    path (the lane that meets the context resolves its stretch in place) and without it (KX_OFF_SLOW: the shard falls back to the
    general engine), with the back-off and without (df_backoff = 1), in the engine's own segments and in segments of 4 096 and of 64
    bytes, on an input that escapes in most segments and on one that escapes once (leaving_inputs) —
    and again on the next two runs of the same Program, in whatever state (1, 2 or 3) the first left the stage.  Always the oracle's
    bytes.  Without the slow path and with the back-off, the first run must leave the stage backing off (2) or given up (3).
    Measured on an MI355X (the line this test prints): 10 programs reached, 8 skipped, of 720 runs 80 resolved their stretch in place
    and 504 fell back."""
    reached = skipped = resolved = fell_back = 0
    for kind in ("plain", "wide"):
        for seed in escaping_seeds(kind):
            datas = leaving_inputs(kind, seed)
            if not datas:
                skipped += 1
                continue
            src = tr.source(kind, seed)
            ran = False
            for disable in (0, host.KX_OFF_SLOW):
                for backoff in (0, 1):
                    p = load(src, disable=disable, df_backoff=backoff)
                    if p is None:
                        continue
                    ran = True
                    try:
                        for seg, data in [(seg, d) for seg in (0, 4096, 64) for d in datas]:
                            want = tr.expect(kind, seed, data)
                            p.configure(segment_bytes=seg)
                            reset(p)
                            states = []
                            for _ in range(3):
                                got, err = run(log, p, data)
                                assert got == want, (kind, seed, src, disable, backoff, seg, len(data), states, err[-400:])
                                states.append(p.stage_delayed_form(0))
                                resolved += "the slow path resolved" in err
                                fell_back += "falls back to the general engine" in err
                            if disable and not backoff:
                                assert states[0] in (2, 3), (kind, seed, src, seg, len(data), states)
                    finally:
                        p.close()
            reached += ran
    print("leaving the form: reached", reached, "skipped", skipped, "runs resolved in place", resolved, "runs fallen back", fell_back)
    assert reached >= tr.FLOORS["plain"]["escape"], (reached, skipped)
    assert fell_back > 0 and resolved > 0, "no run fell back, or none resolved its stretch in place: the case proves nothing about that way out"


# --------------------------------------------------------------------------------------------- c. chunk-parallel replay
ACTION_SEEDS = range(0, tr.NPROG, 2)
ACTION_CHUNKS = [ACTION_SEEDS[c::6] for c in range(6)]
ACTION_TARGET = 40 * 1024
SMALL_CHUNKS = {"KX_ACT_PAR_MIN": "8192", "KX_ACT_CHUNK": "2048"}      # (as test_action_post_pass_replays_independent_chunks_in_parallel)
_ACTIONS = {}


def actions_chunk(log, chunk):
    """-> per seed: None (refused) or {"long", "parallel"}"""
    if chunk in _ACTIONS:
        return _ACTIONS[chunk]
    res = {}
    for seed in ACTION_CHUNKS[chunk]:
        src = tr.source("actions", seed)
        if src is None:
            continue
        data = tr.sample("actions", seed, ACTION_TARGET)
        ff = tr.sample("actions", seed, ACTION_TARGET // 4, b"abc\n\xff\xff")
        datas = [data] + ([ff] if b"\xff" in ff else [])
        wants = [tr.expect("actions", seed, d) for d in datas]
        assert all(isinstance(w, bytes) for w in wants)
        c = {"long": len(data) >= ACTION_TARGET, "parallel": False, "ff": len(datas) > 1}
        for env, fields in ((SMALL_CHUNKS, {"act_lanes": 1}), (SMALL_CHUNKS, {"act_lanes": 2}), ({}, {})):
            p = load(src, env, **fields)
            if p is None:
                res[seed] = None
                break
            try:
                for d, want in zip(datas, wants):
                    got, err = run(log, p, d)
                    assert got == want, ("actions", seed, src, fields, len(d), err[-400:])
                    if env and d is data:
                        par = "chunks of about" in err
                        assert fields["act_lanes"] == 1 or par == c["parallel"], ("lanes and waves disagree on whether the stream can be cut", seed, src)
                        c["parallel"] = par
            finally:
                p.close()
        else:
            res[seed] = c
    _ACTIONS[chunk] = res
    return res


@pytest.mark.parametrize("chunk", range(len(ACTION_CHUNKS)))
def test_action_replay_on_generated_programs(log, chunk):
    """program_actions on accepted inputs of 40 KiB, with chunks of 2 KiB from 8 KiB on (one wave per chunk, act_lanes = 1, and one lane
    per chunk, 2) and with the defaults; and one stream of 10 KiB sampled with the byte FF in the alphabet (escaped in the token stream,
    next to cuts) where the program's classes admit it.  The oracle's bytes every time."""
    res = actions_chunk(log, chunk)
    assert any(c is not None for c in res.values())


def test_action_replay_populations(log):
    """Of the programs with a long input, at least a third replay in parallel chunks (the `chunks of about` line) and at least 5 find
    no safe cut point and fall back to the one-wave replay.  Measured on an MI355X (the line this test prints): 60 programs, none
    refused, all 60 with a long input; 25 replay in parallel chunks, 35 by one wave; 44 have a stream that holds FF."""
    cs = [c for chunk in range(len(ACTION_CHUNKS)) for c in actions_chunk(log, chunk).values()]
    longs = [c for c in cs if c and c["long"]]
    par = sum(c["parallel"] for c in longs)
    print("action replay: programs", len(cs), "refused", cs.count(None), "long", len(longs), "parallel", par, "one wave", len(longs) - par,
          "with an FF stream", sum(c["ff"] for c in longs))
    assert len(longs) >= tr.FLOORS["actions"]["long"] * len(ACTION_SEEDS) // tr.NPROG, len(longs)
    assert 3 * par >= len(longs) and len(longs) - par >= 5, (len(longs), par)


# ----------------------------------------------------------------------------------------------------------- d. batch
BATCH_SEEDS = range(0, tr.NPROG, 4)


def batch_docs(kind, seed):
    """about 200 documents: accepted samples of target lengths 0 to 700 and, for every fourth, its rejected variants"""
    import random
    r = random.Random(seed * 31 + 5)
    docs = []
    for k in range(130):
        t = r.randrange(701)
        docs.append(tr.sample(kind, seed, t))
        if k % 4 == 0:
            docs += tr.variants(kind, seed, t)[:3]
    r.shuffle(docs)
    return docs


@pytest.mark.parametrize("part", range(3))
def test_batch_on_generated_programs(part):
    nprog = 0
    for seed in BATCH_SEEDS[part::3]:
        src = tr.source("plain", seed)
        if src is None:
            continue
        p = load(src)
        if p is None:
            continue
        try:
            docs = batch_docs("plain", seed)
            accepted = sum(isinstance(tr.expect("plain", seed, d), bytes) for d in docs)
            assert 2 * accepted > len(docs), (seed, accepted, len(docs))
            _check(blob_of(src, 3), docs, p.run_batch(docs))
            nprog += 1
        finally:
            p.close()
    assert nprog >= 5, nprog


@pytest.mark.parametrize("part", range(3))
def test_batch_on_generated_action_programs(part):
    """batch_actions = 2 (the batch replay) against the oracle, and batch_actions = 1 (every document takes the single-document route)
    with identical arrays"""
    nprog = 0
    for seed in BATCH_SEEDS[part::3]:
        src = tr.source("actions", seed)
        if src is None:
            continue
        replay, route = load(src, batch_actions=2), load(src, batch_actions=1)
        if replay is None or route is None:
            continue
        try:
            docs = batch_docs("actions", seed)
            accepted = sum(isinstance(tr.expect("actions", seed, d), bytes) for d in docs)
            assert 2 * accepted > len(docs), (seed, accepted, len(docs))
            got = _arrays(replay, docs)
            assert _check_arrays(blob_of(src, 3), docs, got) == accepted
            assert _arrays(route, docs) == got, (seed, src)
            nprog += 1
        finally:
            replay.close()
            route.close()
    assert nprog >= 5, nprog
