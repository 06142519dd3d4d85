"""CPU: what the stage loader builds (kx_stage.h, through kx_stage_describe_cfg) is byte for byte what the fixture holds.

tests/golden/stage_images.json holds, per case, the SHA-256 of each of a stage's four device allocations (main tables, job-stride
alternative, delayed form, slow-path tables) and every field of kx_stage_info.  A case is one stage of a program under one
configuration.  The file was recorded from the loader as it was BEFORE it was split into steps, so equality here says that the
split moved no byte.  `python tests/test_stage_image.py --write` records it again from the current build: for the day a layout is
changed on purpose, never to make this test pass.
"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import randprog                                                                   # noqa: E402
from conftest import GOLDEN, blob_of, dictionary_program                          # noqa: E402
from kleenexlang_amd import compile_file, host                                    # noqa: E402
from test_delayed_form import many_classes_program                                # noqa: E402
from test_dfrec8 import maxima_programs                                           # noqa: E402
from test_instances import CLASSES_PROGRAM, INLINE_PROGRAM, LEAVES_PROGRAM, WIDE_ENTRY_PROGRAM, wide_k2_program   # noqa: E402

FIXTURE = os.path.join(GOLDEN, "stage_images.json")
WHICH = (host.KX_STAGE_MAIN, host.KX_STAGE_ALT, host.KX_STAGE_DELAYED, host.KX_STAGE_SLOW)
EXAMPLES = os.path.join(os.path.dirname(host.PROGRAM_DIR), "examples")
PIPELINE = 'start: p >> a >> b\np := (~/abc/ "a")*\na := (/./ "b")*\nb := (/ab/ "c" | ~/[^ab]/ "lol")*\n'      # (three stages)
ACTIONS = 'main := [acc <- ""] (word)* "=" !acc\nword := w@/[a-z]+/ [acc += w "+"] ~/ /\n'                    # (a stage with register actions)
LONG_CONSTANT = 'main := (~/a/ "%s" | /b/)*\n' % ("z" * 127)                                                  # (a path constant of 127 bytes)
CODERS = {"coder": "([a-c]*|[0-9]+)(,|;)?x*",             # (compile_regex: symbol tables beside plain copies, per-entry table ids)
          "coder_rows": "(([^,\\n]*),([^,\\n]*)\\n)*"}      # (one table on every copying entry: translated once per piece)
RANDOM_SEEDS = range(20)


def programs():
    """name -> blob"""
    out = {}
    for name in ("add_commas", "apache_log", "csv2json", "flip_ab", "iso_datetime_to_json", "thousand_sep"):
        out[name] = blob_of(name)
    for name in ("csv_escaped", "csv_rfc4180", "fields_to_json", "paragraphs"):
        out["examples/" + name] = compile_file(os.path.join(EXAMPLES, name + ".kex"))
    out["pipeline"], out["actions"] = blob_of(PIPELINE), blob_of(ACTIONS)
    out["many_classes"], out["wide_k2"] = blob_of(many_classes_program(2)[0]), blob_of(wide_k2_program()[0])
    for name, src in maxima_programs().items():
        out["maxima_" + name] = blob_of(src)
    out["leaves"], out["inline"], out["classes"], out["wide_entry"] = (blob_of(p) for p in (LEAVES_PROGRAM, INLINE_PROGRAM, CLASSES_PROGRAM, WIDE_ENTRY_PROGRAM))
    out["dictionary_opt0"] = blob_of(dictionary_program()[0], opt=0)
    for name, regex in CODERS.items():
        out[name] = host.compile_regex(regex)
    out["long_constant"] = blob_of(LONG_CONSTANT)
    for seed in RANDOM_SEEDS:
        out["random_%d" % seed] = blob_of(randprog.program_wide(seed) if seed % 2 else randprog.program(seed))
    return out


def variants(name):
    """the kx_config fields a program is crossed with (one group of switches at a time)"""
    out = [{"delayed_form": a, "delay": b} for a in (0, 1, 2) for b in (0, 1, 2)]                # (the first: all defaults)
    out += [{"merge_window": m} for m in (1, 3)]
    out += [{"inline_consts": a, "job_stride": b} for a in (0, 1, 2) for b in (0, 1, 2) if a or b]
    out += [{"disable": bit} for bit in (host.KX_OFF_DIRECT, host.KX_OFF_PAIR, host.KX_OFF_CMPX, host.KX_OFF_SLOW)]
    out += [{"force": host.KX_FORCE_BIG}]
    if name in CODERS:
        out += [dict(v, force=v.get("force", 0) | host.KX_FORCE_TBLMODE) for v in list(out)]
    return out


def observe(blob, stage, fields):
    """one case: {"sha": [4], "bytes": [4], "info": {...}, "alt": {...} or None}"""
    cfg = host.KxConfig(**fields)
    sha, size, infos = [], [], []
    for w in WHICH:
        if w and not infos[0][("has_alt", "has_df", "d.sl_on")[w - 1]]:        # (the stage has no such allocation: nothing more to ask)
            sha.append(""); size.append(0); infos.append(infos[0])
            continue
        info, img = host.stage_describe(blob, stage, w, cfg)
        assert info.image_bytes == (len(img) if img else 0)
        sha.append(hashlib.sha256(img).hexdigest() if img else "")
        size.append(int(info.image_bytes))
        d = info.as_dict()
        del d["image_bytes"]
        infos.append(d)
    assert infos[2] == infos[0] and infos[3] == infos[0]                  # (the report differs by `which` only for the alternative's tables)
    assert (size[1] > 0) == bool(infos[0]["has_alt"]) and (size[2] > 0) == bool(infos[0]["has_df"]) and (size[3] > 0) == bool(infos[0]["d.sl_on"])
    assert {k: v for k, v in infos[1].items() if not k.startswith("t.")} == {k: v for k, v in infos[0].items() if not k.startswith("t.")}
    alt = {k: v for k, v in infos[1].items() if k.startswith("t.")} if infos[0]["has_alt"] else None
    return {"sha": sha, "bytes": size, "info": infos[0], "alt": alt}


def all_cases():
    """case id -> observation, over the whole list"""
    import struct
    out = {}
    for name, blob in programs().items():
        for stage in range(struct.unpack_from("<I", blob, 12)[0]):
            for fields in variants(name):
                cid = "%s/%d/%s" % (name, stage, ",".join("%s=%d" % kv for kv in sorted(fields.items())))
                out[cid] = observe(blob, stage, fields)
    return out


def flat(cases):
    """observations with field names taken out: (field names, alternative's field names, case id -> {sha, bytes, info, alt} of lists)"""
    names = list(next(iter(cases.values()))["info"])
    tnames = [k for k in names if k.startswith("t.")]
    return names, tnames, {cid: {"sha": c["sha"], "bytes": c["bytes"], "info": [c["info"][k] for k in names],
                                 "alt": [c["alt"][k] for k in tnames] if c["alt"] else None} for cid, c in cases.items()}


def pack(cases):
    """the fixture's form.  Nothing is left out, repetition is: a digest is an index into "digests"; per stage ("name/stage") the
    first configuration (all defaults) is written in full, every other one as what differs from it ("info" as {field index: value}),
    and configurations that gave the same share one entry, their names joined by blanks"""
    names, tnames, obs = flat(cases)
    digests = sorted({d for c in obs.values() for d in c["sha"]})
    stages = {}
    for cid, c in obs.items():
        key, variant = cid.rsplit("/", 1)
        c = dict(c, sha=[digests.index(d) for d in c["sha"]])
        base = stages.setdefault(key, [[variant], c])[1]
        if c is base:
            continue
        delta = {k: c[k] for k in ("sha", "bytes", "alt") if c[k] != base[k]}
        changed = {str(i): v for i, v in enumerate(c["info"]) if v != base["info"][i]}
        delta = dict(delta, info=changed) if changed else delta
        for group in [stages[key]] + stages[key][2:]:
            if group[1] == (delta or base):
                group[0].append(variant)
                break
        else:
            stages[key].append([[variant], delta])
    return {"fields": names, "alt_fields": tnames, "digests": digests,
            "stages": {key: dict([(" ".join(g[0]), g[1])] + [(" ".join(v), d) for v, d in g[2:]]) for key, g in stages.items()}}


def unpack(fixture):
    """pack() undone: (field names, alternative's field names, case id -> {sha, bytes, info, alt})"""
    obs = {}
    for key, groups in fixture["stages"].items():
        base = next(iter(groups.values()))
        for variants, delta in groups.items():
            c = dict(base, **{k: v for k, v in delta.items() if k != "info"})
            c["info"] = list(base["info"])
            if delta is not base:
                for i, v in delta.get("info", {}).items():
                    c["info"][int(i)] = v
            c["sha"] = [fixture["digests"][i] for i in c["sha"]]
            obs.update(("%s/%s" % (key, variant), c) for variant in variants.split(" "))
    return fixture["fields"], fixture["alt_fields"], obs


_SEEN = {}


def seen():
    if not _SEEN:
        _SEEN.update(all_cases())
    return _SEEN


def test_every_image_and_every_field_is_what_the_fixture_holds():
    with open(FIXTURE) as f:
        want = json.load(f)
    assert unpack(pack(seen())) == flat(seen())                      # (the fixture's form loses nothing)
    names, tnames, got = flat(seen())
    want_names, want_tnames, want = unpack(want)
    assert names == want_names and tnames == want_tnames
    assert sorted(got) == sorted(want)
    for cid, c in want.items():
        assert got[cid] == c, cid


def test_the_case_list_reaches_every_layout():
    """identity protects only what some case builds: each fact below holds in at least one case and fails in at least one"""
    facts = {
        "general": lambda i: i["general"], "big": lambda i: i["big"], "inl": lambda i: i["t.inl"], "jl": lambda i: i["t.jl"],
        "direct": lambda i: i["t.direct"], "tblmode": lambda i: i["t.tblmode"], "xlat": lambda i: i["t.xlat"] != 0,
        "pair table": lambda i: i["t.pair_words"] > 0, "cshift 2": lambda i: i["t.cshift"] == 2, "short_consts": lambda i: i["t.short_consts"],
        "alternative": lambda i: i["has_alt"], "delayed K=1": lambda i: i["has_df"] and i["d.K"] == 1, "delayed K=2": lambda i: i["has_df"] and i["d.K"] == 2,
        "no delayed form": lambda i: not i["has_df"], "wide delayed form": lambda i: i["d.wide"], "slow path": lambda i: i["d.sl_on"],
        "actions": lambda i: i["actions"]}
    for name, fact in facts.items():
        values = {bool(fact(c["info"])) for c in seen().values()}
        assert values == {True, False}, (name, values)
    assert any(c["alt"] and c["alt"]["t.jl"] for c in seen().values())


def test_corrupt_blobs_go_through_the_host_builder_clean_under_a_sanitizer(tmp_path):
    """tests/native/stage_fuzz.cpp: the truncations and mutations of test_abi's corrupt-blob test through every step of kx_stage.h, in
    a stand-alone program built with AddressSanitizer and UBSan (a CPU machine's job: skipped where a GPU is present)"""
    import subprocess as sp
    import pytest
    import torch
    from kleenexlang_amd import build, program_path
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = str(tmp_path / "stage_fuzz")
    sp.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
            os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "stage_fuzz.cpp")], check=True)
    kexc = os.path.join(build.OUT, "kexc")
    for name in ("flip_ab", "csv2json", "apache_log", "coder"):
        blob = str(tmp_path / (name + ".kxp"))
        source = ["--re", CODERS["coder"]] if name == "coder" else [program_path(name)]
        sp.run([kexc, "compile", "--quiet", "--blob", blob, *source, "--out", str(tmp_path / name)], check=True)
        r = sp.run([exe, blob], stdout=sp.PIPE, stderr=sp.PIPE)
        assert r.returncode == 0, (name, r.stdout[-400:], r.stderr[-3000:])


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_stage_image.py --write")
    recorded = pack(all_cases())
    with open(FIXTURE, "w") as f:
        one = lambda v: json.dumps(v, separators=(",", ":"))                     # (one line per stage: a change shows where it is)
        f.write("{%s,\n\"stages\":{\n%s\n}}\n" % (",\n".join("%s:%s" % (one(k), one(recorded[k])) for k in ("fields", "alt_fields", "digests")),
                                                  ",\n".join("%s:%s" % (one(k), one(v)) for k, v in recorded["stages"].items())))
    print("%s: %d cases" % (FIXTURE, len(unpack(recorded)[2])))
