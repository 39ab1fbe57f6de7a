"""The zstd decoder's host launch policy (zarrs_amd/csrc/zstd_launch.cpp) on the CPU: a small C++ program
(tests/c/zstd_launch_harness.cpp) linked to libzgpu.so calls zstd_scratch_sizes and zstd_launch_policy on
each case; every field is held to the model (tests/zstd_launch_model.py), which is written from DESIGN's
table, and to the figures each case states outright. Every case names the branches of zstd_launch.cpp it
reaches (function:branch); BRANCHES lists them all and a branch without a case fails. The compute-unit
count is an input: 256 (an MI355X) and 64."""
import itertools
import json
import os
import subprocess

import pytest

import zstd_frames as Z
import zstd_launch_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "zarrs_amd", "lib")
CSRC = os.path.join(ROOT, "zarrs_amd", "csrc")
SRC = os.path.join(CSRC, "zstd_launch.cpp")
KIB, MIB = 1 << 10, 1 << 20

BRANCHES = """
window_executors:sparse window_executors:full window_executors:forced-on window_executors:forced-off
zstd_latency_possible:yes zstd_latency_possible:past-limit zstd_latency_possible:xpar-off
ext_rounds:log2
zstd_scratch_sizes:ext zstd_scratch_sizes:ext-not-wanted zstd_scratch_sizes:ext-not-possible zstd_scratch_sizes:alias
zstd_scratch_sizes:lit-stride-floor zstd_scratch_sizes:lit-stride-slot zstd_scratch_sizes:blk-cap-limit
zstd_launch_policy:latency zstd_launch_policy:window zstd_launch_policy:window-no-ext zstd_launch_policy:wave-wide
zstd_launch_policy:wave-dense zstd_launch_policy:dense-forced zstd_launch_policy:wide-forced
zstd_launch_policy:fork zstd_launch_policy:lits-first zstd_launch_policy:lits-first-under-fork
zstd_launch_policy:lit-direct zstd_launch_policy:alias-no-direct
zstd_launch_policy:rec-passed zstd_launch_policy:rec-withheld
zstd_launch_policy:grids-by-cus zstd_launch_policy:grids-by-records
zstd_launch_policy:serial-per-item zstd_launch_policy:serial-listed zstd_launch_policy:serial-skipped
zstd_knobs_from_env:unset zstd_knobs_from_env:set
""".split()


def case(n, slot=4 * KIB, cus=256, wants=None, caps=None, **knobs):
    """A plan's own stage by default: the latency mode wanted, no aliases, one stream, the serial list."""
    assert set(knobs) <= set(M.KNOBS)
    return {"n_items": n, "slot": slot, "cus": cus, "knobs": {**M.KNOBS, **knobs},
            "wants": {"alias": 0, "latency": 1, **(wants or {})}, "caps": dict(caps or {})}


BLOSC = {"alias": 1, "latency": 0}  # the blosc stage's wants
# name, the branches it reaches, the case, figures stated outright (sizes' and launch's fields by name)
CASES = [
    # executor choice, no knobs, 256 CUs
    ("n1", "window_executors:sparse zstd_latency_possible:yes zstd_launch_policy:latency zstd_scratch_sizes:ext "
     "zstd_launch_policy:grids-by-records zstd_launch_policy:lit-direct zstd_launch_policy:rec-passed ext_rounds:log2",
     case(1), {"executor": "LATENCY", "xseg": 8, "rounds": 8, "persist_grid": 256, "round_grid": 4, "grid": 64, "lgrid": 64,
               "bgrid": 64, "ext": 8 * 4096, "ext_cnt": 8 * 24, "lit_direct": 1, "rec_slots": 1}),
    ("n341", "zstd_launch_policy:latency", case(341), {"executor": "LATENCY", "xseg": 8}),
    ("n342", "window_executors:full zstd_launch_policy:wave-wide zstd_scratch_sizes:ext-not-possible "
     "zstd_launch_policy:grids-by-cus",
     case(342), {"executor": "WAVE_WIDE", "xseg": 12, "ext": 0, "ext_cnt": 0, "rounds": 0, "grid": 4096, "lgrid": 1024,
                 "bgrid": 6144}),
    ("n1365", "zstd_launch_policy:wave-wide", case(1365), {"executor": "WAVE_WIDE", "xseg": 12}),  # 1365 x 12 < 256 x 64
    ("n1366", "zstd_launch_policy:wave-dense", case(1366), {"executor": "WAVE_DENSE", "xseg": 12}),
    # the same edges on 64 CUs: (4 * 64 - 1) // 3 = 85; 342 x 12 >= 64 x 64 > 341 x 12
    ("cu64-n85", "zstd_launch_policy:latency", case(85, cus=64), {"executor": "LATENCY", "persist_grid": 64, "lit_rec_wgs": 256}),
    ("cu64-n86", "zstd_launch_policy:wave-wide zstd_launch_policy:grids-by-cus", case(86, cus=64),
     {"executor": "WAVE_WIDE", "grid": 1024, "lgrid": 256, "bgrid": 1536}),
    ("cu64-n341", "zstd_launch_policy:wave-wide", case(341, cus=64), {"executor": "WAVE_WIDE"}),
    ("cu64-n342", "zstd_launch_policy:wave-dense", case(342, cus=64), {"executor": "WAVE_DENSE"}),
    # latency needs its scratch
    ("128mib", "zstd_latency_possible:yes", case(128, MIB), {"executor": "LATENCY", "ext": 1 << 30}),
    ("128mib-and-a-slot", "zstd_latency_possible:past-limit zstd_launch_policy:window zstd_scratch_sizes:ext-not-possible",
     case(129, MIB), {"executor": "WINDOW", "xseg": 8, "ext": 0}),
    ("past-limit-with-ext", "zstd_latency_possible:past-limit zstd_launch_policy:window",
     case(129, MIB, caps={"ext": 1}), {"executor": "WINDOW"}),
    ("no-ext", "zstd_launch_policy:window-no-ext", case(1, caps={"ext": 0}), {"executor": "WINDOW", "xseg": 8, "rounds": 0}),
    ("blosc-few", "zstd_scratch_sizes:ext-not-wanted zstd_scratch_sizes:alias zstd_launch_policy:window-no-ext "
     "zstd_launch_policy:alias-no-direct", case(8, 32 * KIB, wants=BLOSC),
     {"executor": "WINDOW", "ext": 0, "alias": 8 * 48, "lit_direct": 0}),
    ("xpar-0", "zstd_latency_possible:xpar-off zstd_launch_policy:window", case(1, xpar=0), {"executor": "WINDOW", "ext": 0}),
    ("xpar-0-with-ext", "zstd_latency_possible:xpar-off", case(1, caps={"ext": 1}, xpar=0), {"executor": "WINDOW"}),
    ("xwin-0-n1", "window_executors:forced-off zstd_launch_policy:wave-wide", case(1, xwin=0),
     {"executor": "WAVE_WIDE", "xseg": 12, "ext": 0}),
    ("xwin-1-n5000", "window_executors:forced-on zstd_launch_policy:latency", case(5000, xwin=1),
     {"executor": "LATENCY", "xseg": 8, "ext": 8 * 5000 * 4096}),
    ("xwin-1-n5000-32k", "window_executors:forced-on zstd_launch_policy:window", case(5000, 32 * KIB, xwin=1),
     {"executor": "WINDOW", "ext": 0}),
    ("xdense-0", "zstd_launch_policy:wide-forced", case(5000, xdense=0), {"executor": "WAVE_WIDE"}),
    ("xdense-1", "zstd_launch_policy:dense-forced", case(342, xdense=1), {"executor": "WAVE_DENSE"}),
    ("xdense-1-under-window", "zstd_launch_policy:latency", case(1, xdense=1), {"executor": "LATENCY"}),
    ("2000x64k", "zstd_scratch_sizes:ext-not-possible zstd_launch_policy:wave-dense", case(2000, 64 * KIB),
     {"executor": "WAVE_DENSE", "ext": 0, "ext_cnt": 0}),
    # rounds, as DESIGN states them
    ("rounds-8mib", "ext_rounds:log2", case(1, 8 * MIB), {"executor": "LATENCY", "rounds": 13}),
    ("rounds-128mib", "ext_rounds:log2", case(1, 128 * MIB), {"executor": "LATENCY", "rounds": 17, "round_grid": 4096}),
    # stream shape
    ("fork", "zstd_launch_policy:fork", case(342, caps={"side": 1}), {"fork": 1, "lits_first": 0, "lit_direct": 0}),
    ("lits-first", "zstd_launch_policy:lits-first", case(342, caps={"lits_first": 1}), {"fork": 0, "lits_first": 1, "lit_direct": 0}),
    ("lits-first-under-fork", "zstd_launch_policy:lits-first-under-fork", case(342, caps={"side": 1, "lits_first": 1}),
     {"fork": 1, "lits_first": 0, "lit_direct": 0}),
    ("one-stream", "zstd_launch_policy:lit-direct", case(342), {"fork": 0, "lits_first": 0, "lit_direct": 1}),
    ("blosc-many", "zstd_launch_policy:alias-no-direct zstd_launch_policy:fork zstd_launch_policy:wave-dense",
     case(4096, 256 * KIB, wants=BLOSC, caps={"side": 1}), {"executor": "WAVE_DENSE", "fork": 1, "lit_direct": 0}),
    ("alias-one-stream", "zstd_launch_policy:alias-no-direct", case(342, wants=BLOSC), {"fork": 0, "lit_direct": 0}),
    ("blosc-no-alias", "zstd_launch_policy:lit-direct", case(342, wants={"alias": 0, "latency": 0}), {"alias": 0, "lit_direct": 1}),
    # record slots: passed while the literal grid fits the workgroups they were sized for
    ("rec-exact", "zstd_launch_policy:rec-passed", case(342, caps={"lit_rec_wgs": 1024}), {"lgrid": 1024, "rec_slots": 1}),
    ("rec-one-short", "zstd_launch_policy:rec-withheld", case(342, caps={"lit_rec_wgs": 1023}), {"lgrid": 1024, "rec_slots": 0}),
    ("rec-none", "zstd_launch_policy:rec-withheld", case(1, caps={"lit_rec_wgs": 0}), {"lgrid": 64, "rec_slots": 0}),
    # serial fallback
    ("serial-unlisted", "zstd_launch_policy:serial-per-item", case(5000, caps={"ser_list": 0}),
     {"serial": "PER_ITEM", "serial_grid": 5000}),
    ("serial-listed", "zstd_launch_policy:serial-listed", case(5000), {"serial": "LISTED", "serial_grid": 1024}),
    ("serial-listed-few", "zstd_launch_policy:serial-listed", case(3, cus=64), {"serial": "LISTED", "serial_grid": 3}),
    ("serial-skipped", "zstd_launch_policy:serial-skipped", case(5000, caps={"launch_serial": 0}),
     {"serial": "NONE", "serial_grid": 0}),
    # scratch sizes: the slots at which the capacities change form
    ("slot-256", "zstd_scratch_sizes:lit-stride-floor", case(3, 256),
     {"blk_cap": 64, "lit_stride": 147712, "seq_cap": 1088, "blks": 3 * 64 * 160, "norm": 3 * 64 * 384, "nblk": 12, "mode": 12,
      "ser_list": 12, "lit": 3 * 147712, "seq": 3 * 1088 * 12, "lit_rec": 1024 * 256 * 1088, "lit_rec_wgs": 1024}),
    ("slot-4k", "zstd_scratch_sizes:lit-stride-floor", case(3, 4 * KIB), {"blk_cap": 64, "lit_stride": 147712, "seq_cap": 2048}),
    ("slot-32k-256", "zstd_scratch_sizes:lit-stride-floor", case(3, 32 * KIB - 256), {"blk_cap": 64, "seq_cap": 8128 + 1024}),
    ("slot-32k", "zstd_scratch_sizes:lit-stride-floor", case(3, 32 * KIB), {"blk_cap": 65, "seq_cap": 8192 + 1024}),
    ("slot-16m", "zstd_scratch_sizes:lit-stride-slot", case(3, 16 * MIB),
     {"blk_cap": 576, "lit_stride": 18 * MIB, "seq_cap": 4 * MIB + 1024, "seq": 3 * (4 * MIB + 1024) * 12}),
    ("slot-64g", "zstd_scratch_sizes:blk-cap-limit", case(1, 64 << 30), {"blk_cap": 1 << 20, "executor": "WINDOW"}),
]
IDS = [c[0] for c in CASES]
SCRATCH_SLOTS = [256, 4 * KIB, 32 * KIB - 256, 32 * KIB, 16 * MIB]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("zstd_launch") / "zstd_launch_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "c", "zstd_launch_harness.cpp"), "-L" + LIB, "-lzgpu",
                           "-Wl,-rpath," + LIB])
    return exe


def run(exe, cases):
    r = subprocess.run([exe] + [json.dumps(c) for c in cases], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


def caps_of(c, S):
    """The caps the harness fills in: what the case's own sizes provide where the case does not say."""
    return {"side": 0, "alias": int(S["alias"] != 0), "lits_first": 0, "ext": int(S["ext"] != 0),
            "lit_rec_wgs": S["lit_rec_wgs"], "ser_list": 1, "launch_serial": 1, **c["caps"]}


def test_every_branch_has_a_case():
    reached = {t for _, tags, _, _ in CASES for t in tags.split()} | {"zstd_knobs_from_env:unset", "zstd_knobs_from_env:set"}
    assert sorted(set(BRANCHES) - reached) == [] and sorted(reached - set(BRANCHES)) == []
    assert len(set(IDS)) == len(IDS)
    src = open(SRC).read()
    for t in BRANCHES:  # every tag names a function of zstd_launch.cpp
        assert " " + t.split(":")[0] + "(" in src, t
    assert {c[2]["cus"] for c in CASES} == {256, 64}


def test_headers_need_no_hip(tmp_path):
    """zstd_launch.hpp and kernels/zstd_params.hpp compile with plain g++ and no ROCm include path."""
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "%s"\nint main() { return 0; }\n' % os.path.join(CSRC, "zstd_launch.hpp"))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(probe)])


def test_the_environment_is_read_in_one_place():
    """ZGPU_ZSTD_* names a variable in one .cpp / .hip / .inc under csrc only, zstd_launch.cpp, and four of them."""
    import re
    found = {}
    for d, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith((".cpp", ".hip", ".inc")):
                names = set(re.findall(r'"(ZGPU_ZSTD_\w+)"', open(os.path.join(d, f)).read()))
                if names:
                    found[f] = names
    assert found == {"zstd_launch.cpp": {"ZGPU_ZSTD_XWIN", "ZGPU_ZSTD_XPAR", "ZGPU_ZSTD_XDENSE", "ZGPU_ZSTD_FORCE_SERIAL"}}
    assert "getenv" not in open(os.path.join(CSRC, "kernels", "zstd.hip")).read()


@pytest.mark.parametrize("env,want", [
    ({}, {"xwin": -1, "xpar": 1, "xdense": -1, "force_serial": 0}),
    ({"ZGPU_ZSTD_XWIN": "0", "ZGPU_ZSTD_XPAR": "0", "ZGPU_ZSTD_XDENSE": "1", "ZGPU_ZSTD_FORCE_SERIAL": "1"},
     {"xwin": 0, "xpar": 0, "xdense": 1, "force_serial": 1}),
    ({"ZGPU_ZSTD_XWIN": "1", "ZGPU_ZSTD_XPAR": "1", "ZGPU_ZSTD_XDENSE": "0", "ZGPU_ZSTD_FORCE_SERIAL": "0"},
     {"xwin": 1, "xpar": 1, "xdense": 0, "force_serial": 0}),
    ({"ZGPU_ZSTD_XWIN": "-1", "ZGPU_ZSTD_XDENSE": "-1"}, {"xwin": -1, "xpar": 1, "xdense": -1, "force_serial": 0}),
], ids=["unset", "set-a", "set-b", "minus-one"])
def test_knobs_from_env(harness, env, want):
    e = {k: v for k, v in os.environ.items() if not k.startswith("ZGPU_ZSTD_")}
    r = subprocess.run([harness, "env"], capture_output=True, text=True, timeout=60, env={**e, **env})
    assert r.returncode == 0 and json.loads(r.stdout) == want


@pytest.mark.parametrize("name,tags,c,stated", CASES, ids=IDS)
def test_policy_matches_the_model(harness, name, tags, c, stated):
    J = run(harness, [c])[0]
    S, L = J["sizes"], J["launch"]
    for k, v in stated.items():
        assert (S[k] if k in S else L[k]) == v, k
    n, slot, cus, knobs = c["n_items"], c["slot"], c["cus"], c["knobs"]
    assert S == M.sizes(n, slot, cus, c["wants"], knobs)
    assert L == M.launch(n, slot, cus, caps_of(c, S), knobs)
    assert J["latency_possible"] == M.latency_possible(n, slot, cus, knobs)
    # what holds for every case: the window executors cut 8 segments, the wave executors 12; the grids' caps
    assert L["xseg"] == (8 if L["executor"] in ("LATENCY", "WINDOW") else 12)
    recs = n * S["blk_cap"]
    assert L["grid"] == min(recs, cus * 16) and L["lgrid"] == min(recs, cus * 4)
    assert L["bgrid"] == min(recs, max(cus * 16, cus * 4 * 6))
    caps = caps_of(c, S)
    assert L["fork"] == caps["side"] and (not L["lits_first"] or not L["fork"])
    assert L["lit_direct"] == int(not L["fork"] and not caps["alias"] and not L["lits_first"])
    assert L["rec_slots"] == int(L["lgrid"] <= caps["lit_rec_wgs"])
    assert L["rounds"] <= M.ZEXT_ROUNDS and (L["rounds"] > 0) == (L["executor"] == "LATENCY")


def test_one_predicate_sizes_and_selects_the_latency_mode(harness):
    """ext_bytes > 0 exactly when the policy, given ext arrays, takes the latency mode for those inputs; with
    the sizes' own ext the executor is then LATENCY, and never without. 2,000 items of 64 KiB hold no ext."""
    pts = []
    for n, slot, xwin, xpar, cus in itertools.product([1, 85, 86, 341, 342, 2000, 5000], [256, 4 * KIB, 64 * KIB, MIB, 16 * MIB],
                                                      [-1, 0, 1], [1, 0], [256, 64]):
        pts.append(case(n, slot, cus, xwin=xwin, xpar=xpar))
    assert len(pts) >= 200
    own = run(harness, pts)
    given = run(harness, [{**c, "caps": {"ext": 1}} for c in pts])
    seen = set()
    for c, a, b in zip(pts, own, given):
        has = a["sizes"]["ext"] > 0
        assert has == (b["launch"]["executor"] == "LATENCY") == (a["launch"]["executor"] == "LATENCY"), c
        assert has == bool(a["latency_possible"]) == M.latency_possible(c["n_items"], c["slot"], c["cus"], c["knobs"]), c
        assert a["sizes"]["ext"] == (8 * c["n_items"] * c["slot"] if has else 0)
        seen.add(has)
    assert seen == {True, False}
    J = run(harness, [case(2000, 64 * KIB)])[0]
    assert J["sizes"]["ext"] == 0 and J["sizes"]["ext_cnt"] == 0


@pytest.mark.parametrize("slot", SCRATCH_SLOTS)
@pytest.mark.parametrize("cus", [256, 64])
def test_scratch_sizes(harness, slot, cus):
    """Every capacity by its rule, every buffer's bytes, and the frame builders' mirror (zstd_frames.layout)."""
    n = 5
    S = run(harness, [case(n, slot, cus, wants={"alias": 1, "latency": 1})])[0]["sizes"]
    assert S["blk_cap"] == min(slot // 32768 + 64, 1 << 20)
    floor = 131072 + 64 + 2 * Z.HUF_TAB
    assert S["lit_stride"] == -(-max(slot + slot // 8, floor) // 256) * 256 and S["lit_stride"] % 256 == 0
    assert S["seq_cap"] == slot // 4 + 1024
    assert (S["blk_cap"], S["lit_stride"], S["seq_cap"]) == Z.layout(slot)
    assert S["lit_rec_wgs"] == cus * 4
    want = {"blks": n * S["blk_cap"] * 160, "norm": n * S["blk_cap"] * 3 * 64 * 2, "nblk": 4 * n, "mode": 4 * n,
            "lit": n * S["lit_stride"], "seq": n * S["seq_cap"] * 3 * 4, "ser_list": 4 * n,
            "lit_rec": cus * 4 * 256 * (1024 + 64), "alias": n * 3 * 2 * 8, "ext": 2 * n * slot * 4, "ext_cnt": 24 * 8}
    assert {k: S[k] for k in want} == want
    assert len(want) == 11  # every buffer of ZstdScratch


def test_wspan_mirror():
    """zstd_frames.WSPAN restates xwin::WSPAN of kernels/zstd_params.hpp (the round rule's divisor)."""
    import re
    src = open(os.path.join(CSRC, "kernels", "zstd_params.hpp")).read()
    cells = int(re.search(r"CELLS = (\d+);", src).group(1))
    assert "W = CELLS - 16;" in src and "WSPAN = W - 16;" in src and Z.WSPAN == cells - 32
