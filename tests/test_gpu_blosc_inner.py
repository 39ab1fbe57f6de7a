"""The zstd and zlib streams inside blosc frames on the GPU, on hand-built frames
(tests/blosc_inner_streams.py; c-blosc referees every case on the CPU, tests/test_blosc_inner_model.py): the
blosc stage's own zstd pipeline (a second ZstdScratch with block aliases, slots of sub_slot bytes, the
other compressors' streams as skipped entries of its table) with k_zstd_plan's alias rule at every
boundary and k_blosc_finish's readers of aliased blocks (the u16 / u32 plane fast path, the byte loop,
bitunshuffle, split and leftover blocks) at every plane relation; and k_gzip<true>, the blosc stage's
instantiation of the DEFLATE decoder, on every hand-built DEFLATE stream.

The harness is test_gpu_blosc_frames.Call: one plan per family, path and chunk size, executed twice (the
second execution lays the stream table out with k_blosc_layout), the output prefilled with a sentinel,
guard and tail checked, frames at unaligned offsets. Asserted per execution: every status (0, or
CORRUPT_STREAM where c-blosc refuses the frame), the return code (the first failing status), every
valid chunk bit-exact beside the corrupt ones, and the counters: zstd_serial + zstd_parallel is the
number of zstd streams with the cases' `parallel` intent honoured, zstd_latency is 0 (the blosc stage
never takes the latency mode), and blosc_aliased is the number of alias entries the restated rule
gives the call's streams; 0 with ZGPU_BLOSC_ALIAS=0 and on the forced serial decoder. Without that
counter a call that aliased nothing at all, or one block too many whose bytes an earlier call left in
the reused slot, would pass on its bytes alone.

Paths of the zstd families: the window executor, the wave executor wide and dense, and the forced
serial decoder, each with aliases on and off, on direct rows; slot rows (ZGPU_BLOSC_NO_DIRECT) with
aliases on and off; host input once. zlib_wrapped: direct rows, slot rows, host input, and the lookahead
decode (ZGPU_GZIP_SEG=0) in a child process.

Cases per family: zstd_wrapped 94, alias_planes 66, alias_rule 23, alias_layouts 49, zlib_wrapped 263
(35 corrupt), sizes 12 (8 of a wrong size), mixed 5."""
import json
import os
import subprocess
import sys

import pytest

import blosc_inner_streams as I

pytestmark = pytest.mark.gpu

ENV_VARS = ["ZGPU_ZSTD_XWIN", "ZGPU_ZSTD_XPAR", "ZGPU_ZSTD_XDENSE", "ZGPU_ZSTD_FORCE_SERIAL", "ZGPU_BLOSC_ALIAS",
            "ZGPU_BLOSC_NO_DIRECT", "ZGPU_GZIP_SEG"]
EXECUTORS = {
    "window": {"ZGPU_ZSTD_XWIN": "1", "ZGPU_ZSTD_XPAR": "0"},
    "wave": {"ZGPU_ZSTD_XWIN": "0", "ZGPU_ZSTD_XDENSE": "0"},
    "wave_dense": {"ZGPU_ZSTD_XWIN": "0", "ZGPU_ZSTD_XDENSE": "1"},
    "serial": {"ZGPU_ZSTD_FORCE_SERIAL": "1"},
}
NOALIAS = {"ZGPU_BLOSC_ALIAS": "0"}
ZSTD_PATHS = {f"{e}-{a}": dict(env, **(NOALIAS if a == "noalias" else {})) for e, env in EXECUTORS.items()
              for a in ("alias", "noalias")}
ZSTD_PATHS["slot_rows-alias"] = {"ZGPU_BLOSC_NO_DIRECT": "1"}
ZSTD_PATHS["slot_rows-noalias"] = dict(NOALIAS, ZGPU_BLOSC_NO_DIRECT="1")
ZSTD_PATHS["host-alias"] = {}
ZLIB_PATHS = {"direct_rows": {}, "slot_rows": {"ZGPU_BLOSC_NO_DIRECT": "1"}, "host": {}}


def _harness():
    import test_gpu_blosc_frames as H  # the Call harness, shared (imported late: it imports torch lazily too)
    return H


def _by_size(cases):
    g = {}
    for c in cases:
        g.setdefault(c.size, []).append(c)
    return sorted(g.items())


def _run_group(tag, cases, n, env, host):
    """One plan over the cases (all of chunk size n), executed twice: the problems found."""
    H = _harness()
    from zarrs_amd import _lib as L
    B = H.B
    items = [H.Item(c.id, c.frame, B.OK if c.status == I.OK else B.CORRUPT, c.expect, n) for c in cases]
    nz = sum(c.n_zstd() for c in cases)
    nz_good = sum(1 for c in cases if c.comp == I.ZSTD for _, _, ne, s in c.streams() if s.kind == "zstd" and len(s.dec) == ne)
    must = sum(1 for c in cases if c.comp == I.ZSTD for _, _, ne, s in c.streams()
               if s.kind == "zstd" and s.parallel is True and len(s.dec) == ne)
    lo = sum(c.alias_count()[0] for c in cases)
    hi = sum(c.alias_count()[1] for c in cases)
    serial = env.get("ZGPU_ZSTD_FORCE_SERIAL") == "1"
    if serial or env.get("ZGPU_BLOSC_ALIAS") == "0":
        lo = hi = 0
    call = H.Call(items, n, host)
    problems = []
    try:
        for k in (1, 2):  # the first execution reads the layout back; the second runs k_blosc_layout
            t = f"{tag}/{k}"
            rc, st, rows, tail = call.execute()
            ctr = call.counters()
            ser, par, lat, ali = (ctr[L.CTR_ZSTD_SERIAL], ctr[L.CTR_ZSTD_PARALLEL], ctr[L.CTR_ZSTD_LATENCY],
                                  ctr[L.CTR_BLOSC_ALIASED])
            print(t, "rc", rc, "non-zero statuses", sum(1 for s in st if s), "of", len(st), "zstd streams", nz, "serial", ser,
                  "parallel", par, "latency", lat, "aliased", ali, "model", (lo, hi))
            problems += H._check(t, items, rc, st, rows, tail)
            for it, s in zip(items, st):
                if it.status == B.CORRUPT and s not in (0, L.CORRUPT_STREAM):
                    problems.append(f"{t}: {it.name}: status {s}, expected CORRUPT_STREAM")
            first = next((s for s in st if s), 0)
            if rc != first:
                problems.append(f"{t}: return code {rc}, the first failing status is {first}")
            if not (nz_good <= ser + par <= nz) or lat != 0:
                problems.append(f"{t}: zstd_serial {ser} + zstd_parallel {par} for {nz} zstd streams ({nz_good} valid), latency {lat}")
            if (serial and par) or (not serial and par < must):
                problems.append(f"{t}: zstd_parallel {par}, zstd_serial {ser}: {must} streams are meant for the parallel pipeline"
                                + (", all for the serial decoder here" if serial else ""))
            if not lo <= ali <= hi:
                problems.append(f"{t}: blosc_aliased {ali}, the rule gives {lo if lo == hi else (lo, hi)}")
            if ctr[L.CTR_BLOSC_RERUN]:
                problems.append(f"{t}: the execution was re-run")
    finally:
        call.close()
    return problems


def _run_family(family, env, host, monkeypatch=None):
    if monkeypatch is not None:
        for v in ENV_VARS:
            monkeypatch.delenv(v, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    cases = I.interleave(I.family(family))
    assert cases
    problems = []
    for n, group in _by_size(cases):
        assert n <= 128 * 1024
        problems += _run_group(f"{family}/{n}", group, n, env, host)
    return problems


_ZSTD = [(f, p) for f in I.ZSTD_FAMILIES for p in ZSTD_PATHS]


@pytest.mark.parametrize("family,path", _ZSTD, ids=[f"{f}-{p}" for f, p in _ZSTD])
def test_zstd_family_on_every_path(family, path, monkeypatch):
    problems = _run_family(family, ZSTD_PATHS[path], path.startswith("host"), monkeypatch)
    assert not problems, "\n".join(problems[:60])


@pytest.mark.parametrize("path", list(ZLIB_PATHS))
def test_zlib_family_on_every_path(path, monkeypatch):
    problems = _run_family("zlib_wrapped", ZLIB_PATHS[path], path == "host", monkeypatch)
    assert not problems, "\n".join(problems[:60])


def _child():
    """The child of test_zlib_lookahead_path: zlib_wrapped and mixed on direct rows, one JSON line."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    problems = _run_family("zlib_wrapped", {}, False) + _run_family("mixed", {}, False)
    print(json.dumps({"cases": len(I.family("zlib_wrapped")) + len(I.family("mixed")), "problems": problems[:60]}))


def test_zlib_lookahead_path():
    """ZGPU_GZIP_SEG=0: k_gzip<true>'s lookahead symbol decode (no segmented rounds), in a fresh process
    (the variable is read once per process), on every zlib case and on the mixed call."""
    env = dict(os.environ, ZGPU_GZIP_SEG="0")
    for v in ENV_VARS[:-1]:
        env.pop(v, None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["cases"] == len(I.family("zlib_wrapped")) + len(I.family("mixed"))
    assert res["problems"] == [], "\n".join(res["problems"])


if __name__ == "__main__":
    _child()
