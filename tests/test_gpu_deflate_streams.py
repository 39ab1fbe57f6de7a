"""k_gzip on hand-built DEFLATE streams (tests/deflate_streams.py: what RFC 1951 allows and zlib's
encoder never emits, at the executor's ring/flush edge, its dependency rounds, the table builders'
limits, the lane-parallel header decode's windows, block and lane-region boundaries, lanes out of sync,
and streams of the wrong decoded size), bit-exact against the reference executor and zlib
(tests/test_deflate_streams_model.py ties those together on the CPU and shows that each case reaches
its state in the model). One decode_batch call per family and decoded size, the streams concatenated
at unaligned device offsets, corrupt ones beside valid ones; on the pipelined and the one-wave gzip
kernel, each with and without a trailing crc32c, on numcodecs.zlib (k_gzip<true, false, true>), into
16-B aligned rows with the direct path on and off, as lone items, and on the lookahead path
(ZGPU_GZIP_SEG=0, read once per process: a child process).

The executor_ring family is the regression test of two wrong-bytes defects these streams found: with
BATCH_CAP = RING / 2 a batch could hold RING - 30 or more unflushed bytes, and a short match's source
was then read stale from the slot, or a flush wrote newer ring bytes over flushed ones (42 of the
family's cases failed with CORRUPT_STREAM, the ones the CPU model puts in those states)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import deflate_streams as D

pytestmark = pytest.mark.gpu

BYTES_LE = {"name": "bytes", "configuration": {"endian": "little"}}
GZ = {"name": "gzip", "configuration": {"level": 1}}
ZL = {"name": "numcodecs.zlib", "configuration": {"level": 1}}
SENTINEL = 0xA5
PATHS = {  # name: (stream kind, codecs, environment)
    "pipelined": ("gz", [BYTES_LE, GZ], {}),
    "one_wave": ("gz", [BYTES_LE, GZ], {"ZGPU_GZIP_PIPE_MAX": "0"}),
    "pipelined_crc32c": ("gz_crc", [BYTES_LE, GZ, {"name": "crc32c"}], {}),
    "one_wave_crc32c": ("gz_crc", [BYTES_LE, GZ, {"name": "crc32c"}], {"ZGPU_GZIP_PIPE_MAX": "0"}),
    "zlib": ("zlib", [BYTES_LE, ZL], {}),
}
GZIP_VARS = ["ZGPU_GZIP_PIPE_MAX", "ZGPU_GZIP_DIRECT", "ZGPU_GZIP_LPT"]


def _want_status(c):
    from zarrs_amd import _lib as L
    return {D.OK: 0, D.CORRUPT: L.CORRUPT_STREAM, D.SIZE: L.DECODED_SIZE_MISMATCH}[c.status]


def _decode(cases, kind, codecs):
    """One zgpu_decode_batch over `cases` (all of one chunk size), each into its own row of a
    sentinel-filled output with a sentinel tail: (return code, statuses, rows, tail)."""
    import torch
    from zarrs_amd import CodecChain, Context, make_desc
    from zarrs_amd import _lib as L
    n, k = cases[0].size, len(cases)
    assert all(c.size == n for c in cases)
    encs = [c.enc(kind) for c in cases]
    dev = torch.frombuffer(bytearray(b"".join(encs)), dtype=torch.uint8).cuda()
    descs, off = [], 0
    for i, e in enumerate(encs):
        descs.append(make_desc((dev.data_ptr() + off, len(e)), [n], out_start=[i * n]))
        off += len(e)  # unaligned stream starts on purpose
    ch = CodecChain.from_metadata(codecs, "uint8", 0, Context.default())
    out = torch.full((k * n + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    arr = (L.ChunkDesc * k)(*descs)
    st = (C.c_int32 * k)()
    rc = L.load().zgpu_decode_batch(ch._h, 1, arr, k, out.data_ptr(), L.u64s([k * n]),
                                    L.ENC_DEVICE | L.OUT_DEVICE, st, None)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return rc, list(st), got[:k * n].reshape(k, n), got[k * n:]


def _first_wrong(c, got):
    exp = np.frombuffer(c.expect, np.uint8)
    bad = np.flatnonzero(got != exp)
    if not len(bad):
        return None
    p = int(bad[0])
    return (f"{c.name}: {len(bad)} wrong bytes, the first at {p} of {len(exp)} "
            f"(got {int(got[p]):#04x}, expected {int(exp[p]):#04x})")


def _check(tag, cases, rc, st, rows, tail):
    """The problems of one call: statuses, the bytes of every valid item, untouched rows and tail."""
    problems = []
    want = [_want_status(c) for c in cases]
    if st != want:
        problems += [f"{tag}: {c.name}: status {s}, expected {w} ({c.status})"
                     for c, s, w in zip(cases, st, want) if s != w]
    first_bad = next((w for w in want if w), 0)
    if rc != first_bad:
        problems.append(f"{tag}: return code {rc}, expected the first failing status {first_bad}")
    for i, c in enumerate(cases):
        if c.status == D.OK:
            w = _first_wrong(c, rows[i])
            if w:
                problems.append(f"{tag}: {w}")
    if not (tail == SENTINEL).all():
        problems.append(f"{tag}: bytes written past the last row")
    return problems


def _groups(cases):
    g = {}
    for c in cases:
        g.setdefault(c.size, []).append(c)
    return sorted(g.items())


def _setenv(monkeypatch, env):
    for v in GZIP_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("family", list(D.FAMILIES))
def test_family_on_every_path(family, path, monkeypatch):
    kind, codecs, env = PATHS[path]
    _setenv(monkeypatch, env)
    problems = []
    for n, cases in _groups(D.family(family)):
        rc, st, rows, tail = _decode(cases, kind, codecs)
        tag = f"{family}/{path}/{n}"
        print(tag, "rc", rc, "statuses", st)
        problems += _check(tag, cases, rc, st, rows, tail)
    assert not problems, "\n".join(problems[:60])


@pytest.mark.parametrize("path", ["pipelined", "one_wave"])
def test_overlong_stream_writes_nothing_past_its_row(path, monkeypatch):
    """A stream decoding past its chunk (a 258-byte match crossing the chunk's end; a stored block one
    byte too long) as the call's last item: the bytes after its row stay as they were, and the valid
    item before it is exact."""
    kind, codecs, env = PATHS[path]
    _setenv(monkeypatch, env)
    fam = D.family("size")
    ok = next(c for c in fam if c.status == D.OK)
    long_ = [c for c in fam if c.name.startswith("size_long")]
    assert len(long_) == 2
    problems = []
    for c in long_:
        assert len(c.decoded) > c.size
        rc, st, rows, tail = _decode([ok, c], kind, codecs)
        problems += _check(f"overlong/{path}/{c.name}", [ok, c], rc, st, rows, tail)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("path", ["pipelined", "one_wave"])
def test_ring_cases_as_lone_items(path, monkeypatch):
    """The executor-ring cases one stream a call: a lone stream gets no LPT order."""
    kind, codecs, env = PATHS[path]
    _setenv(monkeypatch, env)
    cases = [c for c in D.family("executor_ring") if c.ring]
    assert len(cases) >= 30
    problems = []
    for c in cases:
        rc, st, rows, tail = _decode([c], kind, codecs)
        problems += _check(f"lone/{path}", [c], rc, st, rows, tail)
    assert not problems, "\n".join(problems[:60])


@pytest.mark.parametrize("direct", ["1", "0"])
@pytest.mark.parametrize("path", ["pipelined", "one_wave"])
def test_valid_4k_cases_into_aligned_rows(path, direct, monkeypatch):
    """Every valid 4096-byte case as a whole chunk of a 1-d uint8 array on 16-B aligned rows (the
    GzDirect layout of test_gpu_gzip_direct.py), the direct path on and off; sentinels between the
    rows and outside the window stay."""
    import torch
    from zarrs_amd import CodecChain, Context, make_desc
    kind, codecs, env = PATHS[path]
    _setenv(monkeypatch, dict(env, ZGPU_GZIP_DIRECT=direct))
    cases = [c for f in D.FAMILIES for c in D.family(f) if c.status == D.OK and c.size == 4096]
    n, gap, ws = 4096, 16, 16
    win = len(cases) * (n + gap)
    encs = [c.enc(kind) for c in cases]
    dev = torch.frombuffer(bytearray(b"".join(encs)), dtype=torch.uint8).cuda()
    descs, off = [], 0
    for i, e in enumerate(encs):
        descs.append(make_desc((dev.data_ptr() + off, len(e)), [n], out_start=[i * (n + gap)]))
        off += len(e)
    ch = CodecChain.from_metadata(codecs, "uint8", 0, Context.default())
    out = torch.full((win + 48,), SENTINEL, dtype=torch.uint8, device="cuda")
    st = ch.decode_batch_into(descs, out, [ws], [win], enc_device=True)
    assert st == [0] * len(cases)
    got = out.cpu().numpy()
    assert (got[:ws] == SENTINEL).all() and (got[ws + win:] == SENTINEL).all()
    body = got[ws:ws + win].reshape(len(cases), n + gap)
    problems = [w for w in (_first_wrong(c, body[i, :n]) for i, c in enumerate(cases)) if w]
    assert not problems, "\n".join(problems[:60])
    assert (body[:, n:] == SENTINEL).all(), "bytes written between the rows"


def _child():
    """The child of test_lookahead_path: the valid cases of every family, one call per decoded size,
    one JSON line of statuses and mismatches."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    res = {"calls": 0, "bad_status": [], "mismatches": []}
    kind, codecs, _ = PATHS["one_wave"]
    for f in D.FAMILIES:
        for n, cases in _groups([c for c in D.family(f) if c.status == D.OK]):
            rc, st, rows, tail = _decode(cases, kind, codecs)
            res["calls"] += 1
            res["bad_status"] += [[c.name, s] for c, s in zip(cases, st) if s != 0]
            res["mismatches"] += [w for w in (_first_wrong(c, rows[i]) for i, c in enumerate(cases)) if w]
            if not (tail == SENTINEL).all():
                res["mismatches"].append(f"{f}/{n}: bytes written past the last row")
    print(json.dumps(res))


def test_lookahead_path():
    """ZGPU_GZIP_SEG=0: the lookahead symbol decode (no segmented rounds) on every valid case."""
    env = dict(os.environ, ZGPU_GZIP_SEG="0", ZGPU_GZIP_PIPE_MAX="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(res)
    assert res["calls"] >= len(D.FAMILIES)
    assert res["bad_status"] == [] and res["mismatches"] == []


if __name__ == "__main__":
    _child()
