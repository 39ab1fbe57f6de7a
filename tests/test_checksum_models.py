"""CPU checkers for numcodecs.zlib / adler32 / fletcher32 and a model of the GPU checksum kernels.

The checkers are Python's zlib (decompress, adler32) and a transcription of the reference's serial
Fletcher-32 loop (h5_checksum_fletcher32, zarrs fletcher32_codec.rs:63-96: big-endian 16-bit words,
folds every 360 words, a trailing odd byte never summed). They are pinned to the committed reference
fixtures here; tests/test_gpu_checksum_zlib.py holds the GPU against them.

linsum_model restates kernels/linsum.hpp in numpy with the kernel's arithmetic: ranges of CK_RANGE
bytes, 256 threads taking 16-byte vectors in turn, uint64 sums reduced modulo M once per thread and
range, the range's tail reduced modulo M before it multiplies A_r.
"""
import json
import os
import zlib

import numpy as np
import pytest

from fixtures import REF

CK_RANGE = 256 << 10  # kernels/linsum.hpp
CK_THREADS = 256
MOD = {"adler32": 65521, "fletcher32": 65535}


def fletcher32(data: bytes) -> int:
    """h5_checksum_fletcher32 as the reference has it (u32 sums; `n` is 0 when the odd byte is tested)."""
    n = len(data) // 2
    s1 = s2 = 0
    i = 0
    while n > 0:
        t = min(n, 360)
        n -= t
        for _ in range(t):
            s1 = (s1 + ((data[i] << 8) | data[i + 1])) & 0xFFFFFFFF
            i += 2
            s2 = (s2 + s1) & 0xFFFFFFFF
        s1 = (s1 & 0xFFFF) + (s1 >> 16)
        s2 = (s2 & 0xFFFF) + (s2 >> 16)
    if n % 2:  # never: n is 0 here
        raise AssertionError
    s1 = (s1 & 0xFFFF) + (s1 >> 16)
    s2 = (s2 & 0xFFFF) + (s2 >> 16)
    return (s2 << 16) | s1


def fletcher32_fast(data: bytes) -> int:
    """The closed form (exact integers): r(S2) << 16 | r(S1), r(x) = 0 if x == 0 else (x - 1) % 65535 + 1."""
    n = len(data) // 2
    w = np.frombuffer(data[:2 * n], dtype=">u2").astype(np.uint64)
    s1 = int(w.sum())
    s2 = int((w * np.arange(n, 0, -1, dtype=np.uint64)).sum()) if n < (1 << 24) else \
        sum(int(x) * (n - k) for k, x in enumerate(w))
    r = lambda x: 0 if x == 0 else (x - 1) % 65535 + 1  # noqa: E731
    return (r(s2) << 16) | r(s1)


def checksum(kind: str, data: bytes) -> int:
    return zlib.adler32(data) if kind == "adler32" else fletcher32_fast(data)


def encode_checksum(kind: str, data: bytes, at_start: bool = False) -> bytes:
    v = checksum(kind, data).to_bytes(4, "little")
    return v + data if at_start else data + v


# ---- the kernel's arithmetic -------------------------------------------------------------------
def _range_sums(kind: str, buf: np.ndarray):
    """wg_linsum: (A_r, B_r, nz) of one range standing alone (Fletcher: an even number of bytes)."""
    M = MOD[kind]
    n = len(buf)
    if kind == "adler32":
        unit = buf.astype(np.uint64)
        weight = np.arange(n, 0, -1, dtype=np.uint64)
        vec = np.arange(n) // 16
    else:
        unit = buf.view(">u2").astype(np.uint64)
        weight = np.arange(n // 2, 0, -1, dtype=np.uint64)
        vec = np.arange(n // 2) // 8
    thread = vec % CK_THREADS
    A = np.zeros(CK_THREADS, dtype=np.uint64)
    B = np.zeros(CK_THREADS, dtype=np.uint64)
    np.add.at(A, thread, unit)
    np.add.at(B, thread, unit * weight)  # below 2^57 per thread (linsum.hpp's static_assert)
    nz = int(A.any())
    return int((A % np.uint64(M)).sum()) % M, int((B % np.uint64(M)).sum()) % M, nz


def _value(kind: str, a: int, b: int, nz: int, length: int) -> int:
    M = MOD[kind]
    if kind == "adler32":
        return (((length % M + b) % M) << 16) | ((1 + a) % M)
    r1 = 0 if not nz else (a or 65535)
    r2 = 0 if not nz else (b or 65535)
    return (r2 << 16) | r1


def _combine(kind: str, parts, covered: int, length: int, y: int = 1) -> int:
    """parts: (offset, bytes, (A_r, B_r, nz)) per range. Workgroup y' takes ranges y', y' + y, ...
    (ck_accumulate), k_linsum_finish adds the workgroups' sums."""
    M = MOD[kind]
    acc = [[0, 0, 0] for _ in range(y)]
    for r, (off, m, (a_r, b_r, nz)) in enumerate(parts):
        tail = covered - off - m
        tail = (tail if kind == "adler32" else tail >> 1) % M  # reduced before the product
        g = acc[r % y]
        g[0] = (g[0] + a_r) % M
        g[1] = (g[1] + b_r + tail * a_r) % M
        g[2] |= nz
    a = sum(g[0] for g in acc) % M
    b = sum(g[1] for g in acc) % M
    return _value(kind, a, b, int(any(g[2] for g in acc)), length)


def linsum_model(kind: str, data: bytes, y: int = 1) -> int:
    buf = np.frombuffer(data, dtype=np.uint8)
    covered = len(buf) if kind == "adler32" else len(buf) & ~1
    parts = []
    for off in range(0, covered, CK_RANGE):
        m = min(CK_RANGE, covered - off)
        parts.append((off, m, _range_sums(kind, buf[off:off + m])))
    return _combine(kind, parts, covered, len(buf), y)


def linsum_model_constant(kind: str, byte: int, length: int, y: int = 1) -> int:
    """The model on `length` equal bytes without the buffer: every full range has the same sums."""
    covered = length if kind == "adler32" else length & ~1
    full = _range_sums(kind, np.full(CK_RANGE, byte, np.uint8))
    parts = [(off, CK_RANGE, full) for off in range(0, covered - covered % CK_RANGE, CK_RANGE)]
    if covered % CK_RANGE:
        m = covered % CK_RANGE
        parts.append((covered - m, m, _range_sums(kind, np.full(m, byte, np.uint8))))
    return _combine(kind, parts, covered, length, y)


def serial_constant(kind: str, byte: int, length: int) -> int:
    """Exact integers for `length` equal bytes."""
    if kind == "adler32":
        return (((length + byte * length * (length + 1) // 2) % 65521) << 16) | ((1 + byte * length) % 65521)
    n, w = length // 2, (byte << 8) | byte
    r = lambda x: 0 if x == 0 else (x - 1) % 65535 + 1  # noqa: E731
    return (r(w * n * (n + 1) // 2) << 16) | r(w * n)


# ---- the committed reference fixtures ----------------------------------------------------------
V3 = {k: f"v3_zarr_python/array_{k}.zarr" for k in ("zlib", "adler32", "fletcher32")}
V2 = {k: f"zarr_python_compat/{k}.zarr" for k in ("adler32", "fletcher32")}


def v3_chunks(kind):
    base = os.path.join(REF, V3[kind])
    meta = json.load(open(os.path.join(base, "zarr.json")))
    return meta, {(i, j): open(os.path.join(base, "c", str(i), str(j)), "rb").read()
                  for i in range(2) for j in range(2)}


def v2_chunks(kind):
    base = os.path.join(REF, V2[kind])
    meta = json.load(open(os.path.join(base, ".zarray")))
    return meta, {(i, j): open(os.path.join(base, f"{i}.{j}"), "rb").read() for i in range(2) for j in range(2)}


def strip_checked(kind: str, enc: bytes) -> bytes:
    """Decode one checksum codec with the checker: adler32's default location is the start."""
    if kind == "adler32":
        stored, data = enc[:4], enc[4:]
    else:
        stored, data = enc[-4:], enc[:-4]
    assert int.from_bytes(stored, "little") == checksum(kind, data)
    return data


@pytest.mark.parametrize("kind", ["adler32", "fletcher32"])
def test_checksum_fixtures(kind):
    meta, chunks = v3_chunks(kind)
    assert meta["codecs"][1] == {"name": f"numcodecs.{kind}", "configuration": {}}
    for enc in chunks.values():
        assert len(strip_checked(kind, enc)) == 100
    meta, chunks = v2_chunks(kind)
    assert meta["compressor"] == {"id": kind} and meta["dtype"] == "<u2" and meta["chunks"] == [50, 50]
    for enc in chunks.values():
        data = strip_checked(kind, enc)
        assert len(data) == 5000
        if kind == "fletcher32":
            assert fletcher32(data) == fletcher32_fast(data)


def test_zlib_fixture():
    meta, chunks = v3_chunks("zlib")
    assert meta["codecs"][1]["name"] == "numcodecs.zlib"
    none = os.path.join(REF, "v3_zarr_python/array_none.zarr", "c")
    for (i, j), enc in chunks.items():
        assert enc[:2] == b"\x78\xda"
        raw = zlib.decompress(enc)
        assert len(raw) == 100 and raw == open(os.path.join(none, str(i), str(j)), "rb").read()


def _cases():
    rng = np.random.default_rng(7)
    lens = [0, 1, 2, 3, 719 * 2, 720 * 2, 721 * 2, CK_RANGE - 1, CK_RANGE, CK_RANGE + 1, 2 * CK_RANGE + 3]
    for n in lens:
        yield f"zeros{n}", bytes(n)
        yield f"ff{n}", b"\xff" * n
        yield f"random{n}", rng.integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("kind", ["adler32", "fletcher32"])
def test_model_equals_serial(kind):
    for name, data in _cases():
        want = zlib.adler32(data) if kind == "adler32" else fletcher32(data)
        assert checksum(kind, data) == want, name
        for y in (1, 2, 3):
            assert linsum_model(kind, data, y) == want, (name, y)
        if name.startswith(("zeros", "ff")):
            assert linsum_model_constant(kind, data[0] if data else 0, len(data)) == want, name


@pytest.mark.parametrize("kind", ["adler32", "fletcher32"])
@pytest.mark.parametrize("byte", [0x00, 0x5A, 0xFF])
def test_model_huge_constant(kind, byte):
    """Past 2^33 bytes: the tail weights exceed 32 bits, so they must be reduced before multiplying."""
    n = (1 << 33) + 2 * CK_RANGE + 12345
    want = serial_constant(kind, byte, n)
    assert serial_constant(kind, byte, 100001) == checksum(kind, bytes([byte]) * 100001)
    for y in (1, 256):
        assert linsum_model_constant(kind, byte, n, y) == want
