"""numcodecs.zlib / numcodecs.adler32 / numcodecs.fletcher32 on the GPU: reference fixtures, the
checksum kernels at every length at which they take another path (vector tail, one range, range
edges, several ranges), error statuses, the zlib stage on every DEFLATE block type, chains, and the
write path. The checkers are Python's zlib and the serial Fletcher loop of test_checksum_models."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import fixtures as F
import oracle as O
from test_checksum_models import CK_RANGE, checksum, encode_checksum, fletcher32, strip_checked, v2_chunks, v3_chunks

pytestmark = pytest.mark.gpu

BYTES_LE = {"name": "bytes", "configuration": {"endian": "little"}}
ADLER_START = {"name": "numcodecs.adler32", "configuration": {}}
ADLER_END = {"name": "numcodecs.adler32", "configuration": {"location": "end"}}
FLETCHER = {"name": "numcodecs.fletcher32"}
CHECKSUMS = {"adler32-start": ("adler32", True, ADLER_START), "adler32-end": ("adler32", False, ADLER_END),
             "fletcher32": ("fletcher32", False, FLETCHER)}


def ZLIB(level=6):
    return {"name": "numcodecs.zlib", "configuration": {"level": level}}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    return Context(0)


def run_batch(torch, ch, encs, chunk_shape, dtype=np.uint8, flags=0, sel=None):
    """One zgpu_decode_batch over device-resident chunks packed back to back (unaligned starts):
    (return code, per-chunk statuses, output rows)."""
    from zarrs_amd import _lib as L, make_desc
    blob = b"".join(encs) or b"\0"
    dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    n = len(encs)
    shape = list(sel[1]) if sel else list(chunk_shape)
    descs, off = [], 0
    for i, e in enumerate(encs):
        descs.append(make_desc((dev.data_ptr() + off, len(e)), chunk_shape, sel[0] if sel else None,
                               sel[1] if sel else None, out_start=[i * shape[0]] + [0] * (len(shape) - 1)))
        off += len(e)
    out_shape = [n * shape[0]] + shape[1:]
    out = torch.zeros(max(int(np.prod(out_shape)), 1) * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")
    arr = (L.ChunkDesc * n)(*descs)
    st = (C.c_int32 * n)()
    rc = L.load().zgpu_decode_batch(ch._h, len(out_shape), arr, n, out.data_ptr(), L.u64s(out_shape),
                                    flags | L.ENC_DEVICE | L.OUT_DEVICE, st, None)
    torch.cuda.synchronize()
    got = out.cpu().numpy()[: int(np.prod(out_shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(out_shape)
    return rc, list(st), got


def contents(rng, n):
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes(), bytes(n), b"\xff" * n]


# ---- reference fixtures ------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["host", "hbm"])
@pytest.mark.parametrize("kind", ["zlib", "adler32", "fletcher32"])
def test_v3_reference_fixture(ctx, torch_cuda, kind, store):
    from zarrs_amd import Array, DeviceStore, MemoryStore
    meta, chunks = v3_chunks(kind)
    ms = MemoryStore({"c/" + "/".join(map(str, k)): v for k, v in chunks.items()})
    arr = Array(DeviceStore.from_store(ms) if store == "hbm" else ms, meta, ctx)
    got = arr.retrieve_array_subset()
    exp = np.zeros((10, 10), np.float32)
    for (i, j), enc in chunks.items():
        raw = zlib.decompress(enc) if kind == "zlib" else strip_checked(kind, enc)
        exp[5 * i:5 * i + 5, 5 * j:5 * j + 5] = np.frombuffer(raw, "<f4").reshape(5, 5)
    assert np.array_equal(got, exp)
    m, none = F.load_array("v3_zarr_python/array_none.zarr")
    nm = {"shape": m["shape"], "data_type": m["data_type"], "fill_value": m["fill_value"], "codecs": m["codecs"],
          "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": m["chunk_shape"]}}}
    plain = Array(MemoryStore({"c/" + "/".join(map(str, k)): v for k, v in none.items()}), nm, ctx)
    assert np.array_equal(got, plain.retrieve_array_subset())
    assert np.array_equal(arr.retrieve_array_subset([1, 2], [6, 5]), exp[1:7, 2:7])


@pytest.mark.parametrize("kind", ["adler32", "fletcher32"])
def test_v2_compat_fixture(ctx, torch_cuda, kind):
    from zarrs_amd import CodecChain
    _, chunks = v2_chunks(kind)
    ch = CodecChain.from_metadata([BYTES_LE, {"name": f"numcodecs.{kind}"}], "uint16", 0, ctx)
    for enc in chunks.values():
        exp = np.frombuffer(strip_checked(kind, enc), "<u2").reshape(50, 50)
        assert np.array_equal(ch.decode(enc, [50, 50]), exp)


# ---- the checksum kernels ----------------------------------------------------------------------
# 1439 / 1440 / 1441: around a multiple of 16 and of 360 words; CK_RANGE -1 / +0 / +1: the single-range
# path's limit (Fletcher's odd byte moves it by one); 2 ranges + 3 and 3 ranges (alone): the two-kernel path
LENGTHS = [0, 1, 2, 3, 4, 1439, 1440, 1441, CK_RANGE - 1, CK_RANGE, CK_RANGE + 1, 2 * CK_RANGE + 3]


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("which", list(CHECKSUMS))
def test_checksum_decode_encode(ctx, torch_cuda, which, n):
    from zarrs_amd import CodecChain
    kind, at_start, codec = CHECKSUMS[which]
    ch = CodecChain.from_metadata([BYTES_LE, codec], "uint8", 0, ctx)
    data = contents(np.random.default_rng(n), n)
    encs = [encode_checksum(kind, d, at_start) for d in data]
    rc, st, got = run_batch(torch_cuda, ch, encs, [n])
    assert rc == 0 and st == [0, 0, 0]
    assert got.tobytes() == b"".join(data)
    assert ch.encoded_size([max(n, 1)]) == max(n, 1) + 4 and ch.encoded_bound([max(n, 1)]) == max(n, 1) + 4
    if n:
        arr = torch_cuda.frombuffer(bytearray(b"".join(data)), dtype=torch_cuda.uint8).cuda()
        out = ch.encode_chunks(arr, [n], [[0], [n], [2 * n]])
        assert [bytes(o.cpu().numpy()) for o in out] == encs


@pytest.mark.parametrize("which", list(CHECKSUMS))
def test_checksum_three_ranges_alone(ctx, torch_cuda, which):
    from zarrs_amd import CodecChain
    kind, at_start, codec = CHECKSUMS[which]
    n = 3 * CK_RANGE - 5
    ch = CodecChain.from_metadata([BYTES_LE, codec], "uint8", 0, ctx)
    d = np.random.default_rng(3).integers(0, 256, n, dtype=np.uint8).tobytes()
    rc, st, got = run_batch(torch_cuda, ch, [encode_checksum(kind, d, at_start)], [n])
    assert rc == 0 and st == [0] and got.tobytes() == d


@pytest.mark.parametrize("which", list(CHECKSUMS))
def test_checksum_mixed_lengths_one_batch(ctx, torch_cuda, which):
    """64 items of different encoded lengths in one batch (a checksum around gzip members): items of
    one range and of several ranges side by side."""
    from zarrs_amd import CodecChain
    kind, at_start, codec = CHECKSUMS[which]
    n = 3 * CK_RANGE
    rng = np.random.default_rng(64)
    ch = CodecChain.from_metadata([BYTES_LE, {"name": "gzip", "configuration": {"level": 1}}, codec], "uint8", 0, ctx)
    data, encs = [], []
    for i in range(64):
        k = [0, 1, 1000, CK_RANGE // 2, CK_RANGE, 2 * CK_RANGE + 777, n][i % 7] if i < 14 else int(rng.integers(0, n))
        d = rng.integers(0, 256, k, dtype=np.uint8).tobytes() + bytes(n - k)
        c = zlib.compressobj(1, zlib.DEFLATED, 31)
        data.append(d)
        encs.append(encode_checksum(kind, c.compress(d) + c.flush(), at_start))
    assert min(map(len, encs)) < CK_RANGE < 2 * CK_RANGE < max(map(len, encs))
    rc, st, got = run_batch(torch_cuda, ch, encs, [n])
    assert rc == 0 and st == [0] * 64
    assert got.tobytes() == b"".join(data)


@pytest.mark.parametrize("n", [1441, 2 * CK_RANGE + 3])
@pytest.mark.parametrize("which", list(CHECKSUMS))
def test_checksum_errors(ctx, torch_cuda, which, n):
    from zarrs_amd import CodecChain, _lib as L
    kind, at_start, codec = CHECKSUMS[which]
    ch = CodecChain.from_metadata([BYTES_LE, codec], "uint8", 0, ctx)
    rng = np.random.default_rng(n + 1)
    data = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for _ in range(3)]
    good = [encode_checksum(kind, d, at_start) for d in data]
    lo = 4 if at_start else 0  # payload [lo, lo + n), checksum the other 4 bytes
    for pos in (lo, lo + n // 2, lo + n - 2, 0 if at_start else n, 3 if at_start else n + 3):
        bad = bytearray(good[1])
        bad[pos] ^= 0x10
        encs = [good[0], bytes(bad), good[2]]
        rc, st, got = run_batch(torch_cuda, ch, encs, [n])
        assert rc == L.INVALID_CHECKSUM and st == [0, L.INVALID_CHECKSUM, 0], pos
        assert got[:n].tobytes() == data[0] and got[2 * n:].tobytes() == data[2]
        exp = bytes(bad[lo:lo + n])
        rc, st, got = run_batch(torch_cuda, ch, encs, [n], flags=L.NO_VALIDATE)
        assert rc == 0 and st == [0, 0, 0] and got[n:2 * n].tobytes() == exp, pos
        rc, st, got = run_batch(torch_cuda, ch, encs, [n], sel=([5], [n - 9]))  # the partial decoder strips
        assert rc == 0 and st == [0, 0, 0] and got[n - 9:2 * (n - 9)].tobytes() == exp[5:n - 4], pos


@pytest.mark.parametrize("which", list(CHECKSUMS))
def test_checksum_input_too_short(ctx, torch_cuda, which):
    from zarrs_amd import CodecChain, _lib as L
    kind, at_start, codec = CHECKSUMS[which]
    ch = CodecChain.from_metadata([BYTES_LE, codec], "uint8", 0, ctx)
    good = encode_checksum(kind, b"", at_start)
    rc, st, _ = run_batch(torch_cuda, ch, [good, good[:3], good], [0])
    assert rc == L.CRC_INPUT_TOO_SHORT and st == [0, L.CRC_INPUT_TOO_SHORT, 0]


@pytest.mark.parametrize("n", [1, 1441, CK_RANGE + 1, 2 * CK_RANGE + 3])
def test_fletcher32_ignores_the_odd_byte(ctx, torch_cuda, n):
    from zarrs_amd import CodecChain
    ch = CodecChain.from_metadata([BYTES_LE, FLETCHER], "uint8", 0, ctx)
    d = bytearray(np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes())
    enc = encode_checksum("fletcher32", bytes(d))
    assert struct.unpack("<I", enc[-4:])[0] == fletcher32(bytes(d))
    d[-1] ^= 0xFF
    rc, st, got = run_batch(torch_cuda, ch, [bytes(d) + enc[-4:]], [n])
    assert rc == 0 and st == [0] and got.tobytes() == bytes(d)


# ---- the zlib stage ----------------------------------------------------------------------------
def _mixed(rng, n):
    words = [b"zarr", b"chunk", b"shard", b"decode", b"gpu", b"codec", b" ", b"\n"]
    text = b"".join(words[i] for i in rng.integers(0, len(words), n // 8 + 1))[: n // 2]
    return text + rng.integers(0, 256, n - len(text), dtype=np.uint8).tobytes()


ZSTREAMS = {"level0": (0, zlib.Z_DEFAULT_STRATEGY), "level1": (1, zlib.Z_DEFAULT_STRATEGY),
            "level6": (6, zlib.Z_DEFAULT_STRATEGY), "level9": (9, zlib.Z_DEFAULT_STRATEGY), "fixed": (6, zlib.Z_FIXED)}


@pytest.mark.parametrize("n", [0, 1, 100, 65537, 1 << 20])
@pytest.mark.parametrize("stream", list(ZSTREAMS))
def test_zlib_streams(ctx, torch_cuda, stream, n):
    """Stored, dynamic and fixed blocks; empty to multi-block streams past one decode segment; a lone
    item and a batch of 64."""
    from zarrs_amd import CodecChain
    level, strat = ZSTREAMS[stream]
    d = _mixed(np.random.default_rng(n + level), n)
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strat)
    enc = c.compress(d) + c.flush()
    assert zlib.decompress(enc) == d
    ch = CodecChain.from_metadata([BYTES_LE, ZLIB(level)], "uint8", 0, ctx)
    for count in (1, 64):
        rc, st, got = run_batch(torch_cuda, ch, [enc] * count, [n])
        assert rc == 0 and st == [0] * count
        assert got.tobytes() == d * count


def test_zlib_errors(ctx, torch_cuda):
    from zarrs_amd import CodecChain, ZgpuError, _lib as L
    ch = CodecChain.from_metadata([BYTES_LE, ZLIB()], "uint8", 0, ctx)
    d = _mixed(np.random.default_rng(5), 5000)
    enc = zlib.compress(d)
    trailer = bytearray(enc)
    trailer[-2] ^= 1
    fdict = bytearray(enc)
    fdict[1] |= 0x20
    fdict[1] = (fdict[1] & 0xE0) | (31 - ((fdict[0] << 8) | (fdict[1] & 0xE0)) % 31) % 31
    assert ((fdict[0] << 8) | fdict[1]) % 31 == 0 and fdict[1] & 0x20
    fcheck = bytearray(enc)
    fcheck[1] ^= 1
    for bad in (trailer, fdict, fcheck):
        for flags in (0, L.NO_VALIDATE):  # flate2 checks the trailer whatever validate_checksums says
            rc, st, got = run_batch(torch_cuda, ch, [enc, bytes(bad), enc], [5000], flags=flags)
            assert rc == L.CORRUPT_STREAM and st == [0, L.CORRUPT_STREAM, 0]
            assert got[:5000].tobytes() == d and got[10000:].tobytes() == d
    for cut in (1, 6, 7, len(enc) // 2, len(enc) - 5, len(enc) - 1):  # a truncated stream: an error, never a fault
        rc, st, _ = run_batch(torch_cuda, ch, [enc, enc[:cut], enc], [5000])
        assert rc != 0 and st[0] == 0 and st[1] != 0 and st[2] == 0, cut
    rc, st, got = run_batch(torch_cuda, ch, [enc + b"trailing garbage \x78\x9c"] * 2, [5000])
    assert rc == 0 and got.tobytes() == d * 2
    small = zlib.compress(b"x" * 100)
    for shape, length in (([101], 100), ([99], 100), ([5000], 100)):
        with pytest.raises(ZgpuError) as ei:
            ch.decode(small, shape)
        assert ei.value.status == L.DECODED_SIZE_MISMATCH
        assert L.last_size_mismatch() == (0, length, shape[0])
    with pytest.raises(ZgpuError) as ei:  # far past the slot: inflate stops there, the total is unknown
        ch.decode(zlib.compress(b"x" * 5000), [99])
    assert ei.value.status == L.DECODED_SIZE_MISMATCH and L.last_size_mismatch() == (0, None, 99)


def test_codec_configurations(ctx, torch_cuda):
    from zarrs_amd import CodecChain, ZgpuError, _lib as L
    for cfg in ({}, {"level": 10}, {"level": -1}, {"level": "6"}, {"level": 1.5}):
        with pytest.raises(ZgpuError) as ei:
            CodecChain.from_metadata([BYTES_LE, {"name": "numcodecs.zlib", "configuration": cfg}], "uint8", 0, ctx)
        assert ei.value.status == L.INVALID_ARGUMENT, cfg
    with pytest.raises(ZgpuError) as ei:
        CodecChain.from_metadata([BYTES_LE, {"name": "numcodecs.adler32", "configuration": {"location": "middle"}}],
                                 "uint8", 0, ctx)
    assert ei.value.status == L.INVALID_ARGUMENT
    ch = CodecChain.from_metadata([BYTES_LE, "https://codec.zarrs.dev/bytes_to_bytes/fletcher32"], "uint8", 0, ctx)
    assert bytes(ch.decode(encode_checksum("fletcher32", b"abcd"), [4])) == b"abcd"
    start = CodecChain.from_metadata([BYTES_LE, {"name": "numcodecs.adler32", "configuration": {"location": "start"}}],
                                     "uint8", 0, ctx)
    assert bytes(start.decode(encode_checksum("adler32", b"abcd", True), [4])) == b"abcd"


# ---- chains ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt", [([5, 7, 3], "uint16"), ([33, 17], "float64")])
def test_chain_transpose_shuffle_zlib_fletcher(ctx, torch_cuda, shape, dt):
    from zarrs_amd import CodecChain
    es = np.dtype(dt).itemsize
    head = [{"name": "transpose", "configuration": {"order": list(range(len(shape)))[::-1]}},
            {"name": "bytes", "configuration": {"endian": "big"}},
            {"name": "numcodecs.shuffle", "configuration": {"elementsize": es}}]
    rng = np.random.default_rng(es)
    a = (rng.standard_normal(shape) * 300).astype(dt)
    inner = O.OracleChain.from_metadata(head, dt, 0, len(shape)).encode(a)
    enc = encode_checksum("fletcher32", zlib.compress(inner, 6))
    ch = CodecChain.from_metadata(head + [ZLIB(6), FLETCHER], dt, 0, ctx)
    assert np.array_equal(ch.decode(enc, shape), a)
    rc, st, got = run_batch(torch_cuda, ch, [enc] * 3, shape, dtype=dt)
    assert rc == 0 and st == [0, 0, 0] and np.array_equal(got, np.concatenate([a] * 3))
    sub = ch.partial_decode(enc, shape, [1] * len(shape), [2] * len(shape))
    assert np.array_equal(sub, a[tuple(slice(1, 3) for _ in shape)])


def test_chain_adler_gzip_crc_and_fletcher_zstd(ctx, torch_cuda):
    from zarrs_amd import CodecChain, _lib as L
    a = (np.random.default_rng(9).standard_normal(3000) * 50).astype(np.float32)
    raw = a.tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    gz = c.compress(encode_checksum("adler32", raw, True)) + c.flush()
    enc = gz + struct.pack("<I", O.crc32c(gz))
    ch = CodecChain.from_metadata([BYTES_LE, ADLER_START, {"name": "gzip", "configuration": {"level": 6}},
                                   {"name": "crc32c"}], "float32", 0, ctx)
    rc, st, got = run_batch(torch_cuda, ch, [enc] * 5, [3000], dtype=np.float32)
    assert rc == 0 and st == [0] * 5 and np.array_equal(got, np.tile(a, 5))
    inner_bad = bytearray(encode_checksum("adler32", raw, True))  # the inner checksum, inside a valid gzip member
    inner_bad[2000] ^= 1
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    gzb = c.compress(bytes(inner_bad)) + c.flush()
    rc, st, _ = run_batch(torch_cuda, ch, [enc, gzb + struct.pack("<I", O.crc32c(gzb))], [3000], dtype=np.float32)
    assert rc == L.INVALID_CHECKSUM and st == [0, L.INVALID_CHECKSUM]
    zc = [BYTES_LE, FLETCHER, {"name": "zstd", "configuration": {"level": 3, "checksum": False}}]
    zenc = O.OracleChain.from_metadata([BYTES_LE, zc[2]], "uint8", 0, 1).encode(
        np.frombuffer(encode_checksum("fletcher32", raw), np.uint8))
    ch = CodecChain.from_metadata(zc, "float32", 0, ctx)
    rc, st, got = run_batch(torch_cuda, ch, [zenc] * 3, [3000], dtype=np.float32)
    assert rc == 0 and st == [0] * 3 and np.array_equal(got, np.tile(a, 3))


def _shard(inner_encs, n_inner):
    """sharding_indexed bytes: present inner chunks in C order, the index (LE u64 pairs + crc32c) at the end."""
    body, index = b"", []
    for k in range(n_inner):
        e = inner_encs.get(k)
        index += [2 ** 64 - 1, 2 ** 64 - 1] if e is None else [len(body), len(e)]
        body += e or b""
    raw = struct.pack(f"<{2 * n_inner}Q", *index)
    return body + raw + struct.pack("<I", O.crc32c(raw))


def _sharding(inner_shape, inner_codecs):
    return {"name": "sharding_indexed", "configuration": {
        "chunk_shape": inner_shape, "codecs": inner_codecs,
        "index_codecs": [BYTES_LE, {"name": "crc32c"}], "index_location": "end"}}


def test_sharding_over_zlib_adler(ctx, torch_cuda):
    from zarrs_amd import CodecChain
    a = np.random.default_rng(11).integers(0, 500, (8, 8)).astype(np.uint16)
    a[4:, :4] = 7  # inner chunk 2 is left out of the shard: the fill value
    inner = {}
    for k, (i, j) in enumerate([(0, 0), (0, 4), (4, 0), (4, 4)]):
        if k != 2:
            inner[k] = encode_checksum("adler32", zlib.compress(a[i:i + 4, j:j + 4].tobytes()))
    shard = _shard(inner, 4)
    ch = CodecChain.from_metadata([_sharding([4, 4], [BYTES_LE, ZLIB(6), ADLER_END])], "uint16", 7, ctx)
    assert np.array_equal(ch.decode(shard, [8, 8]), a)
    assert np.array_equal(ch.partial_decode(shard, [8, 8], [2, 1], [5, 6]), a[2:7, 1:7])


def _stored_zlib(data: bytes, block: int = 16) -> bytes:
    """A valid zlib stream of `block`-byte stored blocks: far longer than any encoder's bound of its input."""
    d = np.frombuffer(data, np.uint8).reshape(-1, block)
    rows = np.zeros((len(d), 5 + block), np.uint8)
    rows[:, 1:5] = np.frombuffer(struct.pack("<HH", block, block ^ 0xFFFF), np.uint8)
    rows[-1, 0] = 1  # BFINAL
    rows[:, 5:] = d
    return b"\x78\x01" + rows.tobytes() + struct.pack(">I", zlib.adler32(data))


@pytest.mark.parametrize("which", list(CHECKSUMS))
def test_sharded_inner_chunk_longer_than_the_chain_bound(ctx, torch_cuda, which):
    """An inner chunk's length is known only on the device, so the host sizes the checksum grid from the
    inner chain's encoded bound (here under one range: one workgroup per item). A stored inner chunk may
    be longer than that bound and than one range; it is verified all the same, good and bad value."""
    from zarrs_amd import CodecChain, _lib as L
    kind, at_start, codec = CHECKSUMS[which]
    n = 240 << 10
    rng = np.random.default_rng(17)
    ch = CodecChain.from_metadata([_sharding([n], [BYTES_LE, ZLIB(0), codec])], "uint8", 0, ctx)
    plain = CodecChain.from_metadata([BYTES_LE, ZLIB(0), codec], "uint8", 0, ctx)
    assert plain.encoded_bound([n]) < CK_RANGE
    data = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for _ in range(4)]
    inner = [encode_checksum(kind, _stored_zlib(d), at_start) for d in data]
    assert all(len(e) > CK_RANGE + 4096 for e in inner)
    bad = bytearray(inner[3])
    bad[1 if at_start else len(bad) - 2] ^= 0x40  # the stored value only: the zlib stream stays valid
    shards = [_shard({0: inner[0], 1: inner[1]}, 2), _shard({0: inner[2], 1: bytes(bad)}, 2)]
    rc, st, got = run_batch(torch_cuda, ch, shards, [2 * n])
    assert rc == L.INVALID_CHECKSUM and st == [0, L.INVALID_CHECKSUM]
    assert got[:2 * n].tobytes() == data[0] + data[1]
    rc, st, got = run_batch(torch_cuda, ch, shards, [2 * n], flags=L.NO_VALIDATE)
    assert rc == 0 and st == [0, 0] and got.tobytes() == b"".join(data)


def test_zlib_after_sharding_regrows_its_slots(ctx, torch_cuda):
    """A codec after sharding_indexed decodes whole shards; zlib streams carry no size, so the slots
    start at 4x the encoded shard and grow 8x per DECODED_SIZE_MISMATCH (this shard is > 32:1: two regrows)."""
    from zarrs_amd import CodecChain
    a = np.zeros((64, 64), np.uint16)
    a[:32, :32] = (np.arange(1024) % 5).reshape(32, 32)
    inner = {k: a[i:i + 32, j:j + 32].tobytes() for k, (i, j) in enumerate([(0, 0), (0, 32), (32, 0), (32, 32)])}
    shard = _shard(inner, 4)
    enc = zlib.compress(shard, 9)
    assert len(shard) > 32 * len(enc) + 256  # past the first slots (4x) and the second (32x)
    ch = CodecChain.from_metadata([_sharding([32, 32], [BYTES_LE]), ZLIB(9)], "uint16", 0, ctx)
    assert np.array_equal(ch.decode(enc, [64, 64]), a)
    assert np.array_equal(ch.partial_decode(enc, [64, 64], [30, 30], [4, 4]), a[30:34, 30:34])


# ---- write path --------------------------------------------------------------------------------
def _bound(n):
    return n + (n >> 12) + (n >> 14) + (n >> 25) + 13


@pytest.mark.parametrize("shape", [[100], [333, 41], [70000]])
def test_encode_zlib_chains(ctx, torch_cuda, shape):
    from zarrs_amd import CodecChain
    n = int(np.prod(shape))
    a = np.abs(np.random.default_rng(n).standard_normal([3 * shape[0]] + shape[1:]) * 90).astype(np.uint16)
    a[: shape[0]] //= 16  # more compressible
    dev = torch_cuda.frombuffer(bytearray(a.tobytes()), dtype=torch_cuda.uint8).cuda().view(torch_cuda.uint16)
    dev = dev.reshape(a.shape)
    starts = [[k * shape[0]] + [0] * (len(shape) - 1) for k in range(3)]
    shuffle = {"name": "numcodecs.shuffle", "configuration": {"elementsize": 2}}
    plain = CodecChain.from_metadata([BYTES_LE, ZLIB(6)], "uint16", 0, ctx)
    assert plain.encoded_size(shape) == -1 and plain.encoded_bound(shape) == _bound(2 * n)
    for k, e in enumerate(plain.encode_chunks(dev, shape, starts)):
        e = bytes(e.cpu().numpy())
        chunk = a[k * shape[0]:(k + 1) * shape[0]]
        assert zlib.decompress(e) == chunk.tobytes() and len(e) <= _bound(2 * n)
        assert np.array_equal(plain.decode(e, shape), chunk)
    full = CodecChain.from_metadata([BYTES_LE, shuffle, ZLIB(6), FLETCHER], "uint16", 0, ctx)
    assert full.encoded_bound(shape) == _bound(2 * n) + 4
    for k, e in enumerate(full.encode_chunks(dev, shape, starts)):
        e = bytes(e.cpu().numpy())
        chunk = a[k * shape[0]:(k + 1) * shape[0]]
        assert struct.unpack("<I", e[-4:])[0] == fletcher32(e[:-4])
        planes = np.frombuffer(zlib.decompress(e[:-4]), np.uint8).reshape(2, n)
        assert planes.T.tobytes() == chunk.tobytes()
        assert np.array_equal(full.decode(e, shape), chunk)
    both = CodecChain.from_metadata([BYTES_LE, ADLER_START, ZLIB(1), ADLER_START, ADLER_END], "uint16", 0, ctx)
    assert both.encoded_bound(shape) == _bound(2 * n + 4) + 8
    for k, e in enumerate(both.encode_chunks(dev, shape, starts)):
        e = bytes(e.cpu().numpy())
        chunk = a[k * shape[0]:(k + 1) * shape[0]]
        mid = strip_checked("adler32", e[:-4])
        assert struct.unpack("<I", e[-4:])[0] == checksum("adler32", e[:-4])
        assert strip_checked("adler32", zlib.decompress(mid)) == chunk.tobytes()
        assert np.array_equal(both.decode(e, shape), chunk)


def test_encode_zlib_incompressible_stays_within_the_bound(ctx, torch_cuda):
    """The encoder's DEFLATE blocks hold at most 16,384 symbols, so stored blocks of incompressible
    input cost more than the 5 bytes per 16 KiB that ZlibCodec's bound allows; past the bound the stream
    is written as 65,535-byte stored blocks instead (24 MiB of noise: about 15 bytes over, counted from the
    block sizes)."""
    from zarrs_amd import CodecChain
    n = 24 << 20
    dev = torch_cuda.randint(0, 256, (n,), dtype=torch_cuda.uint8, device="cuda",
                             generator=torch_cuda.Generator(device="cuda").manual_seed(5))
    raw = bytes(dev.cpu().numpy())
    for codecs, extra in (([BYTES_LE, ZLIB(6)], 0), ([BYTES_LE, ZLIB(6), FLETCHER], 4)):
        ch = CodecChain.from_metadata(codecs, "uint8", 0, ctx)
        (e,) = ch.encode_chunks(dev, [n], [[0]])
        assert e.numel() <= _bound(n) + extra == ch.encoded_bound([n])
        enc = bytes(e.cpu().numpy())
        assert zlib.decompress(enc[:len(enc) - extra]) == raw
        rc, st, got = run_batch(torch_cuda, ch, [enc], [n])
        assert rc == 0 and st == [0] and got.tobytes() == raw


def test_sharded_write_zlib_adler_reads_back(ctx, torch_cuda):
    from zarrs_amd import CodecChain
    a = np.random.default_rng(21).integers(0, 300, (16, 8)).astype(np.uint16)
    a[4:8, 4:] = 0  # an all-fill inner chunk is left out
    ch = CodecChain.from_metadata([_sharding([4, 4], [BYTES_LE, ZLIB(6), ADLER_START])], "uint16", 0, ctx)
    dev = torch_cuda.frombuffer(bytearray(a.tobytes()), dtype=torch_cuda.uint8).cuda().view(torch_cuda.uint16)
    shards = ch.encode_chunks(dev.reshape(16, 8), [8, 8], [[0, 0], [8, 0]])
    for k, s in enumerate(shards):
        s = bytes(s.cpu().numpy())
        part = a[8 * k:8 * k + 8]
        index = struct.unpack("<8Q", s[-68:-4])
        assert struct.unpack("<I", s[-4:])[0] == O.crc32c(s[-68:-4])
        assert (index[6:] == (2 ** 64 - 1,) * 2) == (k == 0)
        off, size = index[0], index[1]
        inner0 = s[off:off + size]
        assert zlib.decompress(inner0[4:]) == part[:4, :4].tobytes()
        assert struct.unpack("<I", inner0[:4])[0] == zlib.adler32(inner0[4:])
        assert np.array_equal(ch.decode(s, [8, 8]), part)
        assert np.array_equal(ch.partial_decode(s, [8, 8], [3, 2], [4, 5]), part[3:7, 2:7])


# ---- the blosc path shares the Adler-32 device function ----------------------------------------
def test_blosc_zlib_streams_still_bit_exact(ctx, torch_cuda):
    from zarrs_amd import CodecChain, ZgpuError, _lib as L
    codecs = [BYTES_LE, {"name": "blosc", "configuration": {"cname": "zlib", "clevel": 5, "shuffle": "shuffle",
                                                            "typesize": 4, "blocksize": 0}}]
    a = np.round(np.random.default_rng(2).standard_normal(150001) * 40).astype(np.float32)
    enc = O.OracleChain.from_metadata(codecs, "float32", 0, 1).encode(a)
    ch = CodecChain.from_metadata(codecs, "float32", 0, ctx)
    rc, st, got = run_batch(torch_cuda, ch, [enc] * 3, [150001], dtype=np.float32)
    assert rc == 0 and st == [0] * 3 and np.array_equal(got, np.tile(a, 3))
    bad = bytearray(enc)
    first = struct.unpack("<I", enc[16:20])[0]  # the first block's streams: [i32 csize | zlib stream] each
    csize = struct.unpack("<i", enc[first:first + 4])[0]
    assert len(zlib.decompress(enc[first + 4:first + 4 + csize])) > csize
    bad[first + 4 + csize - 1] ^= 1  # the first stream's Adler-32 trailer
    with pytest.raises(ZgpuError) as ei:
        ch.decode(bytes(bad), [150001])
    assert ei.value.status == L.CORRUPT_STREAM
