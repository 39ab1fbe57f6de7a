"""GPU decode and encode of the codecs that change element values or widths (packbits,
numcodecs.fixedscaleoffset, bitround; kernels/value.hip and the composed paths of general.cpp's
decode_general) against the numpy model composed with the CPU oracle (tests/value_codecs.py): bit-exact,
no tolerance, encoded bytes in HBM and on the host, full and partial selections."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import value_codecs as V

pytestmark = pytest.mark.gpu

BYTES = {"name": "bytes", "configuration": {"endian": "little"}}
BYTES_BIG = {"name": "bytes", "configuration": {"endian": "big"}}
IDX = [BYTES, {"name": "crc32c"}]
GZIP = {"name": "gzip", "configuration": {"level": 1}}
ZSTD = {"name": "zstd", "configuration": {"level": 3, "checksum": True}}
CRC = {"name": "crc32c"}
BLOSC = {"name": "blosc", "configuration": {"cname": "lz4", "clevel": 5, "shuffle": "shuffle", "typesize": 4,
                                            "blocksize": 0}}
SHAPE = [16, 32, 32]
SELS3 = (([0, 0, 0], SHAPE), ([3, 5, 7], [11, 20, 22]), ([9, 17, 1], [1, 1, 1]))
# bool: 16 elements per thread, 256 threads per workgroup (k_unpackbits)
BOOL_COUNTS = [1, 7, 8, 9, 4099, 16 * 256 + 1]


def sh(cs, inner):
    return {"name": "sharding_indexed", "configuration": {"chunk_shape": cs, "codecs": inner, "index_codecs": IDX}}


def tr(order):
    return {"name": "transpose", "configuration": {"order": order}}


def fso(dtype, astype, offset, scale):
    cfg = {"offset": offset, "scale": scale, "dtype": dtype}
    if astype:
        cfg["astype"] = astype
    return {"name": V.FSO, "configuration": cfg}


def packbits(first=None, last=None, padding="none"):
    cfg = {"padding_encoding": padding}
    if first is not None:
        cfg["first_bit"] = first
    if last is not None:
        cfg["last_bit"] = last
    return {"name": "packbits", "configuration": cfg}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    return Context(0)


def _src(enc, torch, hbm):
    return torch.frombuffer(bytearray(enc), dtype=torch.uint8).cuda() if hbm else enc


def _sels(shape):
    if len(shape) == 3:
        return SELS3
    n = shape[0]
    return (([0], [n]), ([n // 3], [n - n // 3]), ([n - 1], [1]))


def check_decode(ch, torch, enc, shape, exp, tag):
    """every selection, from HBM and from the host, bitwise equal to exp"""
    from zarrs_amd import make_desc
    for hbm in (True, False):
        src = _src(enc, torch, hbm)
        for start, sub in _sels(shape):
            out = np.zeros(sub, exp.dtype)
            st = ch.decode_batch([make_desc(src, shape, start, sub)], out, sub, enc_device=hbm)
            assert st == [0]
            want = np.ascontiguousarray(exp[tuple(slice(s, s + n) for s, n in zip(start, sub))])
            assert out.tobytes() == want.tobytes(), (tag, hbm, start, sub)


def _raw(data_type, shape, seed):
    """every bit pattern of the type (floats: NaNs, infinities and denormals among them)"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(V.NP[data_type])
    n = int(np.prod(shape))
    if data_type == "bool":
        return rng.integers(0, 2, n, dtype=np.uint8).view(np.bool_).reshape(shape)
    return np.frombuffer(rng.bytes(n * dt.itemsize), dt).reshape(shape).copy()


# ---------------------------------------------------------------------------------------------------
# packbits decode
# ---------------------------------------------------------------------------------------------------
PB_TYPES = [("uint16", 3, 12), ("int8", 0, 3), ("int32", 0, 11), ("int16", 0, 11), ("float32", 16, 31),
            ("complex64", 16, 31)]
PB_WRAPS = {
    "alone": lambda pb: [pb],
    "gzip": lambda pb: [pb, GZIP],
    "zstd_crc": lambda pb: [pb, ZSTD, CRC],
    "transpose": lambda pb: [tr([2, 0, 1]), pb],
}
PADDINGS = ["none", "first_byte", "last_byte"]
PB_CASES = [(t, w, PADDINGS[(i + j) % 3]) for i, t in enumerate(PB_TYPES) for j, w in enumerate(sorted(PB_WRAPS))]
PB_CASES += [(t, "alone", p) for i, t in enumerate(PB_TYPES) for p in PADDINGS if p != PADDINGS[i % 3]]


@pytest.mark.parametrize("case", PB_CASES, ids=lambda c: f"{c[0][0]}_{c[0][1]}_{c[0][2]}-{c[1]}-{c[2]}")
def test_packbits_decode_bit_ranges(ctx, torch_cuda, case):
    from zarrs_amd import CodecChain
    (dt, first, last), wrap, padding = case
    codecs = PB_WRAPS[wrap](packbits(first, last, padding))
    a = _raw(dt, SHAPE, PB_TYPES.index((dt, first, last)))
    mc = V.ModelChain(codecs, dt, 0, 3)
    enc = mc.encode(a)
    exp = mc.decode(enc, SHAPE)
    assert exp.dtype == a.dtype and exp.tobytes() != a.tobytes()  # bits outside the range are dropped
    ch = CodecChain.from_metadata(codecs, dt, 0, ctx)
    if wrap == "alone":
        assert ch.encoded_size(SHAPE) == len(enc) == V.packbits_size(a.size, dt, first, last, padding)
    check_decode(ch, torch_cuda, enc, SHAPE, exp, case)


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("n", BOOL_COUNTS)
def test_packbits_decode_bool_counts(ctx, torch_cuda, n, padding):
    from zarrs_amd import CodecChain
    a = _raw("bool", [n], n)
    for codecs in ([packbits(padding=padding)], [packbits(padding=padding), GZIP]):
        mc = V.ModelChain(codecs, "bool", 0, 1)
        enc = mc.encode(a)
        assert mc.decode(enc, [n]).tobytes() == a.tobytes()
        ch = CodecChain.from_metadata(codecs, "bool", 0, ctx)
        check_decode(ch, torch_cuda, enc, [n], a, (n, padding, len(codecs)))


def test_packbits_sign_extension_stops_at_the_byte(ctx, torch_cuda):
    """int32 with last_bit = 11 decodes -5 to 65531; int16 decodes it to -5 (the reference fills only
    the byte that holds the sign bit)."""
    from zarrs_amd import CodecChain
    for dt, want in (("int32", 65531), ("int16", -5)):
        ch = CodecChain.from_metadata([packbits(0, 11)], dt, 0, ctx)
        out = np.zeros([2], V.NP[dt])
        ch.decode_into(bytes([0xFB, 0xBF, 0xFF]), [2], out)
        assert out.tolist() == [want, want]


@pytest.mark.parametrize("wrap", ["alone", "gzip"])
@pytest.mark.parametrize("padding", ["first_byte", "last_byte"])
def test_packbits_wrong_padding_byte_fails_its_descriptor_only(ctx, torch_cuda, padding, wrap):
    from zarrs_amd import CodecChain, ZgpuError, make_desc
    from zarrs_amd import _lib as L
    n = 4099
    codecs = PB_WRAPS[wrap](packbits(padding=padding))
    b2b = O.OracleChain.from_metadata([BYTES] + codecs[1:], "uint8", 0, 1)
    arrays = [_raw("bool", [n], 40 + k) for k in range(3)]
    packed = [bytearray(V.packbits_encode(a, "bool", padding=padding)) for a in arrays]
    packed[1][0 if padding == "first_byte" else -1] ^= 0x02
    with pytest.raises(V.PackBitsError):
        V.packbits_decode(bytes(packed[1]), n, "bool", padding=padding)
    encs = [b2b.encode(np.frombuffer(bytes(p), np.uint8)) for p in packed]
    ch = CodecChain.from_metadata(codecs, "bool", 0, ctx)
    for hbm in (True, False):
        out = np.zeros([3 * n], np.bool_)
        descs = [make_desc(_src(e, torch_cuda, hbm), [n], out_start=[k * n]) for k, e in enumerate(encs)]
        with pytest.raises(ZgpuError) as ei:
            ch.decode_batch(descs, out, [3 * n], enc_device=hbm)
        assert ei.value.status == L.CORRUPT_STREAM
        assert out[:n].tobytes() == arrays[0].tobytes() and out[2 * n:].tobytes() == arrays[2].tobytes()
        # the status array: only the middle descriptor failed
        arr = (L.ChunkDesc * 3)(*descs)
        st = (C.c_int32 * 3)()
        flags = (L.ENC_DEVICE if hbm else 0)
        rc = L.load().zgpu_decode_batch(ch._h, 1, arr, 3, out.ctypes.data, L.u64s([3 * n]), flags, st, None)
        assert rc == L.CORRUPT_STREAM and list(st) == [0, L.CORRUPT_STREAM, 0]


def test_packbits_one_byte_short_is_a_size_mismatch(ctx, torch_cuda):
    from zarrs_amd import CodecChain, ZgpuError, make_desc
    from zarrs_amd import _lib as L
    n = 4099
    a = _raw("bool", [n], 7)
    enc = V.packbits_encode(a, "bool", padding="last_byte")
    ch = CodecChain.from_metadata([packbits(padding="last_byte")], "bool", 0, ctx)
    for hbm in (True, False):
        out = np.zeros([2 * n], np.bool_)
        descs = [make_desc(_src(enc, torch_cuda, hbm), [n], out_start=[0]),
                 make_desc(_src(enc[:-1], torch_cuda, hbm), [n], out_start=[n])]
        with pytest.raises(ZgpuError) as ei:
            ch.decode_batch(descs, out, [2 * n], enc_device=hbm)
        assert ei.value.status == L.DECODED_SIZE_MISMATCH
        assert L.last_size_mismatch() == (1, len(enc) - 1, len(enc))
        assert out[:n].tobytes() == a.tobytes()


# ---------------------------------------------------------------------------------------------------
# fixedscaleoffset decode
# ---------------------------------------------------------------------------------------------------
# (decoded type, astype, offset, scale, a fill value whose decode(encode(fill)) differs from it)
FSO_PAIRS = {
    "f32_u8": ("f4", "u1", 1000, 10, 1001.23),
    "f32_i16": ("<f4", "<i2", -3.5, 100, 1.234),
    "f64_i32": ("<f8", "<i4", 0.1, 1000, 2.00049),
    "f64_u16": ("f8", "u2", -50, 7, 0.1),
    "i32_i16": ("<i4", "<i2", 10, 0.5, 13),
    "u64": ("<u8", None, 5, 0.5, 8),
    "f32": ("f4", None, 0.25, 8, 1.3),
}


def _fso_array(pair, seed):
    """values around the offset that encode into range, then NaN, infinities, denormals, values that
    saturate both ways and (64-bit integers) values above 2^53; two all-fill regions"""
    dtype, astype, offset, scale, fill = FSO_PAIRS[pair]
    dt = np.dtype(V.NP[V.v3_name(dtype)])
    rng = np.random.default_rng(seed)
    if dt.kind == "f":
        a = (offset + rng.standard_normal(SHAPE) * 20 / scale * 8).astype(dt)
        tiny = np.finfo(dt).tiny
        special = [np.nan, np.inf, -np.inf, tiny / 4, -tiny / 8, tiny, 1e30, -1e30, offset + 0.5 / scale,
                   offset - 0.5 / scale, offset + 1.5 / scale, offset + 1e6, offset - 1e6, 0.0, -0.0]
    else:
        info = np.iinfo(dt)
        a = rng.integers(max(info.min, -70000), min(info.max, 70000), SHAPE).astype(dt)
        special = [info.max, info.min, info.max - 1, info.min + 1, 0, 1, 7, 8, 9]
        if dt.itemsize == 8:
            special += [2**53 + 1, 2**53 + 3, 2**60 + 12345, 2**63 - 1 if info.min < 0 else 2**63 + 5]
    flat = a.reshape(-1)
    pos = rng.choice(flat.size, 40 * len(special), replace=False)
    flat[pos] = np.tile(np.array(special, dt), 40)
    a[8:12, 8:24, 0:16] = fill  # whole inner chunks at the fill value: omitted from a shard
    a[0:4, 0:8, 24:32] = fill
    return a


def _fso_codec(pair):
    dtype, astype, offset, scale, _ = FSO_PAIRS[pair]
    return fso(dtype, astype, offset, scale)


def _enc_size(pair):
    dtype, astype, _, _, _ = FSO_PAIRS[pair]
    return np.dtype(V.NP[V.v3_name(astype or dtype)]).itemsize


FSO_PLACES = {
    "bytes_zstd": lambda p: [_fso_codec(p), BYTES, ZSTD],
    "big_shuffle": lambda p: [_fso_codec(p), BYTES_BIG, {"name": "numcodecs.shuffle",
                                                           "configuration": {"elementsize": _enc_size(p)}}],
    "before_shard": lambda p: [_fso_codec(p), sh([4, 8, 8], [BYTES, GZIP])],
    "inside_shard": lambda p: [sh([4, 8, 8], [_fso_codec(p), BYTES, ZSTD])],
    "two_transposes": lambda p: [tr([2, 0, 1]), _fso_codec(p), tr([1, 0, 2]), BYTES, CRC],
}


@pytest.fixture(scope="module")
def fso_arrays():
    return {p: _fso_array(p, k) for k, p in enumerate(sorted(FSO_PAIRS))}


@pytest.mark.parametrize("place", sorted(FSO_PLACES))
@pytest.mark.parametrize("pair", sorted(FSO_PAIRS))
def test_fixedscaleoffset_decode(ctx, torch_cuda, fso_arrays, pair, place):
    from zarrs_amd import CodecChain, make_desc
    dtype, astype, offset, scale, fill = FSO_PAIRS[pair]
    data_type = V.v3_name(dtype)
    codecs = FSO_PLACES[place](pair)
    a = fso_arrays[pair]
    mc = V.ModelChain(codecs, data_type, fill, 3)
    enc = mc.encode(a)
    exp = mc.decode(enc, SHAPE)
    assert exp.dtype == a.dtype
    ch = CodecChain.from_metadata(codecs, data_type, fill, ctx)
    assert ch.dtype == a.dtype
    check_decode(ch, torch_cuda, enc, SHAPE, exp, (pair, place))
    if "shard" not in place:
        return
    # a missing inner chunk and a missing shard decode to the decoded form of the encoded fill value,
    # which is not the array's fill value bit for bit
    gone = mc.decoded_fill([1])
    assert gone.tobytes() != np.array([fill], a.dtype).tobytes()
    assert exp[9, 10, 3].tobytes() == gone.tobytes()
    for hbm in (True, False):
        out = np.zeros([32, 32, 32], a.dtype)
        descs = [make_desc(_src(enc, torch_cuda, hbm), SHAPE, out_start=[0, 0, 0]),
                 make_desc(None, SHAPE, [2, 0, 0], [14, 32, 32], [16, 0, 0])]
        assert ch.decode_batch(descs, out, [32, 32, 32], enc_device=hbm) == [0, 0]
        assert out[:16].tobytes() == exp.tobytes()
        assert out[16:30].tobytes() == mc.decoded_fill([14, 32, 32]).tobytes()
        assert not out[30:].any()  # no descriptor covers it: untouched


def test_fixedscaleoffset_before_and_inside_a_shard(ctx, torch_cuda, fso_arrays):
    """Two conversions: f32 -> i16 before sharding_indexed and i16 -> u8 in its inner chain, with a
    bitround between them; the stripped chain decodes u8."""
    from zarrs_amd import CodecChain
    codecs = [fso("f4", "i2", -3.5, 100), sh([4, 8, 8], [{"name": "bitround", "configuration": {"keepbits": 4}},
                                                         fso("i2", "u1", -20, 0.25), BYTES, ZSTD])]
    a = fso_arrays["f32_i16"]
    mc = V.ModelChain(codecs, "float32", 1.234, 3)
    assert mc.enc_type == "uint8" and len(mc.steps) == 3
    enc = mc.encode(a)
    ch = CodecChain.from_metadata(codecs, "float32", 1.234, ctx)
    check_decode(ch, torch_cuda, enc, SHAPE, mc.decode(enc, SHAPE), "both")


# ---------------------------------------------------------------------------------------------------
# bitround decode
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", ["bytes_blosc", "inside_shard"])
def test_bitround_decode_is_the_identity(ctx, torch_cuda, place):
    from zarrs_amd import CodecChain
    br = {"name": "bitround", "configuration": {"keepbits": 3}}
    codecs = [br, BYTES, BLOSC] if place == "bytes_blosc" else [sh([4, 8, 8], [br, BYTES, ZSTD])]
    rng = np.random.default_rng(11)
    a = (rng.standard_normal(SHAPE) * 100).astype(np.float32)
    a[4:8, 8:16, 8:16] = 0
    mc = V.ModelChain(codecs, "float32", 0.0, 3)
    enc = mc.encode(a)
    stored = V.bitround_encode(a, 3, "float32")
    assert stored.tobytes() != a.tobytes()
    ch = CodecChain.from_metadata(codecs, "float32", 0.0, ctx)
    check_decode(ch, torch_cuda, enc, SHAPE, stored, place)


# ---------------------------------------------------------------------------------------------------
# encode
# ---------------------------------------------------------------------------------------------------
def _tensor(torch, a):
    """a device tensor holding a's bytes (torch has no unsigned 16/32/64-bit element types)"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u" and a.dtype.itemsize > 1:
        a = a.view(f"<i{a.dtype.itemsize}")
    return torch.from_numpy(a.copy()).cuda()


def _gpu_encode(ch, torch, a):
    parts = ch.encode_chunks(_tensor(torch, a), list(a.shape), [[0] * a.ndim])
    return bytes(parts[0].cpu().numpy())


FIXED_CHAINS = {
    "packbits_bool_none": ("bool", [4099], [packbits()]),
    "packbits_bool_first": ("bool", [16 * 256 + 1], [packbits(padding="first_byte")]),
    "packbits_bool_last_crc": ("bool", [9], [packbits(padding="last_byte"), CRC]),
    "packbits_u16": ("uint16", SHAPE, [packbits(3, 12, "last_byte")]),
    "packbits_i8": ("int8", SHAPE, [packbits(0, 3)]),
    "packbits_c64": ("complex64", SHAPE, [packbits(16, 31, "first_byte"), CRC]),
    "packbits_i32_transposed": ("int32", SHAPE, [tr([2, 0, 1]), packbits(0, 11)]),
    "packbits_whole_u16": ("uint16", SHAPE, [packbits(0, 15, "first_byte")]),
}


@pytest.mark.parametrize("name", sorted(FIXED_CHAINS))
def test_packbits_encode_bytewise(ctx, torch_cuda, name):
    from zarrs_amd import CodecChain
    dt, shape, codecs = FIXED_CHAINS[name]
    a = _raw(dt, shape, 3)
    mc = V.ModelChain(codecs, dt, 0, len(shape))
    want = mc.encode(a)
    ch = CodecChain.from_metadata(codecs, dt, 0, ctx)
    assert ch.encoded_size(shape) == ch.encoded_bound(shape) == len(want)
    assert _gpu_encode(ch, torch_cuda, a) == want


@pytest.mark.parametrize("b2b", ["gzip", "zstd_crc"])
def test_packbits_encode_under_a_compressor(ctx, torch_cuda, b2b):
    from zarrs_amd import CodecChain
    codecs = PB_WRAPS[b2b](packbits(3, 12, "first_byte"))
    a = _raw("uint16", SHAPE, 5)
    a[4:] &= 0x00F8  # compressible
    mc = V.ModelChain(codecs, "uint16", 0, 3)
    ch = CodecChain.from_metadata(codecs, "uint16", 0, ctx)
    assert ch.encoded_size(SHAPE) == -1 and ch.encoded_bound(SHAPE) > 0
    got = _gpu_encode(ch, torch_cuda, a)
    packed = V.packbits_encode(a, "uint16", 3, 12, "first_byte")
    assert mc.oracle.decode(got, [len(packed)]).tobytes() == packed
    assert mc.decode(got, SHAPE).tobytes() == (a & 0x1FF8).tobytes()


@pytest.mark.parametrize("pair", sorted(FSO_PAIRS))
def test_fixedscaleoffset_encode(ctx, torch_cuda, fso_arrays, pair):
    from zarrs_amd import CodecChain
    dtype, astype, offset, scale, fill = FSO_PAIRS[pair]
    data_type = V.v3_name(dtype)
    a = fso_arrays[pair]
    # fixed-size chains: bytewise
    for place in ("big_shuffle", "two_transposes"):
        codecs = FSO_PLACES[place](pair)
        mc = V.ModelChain(codecs, data_type, fill, 3)
        ch = CodecChain.from_metadata(codecs, data_type, fill, ctx)
        want = mc.encode(a)
        assert ch.encoded_size(SHAPE) == len(want)
        assert _gpu_encode(ch, torch_cuda, a) == want, (pair, place)
    # chains that end in a compressor, sharded or not: what they decode to is the model's encoding
    for place in ("bytes_zstd", "before_shard", "inside_shard"):
        codecs = FSO_PLACES[place](pair)
        mc = V.ModelChain(codecs, data_type, fill, 3)
        ch = CodecChain.from_metadata(codecs, data_type, fill, ctx)
        assert ch.encoded_bound(SHAPE) > 0
        got = _gpu_encode(ch, torch_cuda, a)
        assert mc.oracle.decode(got, SHAPE).tobytes() == mc.encode_values(a).tobytes(), (pair, place)


BITROUND_TYPES = {"float16": 10, "bfloat16": 7, "float32": 23, "float64": 52, "int32": 32, "uint8": 8}


@pytest.mark.parametrize("data_type", sorted(BITROUND_TYPES))
def test_bitround_encode(ctx, torch_cuda, data_type):
    """keepbits 0, 3 and all of them, on every bit pattern class: all-ones mantissas (the carry goes
    into the exponent) and the maximum unsigned value (the add saturates) among them."""
    from zarrs_amd import CodecChain
    full = BITROUND_TYPES[data_type]
    dt = np.dtype(V.NP[data_type])
    width = dt.itemsize * 8
    udt = np.dtype(f"<u{dt.itemsize}")
    rng = np.random.default_rng(width)
    raw = np.frombuffer(rng.bytes(5003 * dt.itemsize), udt).copy()
    mant = V.MANTISSA.get(data_type, 0)
    ones = (1 << mant) - 1 if mant else 0
    special = [(1 << width) - 1, (1 << width) - 2, 0, 1, 2, 3, 5, 7, (1 << (width - 1)), (1 << (width - 1)) - 1,
               ones, ones | (1 << mant), ones | (0x3F << mant) & ((1 << width) - 1), ((1 << width) - 1) ^ ones]
    raw[:len(special)] = np.array(special, dtype=object).astype(udt)
    small = rng.integers(0, 64, 200).astype(udt)  # integers with few significant bits
    raw[100:300] = small
    fill = "0x" + "00" * dt.itemsize if data_type == "bfloat16" else 0
    for keep in (0, 3, full):
        codecs = [{"name": "bitround", "configuration": {"keepbits": keep}}, BYTES]
        want = V.bitround_bits(raw, keep, data_type)
        mc = V.ModelChain(codecs, data_type, 0, 1)
        assert mc.encode(raw.view(dt)) == want.tobytes()
        ch = CodecChain.from_metadata(codecs, data_type, fill, ctx)
        assert ch.encoded_size([raw.size]) == raw.nbytes
        got = _gpu_encode(ch, torch_cuda, raw if data_type == "bfloat16" else raw.view(dt))
        assert got == want.tobytes(), (data_type, keep)
        if keep == full:
            assert got == raw.tobytes()
    # under a compressor
    codecs = [{"name": "bitround", "configuration": {"keepbits": 3}}, BYTES, ZSTD]
    ch = CodecChain.from_metadata(codecs, data_type, fill, ctx)
    got = _gpu_encode(ch, torch_cuda, raw if data_type == "bfloat16" else raw.view(dt))
    oc = O.OracleChain.from_metadata([BYTES, ZSTD], "uint%d" % width, 0, 1)
    assert oc.decode(got, [raw.size]).tobytes() == V.bitround_bits(raw, 3, data_type).tobytes()


# ---------------------------------------------------------------------------------------------------
# array level
# ---------------------------------------------------------------------------------------------------
def test_array_fixedscaleoffset_bitround_sharded_zstd(ctx, torch_cuda):
    """zarrs_amd.Array over a MemoryStore: fixedscaleoffset + bitround + sharded zstd, a subset that
    straddles shards, a missing shard among them."""
    from zarrs_amd.array import Array, MemoryStore
    codecs = [fso("f4", "i2", -3.5, 100), {"name": "bitround", "configuration": {"keepbits": 6}},
              sh([4, 8, 8], [BYTES, ZSTD])]
    fill = 1.234
    shape, chunk = [32, 64, 32], SHAPE
    rng = np.random.default_rng(21)
    full = (rng.standard_normal(shape) * 30).astype(np.float32)
    full[0:8, 0:16, 0:16] = fill
    mc = V.ModelChain(codecs, "float32", fill, 3)
    store = MemoryStore()
    exp = np.zeros(shape, np.float32)
    for i in range(2):
        for j in range(2):
            sl = (slice(16 * i, 16 * i + 16), slice(32 * j, 32 * j + 32), slice(0, 32))
            if (i, j) == (1, 0):
                exp[sl] = mc.decoded_fill(chunk)  # never written
                continue
            enc = mc.encode(np.ascontiguousarray(full[sl]))
            store[f"c/{i}/{j}/0"] = enc
            exp[sl] = mc.decode(enc, chunk)
    meta = {"shape": shape, "data_type": "float32", "fill_value": fill, "codecs": codecs,
            "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": chunk}},
            "chunk_key_encoding": {"name": "default", "configuration": {"separator": "/"}}}
    arr = Array(store, meta, ctx)
    got = arr.retrieve_array_subset([5, 20, 3], [22, 30, 25])
    assert got.dtype == np.float32
    assert got.tobytes() == np.ascontiguousarray(exp[5:27, 20:50, 3:28]).tobytes()
    assert arr.retrieve_array_subset().tobytes() == exp.tobytes()


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codecs,dt", [([fso("f4", "u1", 1000, 10), BYTES], "float32"),
                                       ([{"name": "bitround", "configuration": {"keepbits": 3}}, BYTES], "float32"),
                                       ([packbits()], "bool"),
                                       ([sh([4, 8, 8], [fso("f4", "u1", 1000, 10), BYTES])], "float32")])
def test_plans_refuse_these_chains(ctx, torch_cuda, codecs, dt):
    from zarrs_amd import CodecChain, make_desc
    from zarrs_amd import _lib as L
    ch = CodecChain.from_metadata(codecs, dt, 0, ctx)
    src = torch_cuda.zeros(1 << 16, dtype=torch_cuda.uint8, device="cuda")
    descs = (L.ChunkDesc * 1)(make_desc(src, SHAPE))
    plan = C.c_void_p()
    rc = L.load().zgpu_plan_create(ch._h, 3, descs, 1, L.u64s(SHAPE), L.ENC_DEVICE | L.OUT_DEVICE, C.byref(plan))
    assert rc == L.UNSUPPORTED and not plan.value
    assert "fused plan" in L.last_error()


@pytest.mark.parametrize("name", ["cast_value", "zfp"])
def test_other_value_codecs_are_still_refused(ctx, name):
    from zarrs_amd import CodecChain, ZgpuError
    from zarrs_amd import _lib as L
    with pytest.raises(ZgpuError) as ei:
        CodecChain.from_metadata([{"name": name, "configuration": {}}, BYTES], "float32", 0, ctx)
    assert ei.value.status == L.UNSUPPORTED


def test_packbits_inside_a_shard_is_refused_clearly(ctx):
    from zarrs_amd import CodecChain, ZgpuError
    from zarrs_amd import _lib as L
    with pytest.raises(ZgpuError) as ei:
        CodecChain.from_metadata([sh([4, 8, 8], [packbits()])], "bool", 0, ctx)
    assert ei.value.status == L.UNSUPPORTED and "sharding_indexed" in str(ei.value)
