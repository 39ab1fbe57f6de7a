"""The numpy model of numcodecs.fixedscaleoffset, bitround and packbits (tests/value_codecs.py) against
hand-checked vectors and zarrs' own bitround fixtures. The GPU tests hold the kernels to this model."""
import json
import os

import numpy as np
import pytest

import value_codecs as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref", "codec", "bitround")
BYTES = {"name": "bytes", "configuration": {"endian": "little"}}


# ---- bitround ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bitround_float32", "bitround_uint8"])
def test_bitround_fixture_is_fixed_point_and_decodes(name):
    root = os.path.join(GOLDEN, name + ".zarr")
    meta = json.load(open(os.path.join(root, "zarr.json")))
    stored = open(os.path.join(root, "c", "0"), "rb").read()
    dt, shape = meta["data_type"], meta["shape"]
    values = np.frombuffer(stored, V.NP[dt])
    assert values.size == shape[0]
    keep = meta["codecs"][0]["configuration"]["keepbits"]
    assert V.bitround_encode(values, keep, dt).tobytes() == stored  # already rounded
    mc = V.ModelChain(meta["codecs"], dt, meta["fill_value"], 1)
    assert mc.decode(stored, shape).tobytes() == stored
    assert mc.encode(values) == stored


def test_bitround_hand_vectors():
    f = np.array([0.0, 1.2345679, -8.358719, 98765.43], np.float32)
    assert V.bitround_encode(f, 3, "float32").tolist() == [0.0, 1.25, -8.0, 98304.0]
    u = np.array([0, 1024, 1280, 1664, 1685, 123145182, 4294967295], np.uint32)
    assert V.bitround_encode(u, 3, "uint32").tolist() == [0, 1024, 1280, 1536, 1792, 117440512, 3758096384]
    b = np.array([0, 3, 7, 15, 17, 54, 89, 128, 255], np.uint8)
    assert V.bitround_encode(b, 3, "uint8").tolist() == [0, 3, 7, 16, 16, 56, 96, 128, 224]
    # all-ones mantissa: the carry goes into the exponent (1.9999999 -> 2.0)
    assert V.bitround_encode(np.array([0x3FFFFFFF], np.uint32).view(np.float32), 3, "float32").tolist() == [2.0]
    # the add saturates instead of wrapping: 0xFFFF_FFFF as float32 bits stays at the top
    assert V.bitround_bits(np.array([0xFFFFFFFF], np.uint32), 3, "float32").tolist() == [0xFFF00000]
    # keepbits >= the mantissa: unchanged
    assert V.bitround_encode(f, 23, "float32").tobytes() == f.tobytes()


# ---- packbits ---------------------------------------------------------------------------------------
def test_packbits_nine_bools():
    a = np.array([1, 0, 0, 1, 0, 0, 1, 0, 1], np.bool_)
    enc = V.packbits_encode(a, "bool")
    assert enc == bytes([0b01001001, 0b00000001])
    assert V.packbits_decode(enc, 9, "bool").tolist() == a.tolist()
    assert V.packbits_size(9, "bool") == 2


def test_packbits_uint16_bits_3_to_12():
    a = np.array([0xFFFF, 0x0008, 0x1000, 0x0AB8], np.uint16)
    # 10-bit fields 0x3FF, 0x001, 0x200, 0x157, least significant first
    word = 0x3FF | (0x001 << 10) | (0x200 << 20) | (0x157 << 30)
    enc = V.packbits_encode(a, "uint16", 3, 12)
    assert enc == word.to_bytes(5, "little")
    assert V.packbits_decode(enc, 4, "uint16", 3, 12).tolist() == [0x1FF8, 0x0008, 0x1000, 0x0AB8]


def test_packbits_sign_extension_stops_at_the_byte():
    for dt, want in (("int32", 65531), ("int16", -5)):
        a = np.array([-5], V.NP[dt])
        enc = V.packbits_encode(a, dt, 0, 11)
        assert enc == bytes([0xFB, 0x0F])
        assert V.packbits_decode(enc, 1, dt, 0, 11).tolist() == [want]
    # an unsigned type is never extended
    assert V.packbits_decode(bytes([0xFB, 0x0F]), 1, "uint16", 0, 11).tolist() == [0x0FFB]


@pytest.mark.parametrize("n,pad", [(8, 0), (7, 1), (1, 7)])
def test_packbits_padding_byte(n, pad):
    a = np.ones(n, np.bool_)
    body = V.packbits_encode(a, "bool")
    assert len(body) == 1
    assert V.packbits_encode(a, "bool", padding="first_byte") == bytes([pad]) + body
    assert V.packbits_encode(a, "bool", padding="last_byte") == body + bytes([pad])
    for p in ("first_byte", "last_byte"):
        enc = V.packbits_encode(a, "bool", padding=p)
        assert V.packbits_decode(enc, n, "bool", padding=p).tolist() == a.tolist()
        bad = bytearray(enc)
        bad[0 if p == "first_byte" else -1] ^= 1
        with pytest.raises(V.PackBitsError):
            V.packbits_decode(bytes(bad), n, "bool", padding=p)
    with pytest.raises(V.PackBitsError):
        V.packbits_decode(body + b"\0", n, "bool")


@pytest.mark.parametrize("dt,first,last", [("uint8", 0, 7), ("int8", 0, 3), ("uint16", 3, 12), ("int16", 0, 15),
                                           ("float32", 0, 31), ("complex64", 0, 31), ("uint64", 0, 62)])
def test_packbits_round_trip_of_representable_values(dt, first, last):
    rng = np.random.default_rng(3)
    bits, ncomp, udt, signed = V._components(dt)
    comps = rng.integers(0, 1 << (last - first + 1), 37 * ncomp, dtype=np.uint64) << np.uint64(first)
    a = comps.astype(udt).view(V.NP[dt])
    enc = V.packbits_encode(a, dt, first, last)
    assert len(enc) == V.packbits_size(37, dt, first, last)
    back = V.packbits_decode(enc, 37, dt, first, last)
    if signed and last % 8 != 7:  # the sign fill changes values whose top extracted bit is set
        top = (comps >> np.uint64(last)) & np.uint64(1)
        keep = top.astype(bool) == 0
        assert back.view(udt)[keep].tolist() == a.view(udt)[keep].tolist()
    else:
        assert back.tobytes() == a.tobytes()


# ---- fixedscaleoffset -------------------------------------------------------------------------------
def test_fso_f32_to_u8_hand_vector():
    # (x - 1000) * 10, rounded half away from zero, saturated into u8
    x = np.array([1000.0, 1000.25, 1000.05, 1012.5, 1025.5, 1030.0, 990.0, np.nan, np.inf, -np.inf], np.float32)
    enc = V.fso_encode(x, 1000, 10, "f4", "u1")
    #            0      2.5->3   0.5(f32: 0.49987793)->0  125  255  300->255  -100->0  nan->0  inf->255  -inf->0
    assert enc.dtype == np.uint8
    assert enc.tolist() == [0, 3, 0, 125, 255, 255, 0, 0, 255, 0]
    dec = V.fso_decode(enc, 1000, 10, "<f4", "|u1")
    assert dec.dtype == np.float32
    assert dec.tolist() == [1000.0, np.float32(1000.3), 1000.0, 1012.5, 1025.5, 1025.5, 1000.0, 1000.0, 1025.5, 1000.0]
    # ties away from zero on both sides (half to even would give 2 and -2)
    t = np.array([1000.25, 999.75], np.float32)
    assert V.fso_encode(t, 1000, 10, "f4", "i1").tolist() == [3, -3]


def test_fso_i32_astype_i16_goes_through_f64_and_f32():
    x = np.array([0, 7, -7, 100000, -100000, 2**31 - 1, -2**31, 16777217], np.int32)
    enc = V.fso_encode(x, 1, 0.5, "<i4", "<i2")
    # (x - 1) * 0.5 in f64, rounded away, as i32; then as f32, as i16 (saturating)
    assert enc.tolist() == [-1, 3, -4, 32767, -32768, 32767, -32768, 32767]
    dec = V.fso_decode(enc, 1, 0.5, "i4", "i2")
    assert dec.dtype == np.int32
    assert dec.tolist() == [-1, 7, -7, 65535, -65535, 65535, -65535, 65535]
    # same type through `astype`: the cast through f32 still runs and loses the low bits of 2^24 + 1
    same = V.fso_encode(np.array([16777217], np.int32), 0, 1, "i4", "i4")
    assert same.tolist() == [16777216]
    assert V.fso_encode(np.array([16777217], np.int32), 0, 1, "i4").tolist() == [16777217]


def test_fso_saturating_casts_never_use_numpys_own():
    big = np.array([2.0**63, -2.0**63, 2.0**64, 1e300, -1e300, np.nan, 2.0**53 + 2], np.float64)
    assert V.sat_cast(big, "<i8").tolist() == [2**63 - 1, -2**63, 2**63 - 1, 2**63 - 1, -2**63, 0, 2**53 + 2]
    assert V.sat_cast(big, "<u8").tolist() == [2**63, 0, 2**64 - 1, 2**64 - 1, 0, 0, 2**53 + 2]
    assert V.sat_cast(np.array([-0.9, 255.9, 256.0, -1.0], np.float32), "u1").tolist() == [0, 255, 255, 0]
    assert V.sat_cast(np.array([-128.9, -129.0, 127.9, 128.0], np.float32), "i1").tolist() == [-128, -128, 127, 127]


@pytest.mark.parametrize("dt,astype,offset,scale", [("u1", None, 3, 1), ("i2", None, -100, 2), ("<i4", "<i2", 10, 1),
                                                    ("u8", None, 0, 1), ("f8", "i4", 0.5, 4), ("f4", "u2", -8, 16)])
def test_fso_round_trip_where_lossless(dt, astype, offset, scale):
    rng = np.random.default_rng(5)
    np_dt = np.dtype(V.NP[V.v3_name(dt)])
    if np_dt.kind == "f":
        x = (rng.integers(0, 1000, 64) / scale + offset).astype(np_dt)  # exact multiples of 1 / scale
    else:
        x = (rng.integers(0, 100, 64) + int(offset)).astype(np_dt)
    enc = V.fso_encode(x, offset, scale, dt, astype)
    assert enc.dtype == np.dtype(V.NP[V.v3_name(astype or dt)])
    assert V.fso_decode(enc, offset, scale, dt, astype).tobytes() == x.tobytes()


def test_model_chain_strips_and_retypes_through_sharding():
    codecs = [{"name": V.FSO, "configuration": {"offset": 1000, "scale": 10, "dtype": "f4", "astype": "u1"}},
              {"name": "sharding_indexed", "configuration": {
                  "chunk_shape": [4], "index_codecs": [BYTES, {"name": "crc32c"}],
                  "codecs": [{"name": "bitround", "configuration": {"keepbits": 2}}, BYTES]}}]
    mc = V.ModelChain(codecs, "float32", 1001.23, 1)
    assert mc.enc_type == "uint8" and mc.enc_fill == 12  # round(12.3) = 12, bitround keeps 0b1100
    assert [c["name"] for c in mc.stripped] == ["sharding_indexed"]
    assert [c["name"] for c in mc.stripped[0]["configuration"]["codecs"]] == ["bytes"]
    a = np.full(8, 1001.23, np.float32)
    a[:4] = [1000, 1000.5, 1002.55, 1025.5]
    enc = mc.encode(a)
    assert len(enc) == 4 + 2 * 16 + 4  # the all-fill inner chunk is omitted
    dec = mc.decode(enc, [8])
    # fixedscaleoffset gives 0, 5, 25, 255; bitround (2 bits from the top set bit, ties to even, the add
    # saturating) makes them 0, 4, 24, 192
    assert dec.tolist() == V.fso_decode(np.array([0, 4, 24, 192, 12, 12, 12, 12], np.uint8), 1000, 10, "f4", "u1").tolist()
    assert mc.decoded_fill([2]).tolist() == [np.float32(1001.2)] * 2
    assert mc.decoded_fill([1]).tobytes() != np.float32(1001.23).tobytes()
