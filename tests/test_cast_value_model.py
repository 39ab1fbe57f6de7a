"""The exact cast_value model (tests/cast_value_model.py) held to every vector of the reference's unit
tests of the codec and of its bulk kernels, and to the bit patterns the codec's rules pin. Numbers
only; the model itself is written from the rules."""
import struct

import numpy as np
import pytest

import cast_value_model as M


def f32(*xs):
    return [struct.unpack("<I", struct.pack("<f", x))[0] for x in xs]


def f64(*xs):
    return [struct.unpack("<Q", struct.pack("<d", x))[0] for x in xs]


def ints(t, *xs):
    w = M.INTS[t][1]
    return [x & ((1 << w) - 1) for x in xs]


def enc(elems, source, **cfg):
    return M.encode_bits(elems, cfg, source)


def test_wrap_int16_to_int8_is_the_specs_example():
    assert enc(ints("int16", 127, 128, 129, -129), "int16", data_type="int8", out_of_range="wrap") == \
        (ints("int8", 127, -128, -127, 127), None)


def test_wrap_u64_max_to_int8():
    assert enc([2 ** 64 - 1], "uint64", data_type="int8", out_of_range="wrap") == (ints("int8", -1), None)


def test_wrap_float_to_uint8_decodes():
    cfg = {"data_type": "uint8", "out_of_range": "wrap"}
    e, bad = M.encode_bits(f32(255.0, 256.0), cfg, "float32")
    assert (e, bad) == ([255, 0], None)
    assert M.decode_bits(e, cfg, "float32") == (f32(255.0, 0.0), None)


def test_clamp_and_scalar_map_precedence():
    nan = f32(float("nan"))
    assert nan == [0x7FC00000]  # the canonical pattern, which the "NaN" key matches
    got = enc(f32(1.5, 300.0) + nan, "float32", data_type="uint8", out_of_range="clamp",
              scalar_map={"encode": [[1.5, 42], ["NaN", 7]]})
    assert got == ([42, 255, 7], None)


def test_duplicate_key_first_wins():
    assert enc(f32(1.0), "float32", data_type="uint8", scalar_map={"encode": [[1.0, 2], [1.0, 3]]}) == ([2], None)


@pytest.mark.parametrize("rounding,want", [("nearest-even", [2, 2, -2, -2]), ("towards-zero", [1, 2, -1, -2]),
                                           ("towards-positive", [2, 3, -1, -2]), ("towards-negative", [1, 2, -2, -3]),
                                           ("nearest-away", [2, 3, -2, -3])])
def test_rounding_modes_to_integer(rounding, want):
    assert enc(f32(1.5, 2.5, -1.5, -2.5), "float32", data_type="int8", rounding=rounding) == (ints("int8", *want), None)


@pytest.mark.parametrize("rounding,want", [
    ("nearest-even", [18446744073709551616.0, 9007199254740992.0]),
    ("towards-zero", [18446744073709549568.0, 9007199254740992.0]),
    ("towards-positive", [18446744073709551616.0, 9007199254740994.0]),
    ("towards-negative", [18446744073709549568.0, 9007199254740992.0]),
    ("nearest-away", [18446744073709551616.0, 9007199254740994.0])])
def test_large_uint64_to_float64(rounding, want):
    assert enc([2 ** 64 - 1, 9007199254740993], "uint64", data_type="float64", rounding=rounding) == (f64(*want), None)


def test_huge_float_wrap_and_clamp():
    fmax = float(np.finfo(np.float32).max)
    assert enc(f32(fmax, 2.0 ** 127, -fmax), "float32", data_type="uint8", out_of_range="wrap") == ([0, 0, 0], None)
    assert enc(f64(2.0 ** 127), "float64", data_type="uint8", out_of_range="wrap") == ([0], None)
    assert enc(f32(fmax, -fmax), "float32", data_type="uint8", out_of_range="clamp") == ([255, 0], None)
    assert enc(f32(fmax, -fmax), "float32", data_type="int8", out_of_range="clamp") == (ints("int8", 127, -128), None)


def test_integers_round_once_to_float32_and_bfloat16():
    half = (1 << 63) + (1 << 39)
    lower, upper = 0x5F000000, 0x5F000001
    one = lambda v, r, s="uint64", t="float32": M.cast(v & (2 ** 64 - 1), s, t, r)  # noqa: E731
    assert one(half + 1, "nearest-even") == upper
    assert one(half - 1, "nearest-away") == lower
    assert one(half, "nearest-even") == lower
    assert one(half, "nearest-away") == upper
    assert one(half + 1, "towards-zero") == lower
    assert one(half + 1, "towards-positive") == upper
    assert one(half + 1, "towards-negative") == lower
    nhalf = -((1 << 62) + (1 << 38))
    nlower, nupper = 0xDE800000, 0xDE800001
    assert one(nhalf - 1, "nearest-even", "int64") == nupper
    assert one(nhalf + 1, "nearest-away", "int64") == nlower
    assert one(nhalf - 1, "towards-positive", "int64") == nlower
    assert one(nhalf - 1, "towards-negative", "int64") == nupper
    bhalf = (1 << 63) + (1 << 55)
    assert one(bhalf + 1, "nearest-even", t="bfloat16") == 0x5F01
    assert one(bhalf - 1, "nearest-away", t="bfloat16") == 0x5F00


def test_range_check_is_on_the_exact_value():
    assert M.cast(65504, "uint16", "float16") == 0x7BFF
    assert M.cast(65519, "uint16", "float16") is None  # nearest-even alone would give 65504
    assert M.cast(65519, "uint16", "float16", "nearest-even", "clamp") == 0x7C00
    assert M.cast(65519, "uint32", "float16", "towards-zero", "wrap") == 0x7BFF
    assert M.cast(65519, "uint32", "float16", "nearest-even", "wrap") == 0x7C00
    assert M.cast(ints("int32", -65519)[0], "int32", "float16", "towards-positive", "wrap") == 0xFBFF
    assert M.cast(ints("int32", -65519)[0], "int32", "float16", "towards-negative", "wrap") == 0xFC00


def test_float_to_float_rules():
    assert M.cast(0xFFC00001, "float32", "float64") == 0x7FF8000000000000  # sign and payload dropped
    assert M.cast(0xFFC00001, "float32", "float16") == 0x7E00
    assert M.cast(0xFFC00001, "float32", "bfloat16") == 0x7FC0
    assert M.cast(0xFFC00001, "float32", "float32") == 0x7FC00000
    assert M.cast(f64(-0.0)[0], "float64", "float16") == 0x8000
    assert M.cast(f64(1e10)[0], "float64", "float16") is None
    assert M.cast(f64(1e10)[0], "float64", "float16", "nearest-even", "clamp") == 0x7C00  # not 65504
    assert M.cast(f64(float("-inf"))[0], "float64", "float16") == 0xFC00
    assert M.cast(f64(2.0 ** -25)[0], "float64", "float16") == 0  # a tie below the smallest subnormal: to even
    assert M.cast(f64(2.0 ** -25)[0], "float64", "float16", "nearest-away") == 1
    assert M.cast(f64(2.0 ** -24)[0], "float64", "float16") == 1  # subnormals kept
    # one rounding, not through float32: 1 + 2^-11 + 2^-40 is above the float16 tie, and float32 drops the 2^-40
    x = f64(1.0 + 2.0 ** -11 + 2.0 ** -40)[0]
    assert M.cast(x, "float64", "float16") == 0x3C01
    assert M.cast(f64(1.0 + 2.0 ** -11)[0], "float64", "float16") == 0x3C00


def test_scalar_map_compares_bits():
    cfg = {"data_type": "uint8", "scalar_map": {"encode": [[-0.0, 9], ["NaN", 1]]}}
    assert M.encode_bits(f32(0.0, -0.0), cfg, "float32") == ([0, 9], None)
    assert M.encode_bits([0xFFC00001], cfg, "float32") == ([], 0)  # not the canonical NaN: no match
    assert M.scalar_bits("0x7fc00001", "float32") == 0x7FC00001
    assert M.scalar_bits("-Infinity", "bfloat16") == 0xFF80
    with pytest.raises(ValueError):
        M.scalar_bits(1.5, "uint8")
    with pytest.raises(ValueError):
        M.scalar_bits(256, "uint8")


def test_xorshift_input_is_the_references():
    b = M.to_bytes(M.xorshift_elements("uint8", 4), "uint8")
    state = 0x9E3779B97F4A7C15
    want = []
    for _ in range(4):
        state ^= (state << 13) % 2 ** 64
        state ^= state >> 7
        state ^= (state << 17) % 2 ** 64
        want.append(state & 0xFF)
    assert list(b) == want


@pytest.mark.parametrize("s", M.TYPES)
def test_infallible_pairs_never_fail(s):
    for t in M.TYPES:
        for oor in M.OUT_OF_RANGE:
            if not M.infallible(s, t, oor):
                continue
            for r in M.ROUNDINGS:
                for elems in (M.edge_elements(s), M.xorshift_elements(s)):
                    assert M.cast_list(elems, s, t, r, oor)[1] is None, (s, t, r, oor)


def test_edge_lists_hold_what_the_cases_need():
    for t in M.TYPES:
        e = M.edge_elements(t)
        vals = [M.decode(b, t) for b in e]
        small = [v[1] for v in vals if v[0] in ("int", "fin")]
        for k in (0, 1, 2, 3):
            assert k in small, (t, k)
        assert len(e) == len(set(e))


def test_chain_wrapper_round_trips():
    bytes_le = {"name": "bytes", "configuration": {"endian": "little"}}
    cv = {"name": "cast_value", "configuration": {"data_type": "int16", "rounding": "nearest-away"}}
    ch = M.CastModelChain([cv, bytes_le, {"name": "zstd", "configuration": {"level": 1}}], "float64", 0, 1)
    a = np.array([0.5, -0.5, 2.5, 1000.25], "<f8")
    got = ch.decode(ch.encode(a), [4])
    assert got.tolist() == [1.0, -1.0, 3.0, 1000.0] and ch.enc_type == "int16"
    with pytest.raises(M.NotRepresentable) as ei:
        ch.encode(np.array([1.0, np.nan], "<f8"))
    assert ei.value.index == 1
