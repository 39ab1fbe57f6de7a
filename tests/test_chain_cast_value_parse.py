"""Parsing and binding of cast_value in the chain model (zarrs_amd/csrc/chain.cpp), on the CPU, through
tests/c/chain_parse_harness.cpp as tests/test_chain_value_parse.py does for the other value codecs. The
expected encoded fill values come from the exact model (tests/cast_value_model.py)."""
import json
import os
import subprocess

import pytest

import cast_value_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "zarrs_amd", "lib")
INVALID_ARGUMENT, UNSUPPORTED = 10, 6  # include/zgpu.h
BYTES = {"name": "bytes", "configuration": {"endian": "little"}}
IDX = [BYTES, {"name": "crc32c"}]


def cv(data_type, **cfg):
    return {"name": "cast_value", "configuration": {"data_type": data_type, **cfg}}


def shard(inner, cs=(4,)):
    return {"name": "sharding_indexed", "configuration": {"chunk_shape": list(cs), "codecs": inner, "index_codecs": IDX}}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain") / "chain_parse_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "c", "chain_parse_harness.cpp"), "-L" + LIB, "-lzgpu",
                           "-Wl,-rpath," + LIB])
    return exe


def parse(exe, codecs, data_type, fill=0, nelem=100):
    fb = M.to_bytes([M.scalar_bits(fill, data_type)], data_type).hex() if data_type in M.TYPES else "00" * 16
    r = subprocess.run([exe, json.dumps(codecs), data_type, fb, str(nelem)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    head, _, rest = r.stdout.strip().partition(" ")
    if head == "ERR":
        status, _, msg = rest.partition(" ")
        return {"err": int(status), "msg": msg}
    return dict(kv.split("=", 1) for kv in rest.split(" "))


def enc_fill(codec, data_type, fill):
    out, bad = M.encode_bits([M.scalar_bits(fill, data_type)], codec["configuration"], data_type)
    assert bad is None
    return M.to_bytes(out, M.target_of(codec["configuration"])).hex()


def test_the_rest_of_the_chain_sees_the_target_type(harness):
    c = cv("int16", rounding="nearest-away")
    r = parse(harness, [c, BYTES, {"name": "crc32c"}], "float64", 3.0)
    assert r["enc_type"] == "int16" and r["value"] == "1" and r["a2a"] == "1"
    assert r["enc_fill"] == enc_fill(c, "float64", 3.0) == "0300"
    assert r["size"] == str(100 * 2 + 4)  # crc32c over 2-byte elements
    r = parse(harness, [cv("float64"), BYTES, {"name": "zstd"}], "uint8", 7)
    assert r["enc_type"] == "float64" and r["enc_fill"] == M.to_bytes([M.scalar_bits(7.0, "float64")], "float64").hex()
    assert int(r["bound"]) >= 800 and r["size"] == "-1"
    # without an endian the bytes codec is bound to the target: a 1-byte target needs none, a wider one does
    assert parse(harness, [cv("uint8", out_of_range="clamp"), "bytes"], "float32")["enc_type"] == "uint8"
    assert parse(harness, [cv("float32"), "bytes"], "uint8")["err"] == INVALID_ARGUMENT


@pytest.mark.parametrize("data_type,fill,codec", [
    ("float32", "NaN", cv("uint8", out_of_range="clamp", scalar_map={"encode": [["NaN", 0]], "decode": [[0, "NaN"]]})),
    ("float32", 300.0, cv("uint8", out_of_range="clamp", scalar_map={"encode": [[300.0, 255]], "decode": [[255, 300.0]]})),
    ("float32", 1.0, cv("bfloat16")),
    ("float64", -0.0, cv("float16", rounding="towards-zero")),
    ("int8", -56, cv("uint8", out_of_range="wrap")),
    ("uint64", 2 ** 64 - 2 ** 11, cv("float64")),
    ("int16", -3, cv("int64")),
    ("bfloat16", "0x3f80", cv("float32")),
    ("float16", "-Infinity", cv("float64")),
])
def test_encoded_fill(harness, data_type, fill, codec):
    r = parse(harness, [codec, BYTES], data_type, fill)
    assert r["enc_type"] == M.target_of(codec["configuration"])
    assert r["enc_fill"] == enc_fill(codec, data_type, fill)


def test_scalar_map_values_read_as_fill_values(harness):
    # the first of two equal keys wins; a hex-bits key; a uint64 key past int64; an integer for a float key
    c = cv("uint8", scalar_map={"encode": [[5, 1], [5, 2]]})
    assert parse(harness, [c, BYTES], "float32", 5.0)["err"] == INVALID_ARGUMENT  # 1 does not decode back to 5.0
    c = cv("uint8", scalar_map={"encode": [[5, 1], [5, 2]], "decode": [[1, 5.0]]})
    assert parse(harness, [c, BYTES], "float32", 5.0)["enc_fill"] == "01"
    c = cv("uint8", scalar_map={"encode": [["0x7fc00001", 9]], "decode": [[9, "0x7fc00001"]]})
    assert parse(harness, [c, BYTES], "float32", "0x7fc00001")["enc_fill"] == "09"
    c = cv("int8", scalar_map={"encode": [[18446744073709551615, -1]], "decode": [[-1, 18446744073709551615]]})
    assert parse(harness, [c, BYTES], "uint64", 18446744073709551615)["enc_fill"] == "ff"


def test_entry_order_and_object_data_type(harness):
    c = cv({"name": "int16"}, rounding="towards-negative")
    a = parse(harness, [c, BYTES, {"name": "crc32c"}], "float32", -1.0)
    b = parse(harness, [{"name": "crc32c"}, BYTES, c], "float32", -1.0)
    assert a == b and a["enc_type"] == "int16" and a["enc_fill"] == "ffff"
    assert parse(harness, [cv({"name": "int16", "configuration": {}}), BYTES], "float32")["enc_type"] == "int16"


def test_value_codecs_compose_and_bind_through_sharding(harness):
    fso = {"name": "numcodecs.fixedscaleoffset", "configuration": {"offset": 1000, "scale": 10, "dtype": "<f4"}}
    r = parse(harness, [fso, cv("int16"), BYTES, {"name": "zstd"}], "float32", 1000.0)
    assert r["enc_type"] == "int16" and r["a2a"] == "2" and r["enc_fill"] == "0000"
    br = {"name": "bitround", "configuration": {"keepbits": 3}}
    r = parse(harness, [br, cv("bfloat16"), BYTES], "float32", 1.0)
    assert r["enc_type"] == "bfloat16" and r["enc_fill"] == "803f"
    r = parse(harness, [cv("uint8", out_of_range="clamp"), shard([BYTES, {"name": "crc32c"}])], "float32", 3.0)
    assert r["a2b"] == "sharding" and r["enc_type"] == "uint8" and r["inner_enc_type"] == "uint8" and r["enc_fill"] == "03"
    r = parse(harness, [shard([cv("uint8", out_of_range="clamp"), BYTES])], "float32", 3.0)
    assert r["a2b"] == "sharding" and r["enc_type"] == "float32" and r["inner_enc_type"] == "uint8" and r["value"] == "1"


@pytest.mark.parametrize("target", ["int2", "int4", "uint2", "uint4", "float8_e4m3", "float8_e5m2", "float4_e2m1fn",
                                    "bool", "complex64", "complex128", "r16", "string"])
def test_other_target_types_are_unsupported(harness, target):
    for mu in (True, False):
        c = dict(cv(target), must_understand=mu)
        r = parse(harness, [c, BYTES], "float32")
        assert r["err"] == UNSUPPORTED and target in r["msg"]
        assert parse(harness, [dict(cv("int16"), must_understand=mu), BYTES], "float32")["enc_type"] == "int16"


@pytest.mark.parametrize("source", ["bool", "complex64"])
def test_other_source_types_are_unsupported(harness, source):
    r = parse(harness, [cv("uint8"), BYTES], source)
    assert r["err"] == UNSUPPORTED and source in r["msg"]
    assert parse(harness, [cv("uint8"), BYTES], "int8")["enc_type"] == "uint8"


def test_refusals(harness):
    def err(codec, dt="float32", fill=0):
        return parse(harness, [codec, BYTES], dt, fill)
    # wrap needs an integer target (the reference: UnsupportedDataType)
    for t in M.FLOATS:
        assert err(cv(t, out_of_range="wrap"), "int32")["err"] == UNSUPPORTED
    assert "err" not in err(cv("int8", out_of_range="wrap"), "int32")
    # deny_unknown_fields, bad enum strings, malformed maps
    assert err(cv("uint8", astype="u1"))["err"] == INVALID_ARGUMENT
    assert err(cv("uint8", rounding="nearest"))["err"] == INVALID_ARGUMENT
    assert err(cv("uint8", rounding=1))["err"] == INVALID_ARGUMENT
    assert err(cv("uint8", out_of_range="saturate"))["err"] == INVALID_ARGUMENT
    assert err(cv("uint8", out_of_range=""))["err"] == INVALID_ARGUMENT
    assert err(cv(8))["err"] == INVALID_ARGUMENT
    for sm in ([], {"both": []}, {"encode": {}}, {"encode": [[1.0]]}, {"encode": [[1.0, 2, 3]]}, {"encode": [1.0, 2]},
               {"encode": [[1.0, 256]]}, {"encode": [[1.0, -1]]}, {"encode": [[1.0, 1.5]]}, {"encode": [["nan", 1]]},
               {"encode": [["0x7fc0", 1]]}, {"decode": [[1.0, 1.0]]}, {"decode": [[1, [1.0]]]}, {"encode": [[True, 1]]}):
        assert err(cv("uint8", scalar_map=sm))["err"] == INVALID_ARGUMENT, sm
    assert err(cv("uint64", scalar_map={"decode": [[18446744073709551616, 0.0]]}))["err"] == INVALID_ARGUMENT
    # more scalar_map entries than the kernel argument holds
    many = [[float(k), k] for k in range(M.MAP_MAX + 1)]
    r = err(cv("uint8", scalar_map={"encode": many}))
    assert r["err"] == UNSUPPORTED and "scalar_map" in r["msg"]
    assert "err" not in err(cv("uint8", scalar_map={"encode": many[:M.MAP_MAX]}))
    # the fill value
    r = err(cv("uint8"), fill="NaN")
    assert r["err"] == INVALID_ARGUMENT
    r = err(cv("uint8"), fill=300.0)
    assert r["err"] == INVALID_ARGUMENT
    r = err(cv("uint8", out_of_range="clamp"), fill=300.0)
    assert r["err"] == INVALID_ARGUMENT and "cast_value fill value does not survive a round-trip cast" in r["msg"]
    r = err(cv("int16"), fill=0.5)
    assert r["err"] == INVALID_ARGUMENT and "round-trip" in r["msg"]
    r = err(cv("uint8", scalar_map={"encode": [["NaN", 0]]}), fill="NaN")  # 0 decodes to 0.0
    assert r["err"] == INVALID_ARGUMENT and "round-trip" in r["msg"]
    # an invalid configuration of an optional codec is skipped, an unsupported one is not
    assert parse(harness, [dict(cv("uint8", rounding="nearest"), must_understand=False), BYTES], "float32")["value"] == "0"
    assert parse(harness, [dict(cv("float32", out_of_range="wrap"), must_understand=False), BYTES], "int8")["err"] == UNSUPPORTED


def test_a_configuration_without_data_type_is_not_the_v1_form(harness):
    for cfg in ({}, {"rounding": "nearest-even"}):
        for mu in (True, False):
            r = parse(harness, [{"name": "cast_value", "configuration": cfg, "must_understand": mu}, BYTES], "float32")
            assert r["err"] == UNSUPPORTED and "configuration variant is unsupported" in r["msg"]
