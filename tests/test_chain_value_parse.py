"""Parsing and binding of numcodecs.fixedscaleoffset, bitround and packbits in the chain model
(zarrs_amd/csrc/chain.cpp), on the CPU: a small C++ program (tests/c/chain_parse_harness.cpp) linked to
libzgpu.so calls parse_chain, as tests/test_c_harness.py links the C ABI. The expected encoded fill
values come from the numpy model (tests/value_codecs.py)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import value_codecs as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "zarrs_amd", "lib")
INVALID_ARGUMENT, UNSUPPORTED = 10, 6  # include/zgpu.h (test_status_numbers_match_the_header)
BYTES = {"name": "bytes", "configuration": {"endian": "little"}}
IDX = [BYTES, {"name": "crc32c"}]


def fso(dtype, astype=None, offset=1000, scale=10, **extra):
    cfg = {"offset": offset, "scale": scale, "dtype": dtype, **extra}
    if astype is not None:
        cfg["astype"] = astype
    return {"name": "numcodecs.fixedscaleoffset", "configuration": cfg}


def bitround(keepbits, name="bitround"):
    return {"name": name, "configuration": {"keepbits": keepbits}}


def packbits(**cfg):
    return {"name": "packbits", "configuration": cfg}


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
    fb = np.array([fill], V.NP[data_type]).tobytes().hex()
    r = subprocess.run([exe, json.dumps(codecs), data_type, fb, str(nelem)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    head, _, rest = r.stdout.strip().partition(" ")
    if head == "ERR":
        status, _, msg = rest.partition(" ")
        return {"err": int(status), "msg": msg}
    return dict(kv.split("=", 1) for kv in rest.split(" "))


def test_status_numbers_match_the_header():
    txt = open(os.path.join(ROOT, "include", "zgpu.h")).read()
    assert int(re.search(r"ZGPU_INVALID_ARGUMENT = (\d+)", txt).group(1)) == INVALID_ARGUMENT
    assert int(re.search(r"ZGPU_UNSUPPORTED = (\d+)", txt).group(1)) == UNSUPPORTED


def test_fixedscaleoffset_retypes_the_rest_of_the_chain(harness):
    r = parse(harness, [fso("<f4", "|u1"), BYTES], "float32", 1001.23)
    want = V.fso_encode(np.array([1001.23], np.float32), 1000, 10, "f4", "u1")
    assert r["enc_type"] == "uint8" and r["enc_fill"] == want.tobytes().hex() == "0c"
    assert r["size"] == r["bound"] == "100" and r["value"] == "1" and r["a2b"] == "bytes"
    # no astype: the data type stays, the fill value is still encoded
    r = parse(harness, [fso("f8", offset=0.5, scale=4), BYTES], "float64", 3.3)
    assert r["enc_type"] == "float64"
    assert r["enc_fill"] == V.fso_encode(np.array([3.3]), 0.5, 4, "f8").tobytes().hex()
    assert r["size"] == "800"
    # a one-byte encoded type needs no endian; the decoded type's two bytes would
    r = parse(harness, [fso("i2", "i1"), {"name": "bytes"}], "int16")
    assert r["enc_type"] == "int8" and r["size"] == "100"
    assert parse(harness, [fso("i1", "i2"), {"name": "bytes"}], "int8")["err"] == INVALID_ARGUMENT
    # entries are sorted by kind: the value codec binds first wherever it stands
    r = parse(harness, [BYTES, fso("f4", "u2")], "float32")
    assert r["enc_type"] == "uint16" and r["size"] == "200"
    # crc32c and a compressor see the encoded width
    r = parse(harness, [fso("f4", "u1"), BYTES, {"name": "crc32c"}], "float32")
    assert r["size"] == "104"


def test_fixedscaleoffset_configuration_errors(harness):
    assert parse(harness, [fso("f4", "u1", bogus=1), BYTES], "float32")["err"] == INVALID_ARGUMENT
    assert parse(harness, [{"name": "numcodecs.fixedscaleoffset", "configuration": {"offset": 0, "dtype": "f4"}}, BYTES],
                 "float32")["err"] == INVALID_ARGUMENT
    assert parse(harness, [fso("float", "u1"), BYTES], "float32")["err"] == INVALID_ARGUMENT
    assert parse(harness, [fso("f8", "u1"), BYTES], "float32")["err"] == UNSUPPORTED  # dtype != the array's
    assert parse(harness, [fso("f2", "u1"), BYTES], "float16")["err"] == UNSUPPORTED  # not an element type
    assert parse(harness, [fso("f4", "f2"), BYTES], "float32")["err"] == UNSUPPORTED
    # a codec zarrs would create stays an error with must_understand false
    opt = dict(fso("f8", "u1"), must_understand=False)
    assert parse(harness, [opt, BYTES], "float32")["err"] == UNSUPPORTED


def test_bitround_keeps_the_type_and_rounds_the_fill(harness):
    for name in ("bitround", "numcodecs.bitround"):
        r = parse(harness, [bitround(3, name), BYTES], "float32", 1.2345679)
        assert r["enc_type"] == "float32" and r["enc_fill"] == np.float32(1.25).tobytes().hex()
        assert r["value"] == "1" and r["a2a"] == "1"
    for dt in ("float16", "float64", "int8", "uint8", "int32", "uint64"):
        assert parse(harness, [bitround(2), BYTES], dt)["enc_type"] == dt
    assert parse(harness, [bitround(2), BYTES], "complex64")["err"] == UNSUPPORTED
    assert parse(harness, [bitround(2), BYTES], "bool")["err"] == UNSUPPORTED
    assert parse(harness, [{"name": "bitround", "configuration": {"keepbits": 2, "x": 1}}, BYTES], "float32")["err"] \
        == INVALID_ARGUMENT
    assert parse(harness, [{"name": "bitround", "configuration": {}}, BYTES], "float32")["err"] == INVALID_ARGUMENT
    assert parse(harness, [bitround(-1), BYTES], "float32")["err"] == INVALID_ARGUMENT


def test_value_codecs_mix_with_transposes_and_sharding(harness):
    t = {"name": "transpose", "configuration": {"order": [1, 0]}}
    r = parse(harness, [t, fso("f4", "i2"), t, bitround(3), shard([fso("i2", "u1", 0, 1), BYTES], (2, 2))], "float32")
    assert r["a2a"] == "4" and r["enc_type"] == "int16" and r["inner_enc_type"] == "uint8" and r["value"] == "1"
    r = parse(harness, [shard([bitround(3), BYTES])], "float32")
    assert r["a2a"] == "0" and r["value"] == "1"
    assert parse(harness, [shard([BYTES])], "float32")["value"] == "0"


def test_packbits_binding(harness):
    r = parse(harness, [packbits()], "bool", 0, 9)
    assert (r["a2b"], r["bits"], r["comp"], r["size"], r["bound"]) == ("packbits", "0..0", "1", "2", "2")
    r = parse(harness, [packbits(padding_encoding="first_byte")], "bool", 0, 9)
    assert r["size"] == "3" and r["padding"] == "1"
    r = parse(harness, [packbits(first_bit=3, last_bit=12, padding_encoding="last_byte"), {"name": "crc32c"}], "uint16", 0, 4)
    assert r["bits"] == "3..12" and r["size"] == str(5 + 1 + 4) and r["padding"] == "2" and r["signed"] == "0"
    r = parse(harness, [packbits(last_bit=11)], "int32", 0, 3)
    assert r["signed"] == "1" and r["size"] == "5" and r["comp"] == "32"
    r = parse(harness, [packbits(first_bit=16, last_bit=None)], "complex64", 0, 3)
    assert r["bits"] == "16..31" and r["comp"] == "32" and r["ncomp"] == "2"
    assert r["size"] == str(3 * 2 * 16 // 8)
    r = parse(harness, [packbits(first_bit=16)], "float32", 0, 3)
    assert r["size"] == "6" and r["signed"] == "0"
    # under a compressor the bound starts from the packed size
    r = parse(harness, [packbits(), {"name": "gzip", "configuration": {"level": 1}}], "bool", 0, 4099)
    assert r["size"] == "-1" and int(r["bound"]) > 513
    # a fixedscaleoffset before it: the bit range is bound to the encoded type
    r = parse(harness, [fso("f4", "u1"), packbits(last_bit=3)], "float32", 0, 10)
    assert r["comp"] == "8" and r["size"] == "5"
    assert parse(harness, [fso("f4", "u1"), packbits(last_bit=8)], "float32")["err"] == INVALID_ARGUMENT


def test_packbits_whole_component_is_bytes(harness):
    """The reference's fast path: all bits of a byte-sized component are `bytes` little-endian, with no
    padding byte whatever padding_encoding says, and such chains keep the fused plan."""
    for dt, es in (("uint8", 1), ("int16", 2), ("float32", 4), ("complex64", 8)):
        r = parse(harness, [packbits(padding_encoding="first_byte")], dt, 0, 10)
        assert r["a2b"] == "bytes" and r["size"] == str(10 * es)
    assert parse(harness, [packbits(first_bit=0, last_bit=15)], "uint16")["a2b"] == "bytes"
    assert parse(harness, [packbits(first_bit=0, last_bit=14)], "uint16")["a2b"] == "packbits"


def test_packbits_configuration_errors(harness):
    assert parse(harness, [packbits(first_bit=5, last_bit=4)], "uint16")["err"] == INVALID_ARGUMENT
    assert parse(harness, [packbits(last_bit=16)], "uint16")["err"] == INVALID_ARGUMENT
    assert parse(harness, [packbits(last_bit=1)], "bool")["err"] == INVALID_ARGUMENT
    assert parse(harness, [packbits(padding_encoding="start_byte")], "bool")["err"] == INVALID_ARGUMENT
    assert parse(harness, [packbits(bits=3)], "bool")["err"] == INVALID_ARGUMENT
    assert parse(harness, [packbits(first_bit=-1)], "uint8")["err"] == INVALID_ARGUMENT
    assert parse(harness, [packbits(), BYTES], "bool")["err"] == INVALID_ARGUMENT  # two array->bytes codecs
    r = parse(harness, [shard([packbits()])], "bool")
    assert r["err"] == UNSUPPORTED and "sharding_indexed" in r["msg"]


@pytest.mark.parametrize("name", ["cast_value", "zfp", "reshape", "zarrs.squeeze", "numcodecs.pcodec", "zarrs.gdeflate",
                                  "vlen-utf8", "zarrs.optional"])
def test_other_zarrs_codecs_stay_refused(harness, name):
    for mu in (True, False):
        r = parse(harness, [{"name": name, "configuration": {}, "must_understand": mu}, BYTES], "float32")
        assert r["err"] == UNSUPPORTED
