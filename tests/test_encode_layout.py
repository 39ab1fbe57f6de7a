"""The write path's host layout (zarrs_amd/csrc/encode_layout.cpp) on the CPU: a small C++ program
(tests/c/encode_layout_harness.cpp) linked to libzgpu.so calls encode_layout and the three size functions on
one case and prints them; every field is held to the model (tests/encode_layout_model.py), which is written
from the rules, and to the few figures each case states outright. Every case names the branches of
encode_layout.cpp it reaches (function:branch); BRANCHES lists them all and a branch without a case fails.
(Two throws of bytes_layout have no case because parse_chain lets nothing through to them: a blosc cname the
parser does not know, and a bytes->bytes codec of a kind that has no stage.)"""
import json
import os
import subprocess

import pytest

import encode_layout_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "zarrs_amd", "lib")
CSRC = os.path.join(ROOT, "zarrs_amd", "csrc")

BRANCHES = """
encode_layout:bytes encode_layout:packbits encode_layout:sharded check_transposes:rank
bytes_layout:not-bytes bytes_layout:fused-shuffle bytes_layout:shuffle-not-first bytes_layout:shuffle-elementsize
bytes_layout:checksum bytes_layout:gzip bytes_layout:zlib bytes_layout:zstd bytes_layout:blosc
bytes_layout:blosc-default-shuffle bytes_layout:blosc-after-compressor bytes_layout:bz2 bytes_layout:fixed-walk
bytes_layout:slots bytes_layout:pool-alternates bytes_layout:too-many-checksums blosc_compressor:every-cname
shard_grid:rank shard_grid:not-divisible shard_grid:grid
sharded_layout:around sharded_layout:index-chain sharded_layout:fixed-inner sharded_layout:var-inner
sharded_layout:index-at-start packbits_layout:direct packbits_layout:fixed packbits_layout:compressed
encoded_bound:plain encoded_bound:sharded encoded_bound:unbounded
""".split()

BYTES = {"name": "bytes", "configuration": {"endian": "little"}}
BIG = {"name": "bytes", "configuration": {"endian": "big"}}
CRC = {"name": "crc32c"}
CRC_START = {"name": "crc32c", "configuration": {"location": "start"}}
ADLER = {"name": "numcodecs.adler32"}
FLETCHER = {"name": "numcodecs.fletcher32"}
GZIP = {"name": "gzip", "configuration": {"level": 1}}
ZLIB = {"name": "numcodecs.zlib", "configuration": {"level": 2}}
ZSTD = {"name": "zstd", "configuration": {"level": 3, "checksum": True}}
BZ2 = {"name": "numcodecs.bz2", "configuration": {"level": 1}}
PACKBITS = {"name": "packbits", "configuration": {"first_bit": 1, "last_bit": 5}}


def tr(*order):
    return {"name": "transpose", "configuration": {"order": list(order)}}


def shuffle(es):
    return {"name": "numcodecs.shuffle", "configuration": {"elementsize": es}}


def blosc(cname, **cfg):
    return {"name": "blosc", "configuration": {"cname": cname, "clevel": 4, **cfg}}


def shard(cs, inner, index=(BYTES, CRC), **cfg):
    return {"name": "sharding_indexed", "configuration": {"chunk_shape": list(cs), "codecs": inner,
                                                          "index_codecs": list(index), **cfg}}


def case(codecs, shape, dtype="float32"):
    return {"codecs": codecs, "data_type": dtype, "fill": "00" * 16, "nd": len(shape), "chunk_shape": list(shape)}


F, S = [8, 6], [8, 8]  # 192 bytes of float32; shards of four [4, 4] inner chunks
# name, the branches it reaches, the case, figures stated outright ("err": the refusal's status)
CASES = [
    ("fixed-plain", "encode_layout:bytes encoded_bound:plain", case([BYTES], F), {"path": M.FIXED, "size": 192, "fixed": 1}),
    ("fixed-crc-both-ends", "bytes_layout:checksum bytes_layout:fixed-walk", case([tr(1, 0), BIG, CRC_START, CRC], F),
     {"path": M.FIXED, "size": 200, "data_off": 4, "lo": [4, 0], "in": [192, 196]}),
    ("fixed-three-kinds", "bytes_layout:checksum bytes_layout:fixed-walk", case([BYTES, CRC, ADLER, FLETCHER, CRC_START], [37], "uint8"),
     {"size": 53, "data_off": 8, "lo": [8, 8, 4, 4], "kinds": [0, 5, 6, 0], "at_start": [0, 1, 0, 1]}),
    ("fixed-15-checksums", "bytes_layout:fixed-walk", case([BYTES] + [CRC] * 15, F), {"path": M.FIXED, "size": 252}),
    ("shuffle-fused", "bytes_layout:fused-shuffle", case([BYTES, shuffle(4), CRC], F), {"shuffle": 1, "size": 196, "n_stages": 1}),
    ("shuffle-not-first", "bytes_layout:shuffle-not-first", case([BYTES, CRC, shuffle(4)], F), {"err": M.UNSUPPORTED}),
    ("shuffle-elementsize", "bytes_layout:shuffle-elementsize", case([BYTES, shuffle(2)], F), {"err": M.UNSUPPORTED}),
    ("gzip", "bytes_layout:gzip bytes_layout:slots", case([BYTES, GZIP], F),
     {"path": M.VAR, "size": 242, "headroom": 64, "pitch": 512, "n_pools": 2, "pool": [1], "level": [1], "fixed": 0}),
    ("zlib", "bytes_layout:zlib", case([BYTES, ZLIB], F), {"size": 205, "pitch": 512, "zlib": [1], "level": [2]}),
    ("zstd", "bytes_layout:zstd", case([BYTES, ZSTD], F), {"size": 217, "zstd_checksum": [1], "level": [3]}),
    ("gzip-crc-zstd", "bytes_layout:pool-alternates", case([BYTES, GZIP, CRC, ZSTD], F),
     {"size": 271, "in": [192, 242, 246], "pool": [1, 0, 0], "pitch": 512}),
    ("three-compressors", "bytes_layout:pool-alternates", case([BYTES, ZLIB, GZIP, ZSTD], [24], "uint8"), {"pool": [1, 0, 1]}),
    ("crc-gzip-crc", "bytes_layout:checksum", case([BYTES, CRC, GZIP, CRC_START], F),
     {"in": [192, 196, 196 + 18 + 25 + 4 + 5], "size": 252, "pitch": 512, "data_off": 0}),
    ("gzip-14-checksums", "bytes_layout:slots", case([BYTES] + [CRC_START] * 14 + [GZIP], F), {"path": M.VAR, "pitch": 512}),
    ("gzip-15-checksums", "bytes_layout:too-many-checksums", case([BYTES] + [CRC] * 15 + [GZIP], F), {"err": M.UNSUPPORTED}),
    ("bz2", "bytes_layout:bz2 encoded_bound:plain", case([BYTES, BZ2], F), {"err": M.UNSUPPORTED, "bound": 192 + 24 + 1024, "fixed_size": -1}),
    ("blosc-lz4", "bytes_layout:blosc blosc_compressor:every-cname", case([BYTES, blosc("lz4", shuffle="shuffle", typesize=4, blocksize=64)], F),
     {"size": 208, "blosc": [[1, 1, 4, 64]], "level": [4]}),
    ("blosc-lz4hc", "blosc_compressor:every-cname", case([BYTES, blosc("lz4hc", shuffle="noshuffle", typesize=4)], F), {"blosc": [[1, 0, 4, 0]]}),
    ("blosc-blosclz", "blosc_compressor:every-cname", case([BYTES, blosc("blosclz", shuffle="bitshuffle", typesize=4)], F), {"blosc": [[0, 2, 4, 0]]}),
    ("blosc-snappy", "blosc_compressor:every-cname", case([BYTES, blosc("snappy", shuffle="shuffle", typesize=2)], F), {"blosc": [[2, 1, 2, 0]]}),
    ("blosc-zlib", "blosc_compressor:every-cname", case([BYTES, blosc("zlib", shuffle="shuffle", typesize=4)], F), {"blosc": [[3, 1, 4, 0]]}),
    ("blosc-zstd", "blosc_compressor:every-cname", case([BYTES, blosc("zstd", shuffle="shuffle", typesize=4), CRC], F),
     {"blosc": [[4, 1, 4, 0], [0, 0, 0, 0]], "size": 212}),
    ("blosc-unknown-cname", "", case([BYTES, blosc("lzma")], F), {"parse_err": M.INVALID_ARGUMENT}),
    ("blosc-after-gzip", "bytes_layout:blosc-after-compressor", case([BYTES, GZIP, blosc("lz4", typesize=4)], F), {"err": M.UNSUPPORTED}),
    ("blosc-default-shuffle-typesize", "bytes_layout:blosc-default-shuffle", case([BYTES, blosc("lz4", typesize=4)], F), {"blosc": [[1, 2, 4, 0]]}),
    ("blosc-default-shuffle-no-typesize", "bytes_layout:blosc-default-shuffle", case([BYTES, blosc("lz4")], F), {"blosc": [[1, 0, 1, 0]]}),
    ("packbits-direct", "encode_layout:packbits packbits_layout:direct", case([PACKBITS], F, "uint8"),
     {"path": M.PACKBITS, "direct": 1, "packed_len": 30, "upitch": 48, "ppitch": 32, "size": 30, "fixed": 1}),
    ("packbits-checksums", "packbits_layout:fixed", case([tr(1, 0), PACKBITS, CRC_START, ADLER], F, "uint8"),
     {"direct": 0, "size": 38, "fixed": 1, "packed_data_off": 8}),
    ("packbits-gzip", "packbits_layout:compressed", case([PACKBITS, GZIP], F, "uint8"), {"direct": 0, "fixed": 0, "size": 30 + 18 + 4 + 1 + 5}),
    ("packbits-shuffle", "bytes_layout:shuffle-elementsize", case([PACKBITS, shuffle(2)], F, "uint16"), {"err": M.UNSUPPORTED}),
    ("packbits-transpose-rank", "check_transposes:rank", case([tr(1, 0, 2), PACKBITS], F, "uint8"), {"err": M.INVALID_ARGUMENT}),
    ("shard-fixed", "encode_layout:sharded sharded_layout:fixed-inner shard_grid:grid encoded_bound:sharded", case([shard([4, 4], [BYTES, CRC])], S),
     {"path": M.SHARD_FIXED, "n_inner": 4, "inner_n": 16, "cps": [2, 2], "pitch": 256, "size": 4 * 68 + 68, "index_size": 68, "index_data_off": 0}),
    ("shard-fixed-index-start-2crc", "sharded_layout:index-at-start", case([shard([4, 4], [tr(1, 0), BIG], [BIG, CRC_START, CRC], index_location="start")], S),
     {"index_at_start": 1, "index_big_endian": 1, "index_size": 72, "index_data_off": 4, "index_lo": [4, 0], "size": 4 * 64 + 72}),
    ("shard-fixed-index-0crc", "sharded_layout:fixed-inner", case([shard([4, 4], [BYTES], [BYTES])], S), {"index_size": 64, "size": 320}),
    ("shard-var", "sharded_layout:var-inner", case([shard([4, 4], [BYTES, GZIP, CRC], index_location="end")], S),
     {"path": M.SHARD_VAR, "pitch": 0, "inner_pitch": 256, "index_at_start": 0, "size": 4 * (64 + 18 + 8 + 1 + 5 + 4) + 68}),
    ("shard-var-index-start", "sharded_layout:var-inner sharded_layout:index-at-start", case([shard([4, 4], [BYTES, ZSTD], [BYTES, CRC], index_location="start")], S),
     {"path": M.SHARD_VAR, "index_at_start": 1}),
    ("shard-1d", "shard_grid:grid", case([shard([6], [BYTES, CRC])], [36], "uint8"), {"n_inner": 6, "cps": [6], "size": 6 * 10 + 100}),
    ("shard-transpose-before", "sharded_layout:around encoded_bound:unbounded", case([tr(1, 0), shard([4, 4], [BYTES])], S), {"err": M.UNSUPPORTED, "bound": -1}),
    ("shard-gzip-after", "sharded_layout:around encoded_bound:unbounded", case([shard([4, 4], [BYTES]), GZIP], S), {"err": M.UNSUPPORTED, "bound": -1}),
    ("shard-rank", "shard_grid:rank encoded_bound:unbounded", case([shard([4], [BYTES])], S), {"err": M.INVALID_ARGUMENT, "bound": -1}),
    ("shard-not-divisible", "shard_grid:not-divisible", case([shard([3, 4], [BYTES])], S), {"err": M.INVALID_ARGUMENT, "bound": -1}),
    ("shard-index-adler", "sharded_layout:index-chain", case([shard([4, 4], [BYTES], [BYTES, ADLER])], S), {"err": M.UNSUPPORTED}),
    ("shard-index-transposed", "sharded_layout:index-chain", case([shard([4, 4], [BYTES], [tr(0), BYTES, CRC])], S), {"err": M.UNSUPPORTED}),
    ("shard-nested", "bytes_layout:not-bytes encoded_bound:unbounded", case([shard([4, 4], [shard([2, 2], [BYTES])])], S), {"err": M.UNSUPPORTED, "bound": -1}),
    ("shard-inner-bz2", "bytes_layout:bz2 encoded_bound:sharded", case([shard([4, 4], [BYTES, BZ2])], S), {"err": M.UNSUPPORTED, "bound": 4 * (64 + 8 + 1024) + 68}),
    ("shard-inner-transpose-rank", "check_transposes:rank", case([shard([4, 4], [tr(0, 2, 1), BYTES])], S), {"err": M.INVALID_ARGUMENT}),
    ("transpose-rank", "check_transposes:rank", case([tr(1, 0, 2), BYTES], F), {"err": M.INVALID_ARGUMENT}),
    ("u8-70000-gzip", "bytes_layout:gzip", case([BYTES, GZIP], [70000], "uint8"), {"size": 70000 + 18 + 8750 + 1094 + 5, "pitch": 80128}),
    ("u8-70000-zlib", "bytes_layout:zlib", case([BYTES, ZLIB], [70000], "uint8"), {"size": 70000 + 17 + 4 + 13}),
    ("u8-70000-zstd", "bytes_layout:zstd", case([BYTES, ZSTD], [70000], "uint8"), {"size": 70000 + 22 + 210}),
]
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("enc_layout") / "encode_layout_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "c", "encode_layout_harness.cpp"), "-L" + LIB, "-lzgpu",
                           "-Wl,-rpath," + LIB])
    return exe


@pytest.fixture(scope="module")
def results(harness):
    """every case through the harness, once"""
    out = {}
    for name, _, c, _ in CASES:
        r = subprocess.run([harness, json.dumps(c)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = {"parse_err": int(r.stdout.split()[1])} if r.stdout.startswith("ERR ") else json.loads(r.stdout)
    return out


def test_every_branch_has_a_case():
    reached = {t for _, tags, _, _ in CASES for t in tags.split()}
    assert sorted(set(BRANCHES) - reached) == [] and sorted(reached - set(BRANCHES)) == []
    assert len(set(IDS)) == len(IDS)
    src = open(os.path.join(CSRC, "encode_layout.cpp")).read()
    for t in BRANCHES:  # every tag names a function of encode_layout.cpp
        assert " " + t.split(":")[0] + "(" in src, t


def test_header_needs_no_hip(tmp_path):
    """encode_layout.hpp (and what it includes) compiles with plain g++ and no ROCm include path."""
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "%s"\nint main() { return 0; }\n' % os.path.join(CSRC, "encode_layout.hpp"))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(probe)])
    src = open(os.path.join(CSRC, "encode_layout.cpp")).read()
    assert "#include <hip" not in src and "launch.hpp" not in src and "getenv" not in src


def stages(L, key):
    return [s[key] for s in L["stages"]]


STATED = {  # a stated figure -> where the harness prints it
    "n_stages": lambda L: len(L["stages"]), "kinds": lambda L: stages(L, "kind"),
    **{k: (lambda L, k=k: stages(L, k)) for k in ("lo", "in", "pool", "level", "zlib", "zstd_checksum", "blosc", "at_start")},
    "index_size": lambda L: L["index"]["size"], "index_data_off": lambda L: L["index"]["data_off"],
    "index_lo": lambda L: stages(L["index"], "lo"), "inner_pitch": lambda L: L["inner"]["pitch"],
    "packed_data_off": lambda L: L["packed"]["data_off"],
}


@pytest.mark.parametrize("name,tags,c,stated", CASES, ids=IDS)
def test_layout_matches_the_model(results, name, tags, c, stated):
    J = results[name]
    if "parse_err" in stated:
        assert J == {"parse_err": stated["parse_err"]}
        return
    assert max(c["chunk_shape"]) <= 37 or name.startswith("u8-70000")
    if "err" in stated:
        with pytest.raises(M.LayoutError) as e:
            M.model(c)
        assert e.value.status == stated["err"] and J.get("err") == stated["err"] and "layout" not in J, J
        return
    assert "err" not in J, J
    L = J["layout"]
    for k, v in stated.items():
        assert (STATED[k](L) if k in STATED else L[k]) == v, k
    want = M.model(c)
    for k in sorted(set(L) | set(want)):
        assert L[k] == want[k], k


def chain_of_bounds(L):
    """a [bytes, bytes->bytes codecs] layout's stages hand each other their bounds, from the data to the size"""
    n = L["data_bytes"]
    for s in L["stages"]:
        assert s["in"] == n and s["out"] >= n, s
        n = s["out"]
    assert n == L["size"]
    return n


@pytest.mark.parametrize("name,tags,c,stated", CASES, ids=IDS)
def test_size_functions_agree_with_the_layout(results, name, tags, c, stated):
    """chain_fixed_encoded_size, chain_encoded_bound and encoded_bound (zgpu_chain_encoded_bound) against the
    model, against the stated figures, and against the layout's stage bounds wherever the chain has a layout:
    the size queries and the slots the encoders write into cannot part ways unseen."""
    J = results[name]
    if "parse_err" in stated:
        return
    sz = J["sizes"]
    assert sz == M.sizes(c)
    if "bound" in stated:
        assert sz["bound"] == stated["bound"]
    if "fixed_size" in stated:
        assert sz["fixed"] == stated["fixed_size"]
    if "err" in stated:
        return
    L = J["layout"]
    assert sz["bound"] == L["size"] and sz["fixed"] == (L["size"] if L["fixed"] else -1)
    if L["path"] in (M.FIXED, M.VAR):
        assert sz["chain_bound"] == chain_of_bounds(L)
    elif L["path"] == M.PACKBITS:
        assert L["packed"]["data_bytes"] == L["packed_len"] and sz["chain_bound"] == chain_of_bounds(L["packed"])
    else:
        assert sz["chain_bound"] == -1
        assert sz["bound"] == L["n_inner"] * chain_of_bounds(L["inner"]) + chain_of_bounds(L["index"])
        assert L["index"]["data_bytes"] == 16 * L["n_inner"] and L["index"]["fixed"] == 1
