"""The fused plan's host layout (zarrs_amd/csrc/plan_layout.cpp) on the CPU: a small C++ program
(tests/c/plan_layout_harness.cpp) linked to libzgpu.so calls plan_layout / stages_only_layout on one case
and prints the layout; every field is held to the numpy model (tests/plan_layout_model.py), which is written
from the rules, and to the few figures each case states outright. Every case names the branches of
plan_layout.cpp it reaches (function:branch); BRANCHES lists them all and a branch without a case fails."""
import json
import os
import subprocess

import pytest

import plan_layout_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "zarrs_amd", "lib")
SRC = os.path.join(ROOT, "zarrs_amd", "csrc", "plan_layout.cpp")

BRANCHES = """
resolve_levels:value-codec resolve_levels:plain resolve_levels:no-descs resolve_levels:sharded
resolve_levels:outer-transposes resolve_levels:b2b-after-sharding resolve_levels:nested resolve_levels:around-nested
resolve_levels:three-deep resolve_levels:mid-not-divisible check_transposes:rank
desc_ok:selection-past-chunk desc_ok:other-chunk-shape
plan_layout:zero-extent-full-kept plan_layout:zero-extent-partial-dropped
add_plain_item:present add_plain_item:missing add_plain_item:partial
add_shard_items:not-divisible add_shard_items:mixed-shapes add_shard_items:missing-shard add_shard_items:middle-shards
add_leaves:one-shard add_leaves:middle-shard for_each_cell:one-cell for_each_cell:many-cells
index_spec:spec index_spec:too-many-crc index_spec:at-start
build_leaf_stages:checksum build_leaf_stages:fused-shuffle build_leaf_stages:materialising build_leaf_stages:two-pools
build_leaf_stages:nested-compressor stage_for:every-kind
scatter_params:leaf-transpose scatter_params:outer-strides scatter_params:tile-b
scatter_mode:generic-outer scatter_mode:rows scatter_mode:tiled scatter_mode:generic-shuffle scatter_mode:generic-es16
scatter_mode:persistent scatter_mode:not-persistent
rows_copy_unchanged:swap rows_copy_unchanged:out-stride rows_copy_unchanged:ok
blosc_direct:eligible blosc_direct:partial-item blosc_direct:knob
gzip_direct:eligible gzip_direct:row-24 gzip_direct:nd-4 gzip_direct:knob
blosc_need:ranges blosc_need:none-partial blosc_need:knob
stages_only_layout:checksum stages_only_layout:materialising
""".split()

BYTES = {"name": "bytes", "configuration": {"endian": "little"}}
BIG = {"name": "bytes", "configuration": {"endian": "big"}}
CRC = {"name": "crc32c"}
GZIP = {"name": "gzip", "configuration": {"level": 1}}
ZSTD = {"name": "zstd", "configuration": {"level": 1}}
BLOSC = {"name": "blosc", "configuration": {"cname": "lz4", "clevel": 1, "shuffle": "noshuffle", "typesize": 4, "blocksize": 0}}


def tr(*order):
    return {"name": "transpose", "configuration": {"order": list(order)}}


def shuffle(es):
    return {"name": "numcodecs.shuffle", "configuration": {"elementsize": es}}


def shard(cs, inner, **cfg):
    return {"name": "sharding_indexed", "configuration": {"chunk_shape": list(cs), "codecs": inner, **cfg}}


def desc(chunk, start=None, shape=None, out=None, present=True):
    nd = len(chunk)
    return {"chunk_shape": list(chunk), "sel_start": list(start or [0] * nd), "sel_shape": list(shape or chunk),
            "out_start": list(out or [0] * nd), "present": present}


def case(codecs, out_shape, descs, dtype="float32", fill="00" * 16, validate=True, **knobs):
    assert set(knobs) <= set(M.KNOBS)
    return {"codecs": codecs, "data_type": dtype, "fill": fill, "nd": len(out_shape), "out_shape": list(out_shape),
            "validate": validate, "knobs": {**M.KNOBS, **knobs}, "descs": descs}


IDX5 = [BYTES] + [CRC] * 5
R8 = (2,) * 8
# name, the branches it reaches, the case, figures stated outright ("err": the ChainError's status)
CASES = [
    ("plain-whole", "resolve_levels:plain add_plain_item:present scatter_mode:rows for_each_cell:one-cell",
     case([BYTES], [8, 6], [desc([4, 3]), desc([4, 3], out=[4, 3])]), {"scatter_mode": M.ROWS, "n_items": 2}),
    ("plain-partial-missing", "add_plain_item:partial add_plain_item:missing",
     case([BYTES, CRC], [8, 8], [desc([4, 3], [1, 1], [2, 2], [0, 4]), desc([4, 3], out=[4, 0], present=False)]),
     {"flags": [M.PARTIAL, M.FILL], "alg_bytes_static": 4 * 4 + 1000 + 12 * 4}),
    ("plain-1d", "build_leaf_stages:checksum",
     case([BYTES, CRC, {"name": "numcodecs.adler32"}, {"name": "numcodecs.fletcher32"}], [8], [desc([5], [1], [3], [2])],
          dtype="uint8"), {"stages": [[6, 0, 0, 0], [5, 1, 0, 0], [0, 0, 0, 0]], "n_pools": 0}),
    ("plain-zero-extent-full", "plan_layout:zero-extent-full-kept", case([BYTES], [4, 3], [desc([0, 3])]),
     {"n_items": 1, "status": [0]}),
    ("plain-zero-extent-partial", "plan_layout:zero-extent-partial-dropped",
     case([BYTES], [4, 3], [desc([4, 3], [1, 0], [0, 3]), desc([4, 3])]), {"n_items": 1, "status": [0, 0]}),
    ("plain-selection-past-chunk", "desc_ok:selection-past-chunk",
     case([BYTES], [8, 3], [desc([4, 3], [3, 0], [2, 3]), desc([4, 3], out=[4, 0])]),
     {"n_items": 1, "status": [M.INVALID_ARGUMENT, 0]}),
    ("plain-other-chunk-shape", "desc_ok:other-chunk-shape",
     case([BYTES], [8, 3], [desc([4, 3]), desc([2, 3], out=[4, 0]), desc([4, 3], out=[4, 0])]),
     {"n_items": 2, "status": [0, M.INVALID_ARGUMENT, 0]}),
    ("plain-no-descs", "resolve_levels:no-descs", case([BYTES], [4, 3], []), {"n_items": 0, "scatter_units": 0}),
    ("shard-8x6-crossing", "resolve_levels:sharded add_leaves:one-shard for_each_cell:many-cells index_spec:spec",
     case([shard([4, 3], [BYTES])], [8, 8], [desc([8, 6], [1, 1], [6, 4], [1, 2])], dtype="uint16"),
     {"inner": [0, 1, 2, 3], "n_items": 4, "n_inner": 4, "index_bytes": 68}),
    ("shard-1d-index-at-start", "index_spec:at-start",
     case([shard([2], [BYTES, GZIP], index_location="start", index_codecs=[BIG, {"name": "crc32c", "configuration": {"location": "start"}}, CRC])],
          [8], [desc([8], [3], [4], [1])], validate=False), {"inner": [1, 2, 3], "index_bytes": 72}),
    ("shard-transpose-10", "resolve_levels:outer-transposes scatter_params:outer-strides scatter_mode:generic-outer",
     case([tr(1, 0), shard([4, 3], [BYTES])], [6, 8], [desc([6, 8], [1, 2], [4, 5], [2, 1])]),
     {"scatter_mode": M.GENERIC, "out_stride": [1, 8]}),
    ("shard-transpose-201", "resolve_levels:outer-transposes",
     case([tr(2, 0, 1), shard([4, 2, 3], [BYTES])], [4, 6, 8], [desc([4, 6, 8], [1, 0, 3], [3, 5, 4], [0, 1, 2])], dtype="uint8"),
     {"scatter_mode": M.GENERIC}),
    ("shard-transposes-to-identity", "scatter_mode:rows",
     case([tr(1, 0), tr(1, 0), shard([4, 3], [BYTES])], [8, 6], [desc([8, 6], [3, 2], [2, 2], [0, 0])]),
     {"scatter_mode": M.ROWS, "out_stride": [6, 1]}),
    ("shard-rank8", "resolve_levels:outer-transposes",
     case([tr(7, 6, 5, 4, 3, 2, 1, 0), shard([1, 2, 1, 2, 1, 2, 1, 2], [BYTES])], R8,
          [desc(R8, [0, 1, 0, 0, 1, 0, 0, 0], [2, 1, 2, 2, 1, 2, 1, 2])], dtype="uint8"), {"n_inner": 16}),
    ("shard-missing", "add_shard_items:missing-shard",
     case([shard([4, 3], [BYTES])], [8, 6], [desc([8, 6], present=False)]), {"flags": [M.FILL] * 4, "shards": [[0, 0]]}),
    ("shard-not-divisible", "add_shard_items:not-divisible",
     case([shard([4, 3], [BYTES])], [8, 8], [desc([8, 7]), desc([8, 6])]), {"status": [M.INVALID_ARGUMENT, 0], "n_items": 4}),
    ("shard-other-shape", "add_shard_items:mixed-shapes",
     case([shard([4, 3], [BYTES])], [8, 6], [desc([8, 6], [0, 0], [4, 6]), desc([4, 6], out=[4, 0])]), {"status": [0, M.UNSUPPORTED]}),
    ("nested-8x8", "resolve_levels:nested add_shard_items:middle-shards add_leaves:middle-shard",
     case([shard([4, 4], [shard([2, 2], [BYTES, CRC])])], [8, 8], [desc([8, 8], [1, 3], [6, 3], [0, 0])]),
     {"mid_inner": [0, 1, 2, 3], "n_inner": 4, "n_inner2": 4, "n_items": 8}),
    ("nested-not-divisible", "resolve_levels:mid-not-divisible",
     case([shard([4, 4], [shard([3, 2], [BYTES])])], [8, 8], [desc([8, 8])]), {"err": M.INVALID_ARGUMENT}),
    ("mode-tiled", "scatter_params:leaf-transpose scatter_mode:tiled scatter_mode:not-persistent",
     case([tr(1, 0), BYTES], [4, 6], [desc([4, 6])]), {"scatter_mode": M.TILED, "enc_stride": [1, 4], "tiled_p": 0}),
    ("mode-tiled-3d", "scatter_params:tile-b",
     case([tr(1, 2, 0), BYTES], [2, 3, 4], [desc([2, 3, 4])], dtype="uint16"),
     {"scatter_mode": M.TILED, "tile_a": 0, "tile_b": 1, "enc_stride": [1, 8, 2]}),
    ("mode-generic-fused-shuffle", "build_leaf_stages:fused-shuffle scatter_mode:generic-shuffle",
     case([tr(1, 0), BYTES, shuffle(4)], [4, 6], [desc([4, 6])]), {"scatter_mode": M.GENERIC, "stages": [], "shuffle": 1}),
    ("mode-generic-es16", "scatter_mode:generic-es16",
     case([tr(1, 0), BYTES], [4, 6], [desc([4, 6])], dtype="complex128"), {"scatter_mode": M.GENERIC}),
    ("mode-tiled-persistent", "scatter_mode:persistent",
     case([tr(1, 0), BYTES], [64, 128], [desc([64, 64]), desc([64, 64], out=[0, 64])]),
     {"scatter_mode": M.TILED, "tiled_p": 1, "first_path": M.TILED_PERSISTENT, "origin": [0, 64]}),
    ("mode-tiled-partial-not-persistent", "scatter_mode:not-persistent",
     case([tr(1, 0), BYTES], [64, 128], [desc([64, 64]), desc([64, 64], [0, 0], [64, 32], [0, 64])]),
     {"scatter_mode": M.TILED, "tiled_p": 0, "first_path": M.TILED}),
    ("stages-two-pools", "build_leaf_stages:materialising build_leaf_stages:two-pools stage_for:every-kind",
     case([BYTES, shuffle(2), CRC, ZSTD], [4, 4], [desc([4, 4])]),
     {"stages": [[2, 0, 0, 0], [0, 0, 0, 0], [3, 0, 2, 1]], "n_pools": 2, "slot_bytes": 256}),
    ("stages-zlib-bz2", "stage_for:every-kind",
     case([BYTES, {"name": "numcodecs.zlib", "configuration": {"level": 1}}], [8, 8], [desc([8, 8])]), {"stages": [[7, 0, 0, 0]]}),
    ("stages-bz2", "stage_for:every-kind",
     case([BYTES, CRC, {"name": "numcodecs.bz2", "configuration": {"level": 1}}], [8, 8], [desc([8, 8])]),
     {"stages": [[8, 0, 0, 0], [0, 0, 0, 0]], "slot_bytes": 512}),
    ("gzip-direct", "gzip_direct:eligible rows_copy_unchanged:ok",
     case([shard([4, 4], [BYTES, GZIP])], [8, 8], [desc([8, 8])]), {"gz_direct": 1, "lbs": 4, "want": 64}),
    ("gzip-direct-row-24", "gzip_direct:row-24", case([BYTES, GZIP], [4, 8], [desc([4, 6])]), {"gz_direct": 0}),
    ("gzip-direct-nd-4", "gzip_direct:nd-4", case([BYTES, GZIP], [2, 2, 2, 4], [desc([2, 2, 2, 4])]), {"gz_direct": 0}),
    ("gzip-direct-big-endian", "rows_copy_unchanged:swap", case([BIG, GZIP], [4, 4], [desc([4, 4])]), {"gz_direct": 0, "swap": 1}),
    ("gzip-direct-out-stride", "rows_copy_unchanged:out-stride", case([BYTES, GZIP], [4, 6], [desc([4, 4])]), {"gz_direct": 0}),
    ("gzip-direct-knob", "gzip_direct:knob", case([BYTES, GZIP], [4, 4], [desc([4, 4])], gzip_direct=False), {"gz_direct": 0}),
    ("blosc-direct", "blosc_direct:eligible blosc_need:none-partial",
     case([BYTES, BLOSC], [4, 8], [desc([4, 4]), desc([4, 4], out=[0, 4])]), {"bl_direct": 1, "bl_need": []}),
    ("blosc-direct-partial-item", "blosc_direct:partial-item",
     case([BYTES, BLOSC], [4, 8], [desc([4, 4]), desc([4, 4], [0, 0], [2, 4], [0, 4])]), {"bl_direct": 0}),
    ("blosc-direct-knob", "blosc_direct:knob", case([BYTES, BLOSC], [4, 8], [desc([4, 4])], blosc_no_direct=True), {"bl_direct": 0}),
    ("blosc-need-under-transpose", "blosc_need:ranges",
     case([tr(1, 0), BYTES, BLOSC], [8, 8], [desc([4, 6], [1, 2], [2, 3], [0, 0]), desc([4, 6], out=[4, 0], present=False)]),
     {"bl_need": [(2 * 4 + 1) * 4, (4 * 4 + 2 + 1) * 4, 0, -1]}),
    ("blosc-need-knob", "blosc_need:knob",
     case([BYTES, BLOSC], [4, 8], [desc([4, 6], [1, 2], [2, 3])], blosc_no_partial=True), {"bl_need": []}),
    ("unshuffle-wide-knob", "build_leaf_stages:fused-shuffle", case([BYTES, shuffle(2)], [4, 8], [desc([4, 8])], dtype="uint16", unshuffle_wide=2),
     {"pad0": 2, "shuffle": 1}),
    ("err-value-codec", "resolve_levels:value-codec",
     case([{"name": "bitround", "configuration": {"keepbits": 3}}, BYTES], [4], [desc([4])]), {"err": M.UNSUPPORTED}),
    ("err-packbits", "resolve_levels:value-codec",
     case([{"name": "packbits", "configuration": {"first_bit": 3, "last_bit": 12}}], [4], [desc([4])], dtype="uint16"), {"err": M.UNSUPPORTED}),
    ("err-b2b-after-sharding", "resolve_levels:b2b-after-sharding", case([shard([2], [BYTES]), GZIP], [4], [desc([4])]), {"err": M.UNSUPPORTED}),
    ("err-around-nested", "resolve_levels:around-nested",
     case([shard([4], [shard([2], [BYTES]), CRC])], [8], [desc([8])]), {"err": M.UNSUPPORTED}),
    ("err-three-deep", "resolve_levels:three-deep",
     case([shard([4], [shard([2], [shard([1], [BYTES])])])], [8], [desc([8])]), {"err": M.UNSUPPORTED}),
    ("err-transpose-rank", "check_transposes:rank", case([tr(1, 0, 2), BYTES], [4, 4], [desc([4, 4])]), {"err": M.INVALID_ARGUMENT}),
    ("err-outer-transpose-rank", "check_transposes:rank",
     case([tr(1, 0, 2), shard([2, 2], [BYTES])], [4, 4], [desc([4, 4])]), {"err": M.INVALID_ARGUMENT}),
    ("err-nested-compressor", "build_leaf_stages:nested-compressor", case([BYTES, GZIP, ZSTD], [4], [desc([4])]), {"err": M.UNSUPPORTED}),
    ("err-index-crcs", "index_spec:too-many-crc", case([shard([2], [BYTES], index_codecs=IDX5)], [4], [desc([4])]), {"err": M.UNSUPPORTED}),
]
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("layout") / "plan_layout_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "c", "plan_layout_harness.cpp"), "-L" + LIB, "-lzgpu",
                           "-Wl,-rpath," + LIB])
    return exe


def run(exe, c):
    r = subprocess.run([exe, json.dumps(c)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    if r.stdout.startswith("ERR "):
        status, _, msg = r.stdout[4:].strip().partition(" ")
        return {"err": int(status), "msg": msg}
    return json.loads(r.stdout)


def test_every_branch_has_a_case():
    reached = {t for _, tags, _, _ in CASES for t in tags.split()} | {"stages_only_layout:checksum", "stages_only_layout:materialising"}
    assert sorted(set(BRANCHES) - reached) == [] and sorted(reached - set(BRANCHES)) == []
    assert len(set(IDS)) == len(IDS)
    src = open(SRC).read()
    for t in BRANCHES:  # every tag names a function of plan_layout.cpp
        assert " " + t.split(":")[0] + "(" in src, t


def test_header_needs_no_hip(tmp_path):
    """plan_layout.hpp (and common.hpp under it) compile with plain g++ and no ROCm include path."""
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "%s"\nint main() { return 0; }\n' % os.path.join(ROOT, "zarrs_amd", "csrc", "plan_layout.hpp"))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(probe)])


@pytest.mark.parametrize("name,tags,c,stated", CASES, ids=IDS)
def test_model_is_sane(name, tags, c, stated):
    """Without the library: the model's boxes cover every selected element once and stay inside."""
    if "err" in stated:
        with pytest.raises(M.LayoutError) as e:
            M.model(c)
        assert e.value.status == stated["err"]
        return
    extents = list(c["out_shape"]) + [x for d in c["descs"] for x in d["chunk_shape"]]
    assert 1 <= c["nd"] <= 3 or set(extents) <= {1, 2} or name == "gzip-direct-nd-4"  # (whose point is its rank)
    assert max(extents) <= 8 or name.startswith("mode-tiled-p")  # (the persistent kernel's tiles are 64 x 64)
    L, boxes = M.model(c)
    M.check_cover(c, L, boxes)


STATED = {  # a stated figure -> where the harness prints it
    "n_items": lambda J: len(J["items"]), "flags": lambda J: [i[3] for i in J["items"]], "inner": lambda J: [i[5] for i in J["items"]],
    "mid_inner": lambda J: [m[5] for m in J["mids"]], "status": lambda J: J["item_desc_status"],
    "n_inner": lambda J: J["ispec"]["n_inner"], "n_inner2": lambda J: J["ispec2"]["n_inner"],
    "index_bytes": lambda J: J["ispec"]["index_bytes"], "lbs": lambda J: J["gz"]["lbs"], "want": lambda J: J["gz"]["want"],
    **{k: (lambda J, k=k: J["scatter"][k]) for k in ("out_stride", "enc_stride", "tile_a", "tile_b", "swap", "shuffle", "pad0")},
}


@pytest.mark.parametrize("name,tags,c,stated", CASES, ids=IDS)
def test_layout_matches_the_model(harness, name, tags, c, stated):
    J = run(harness, c)
    if "err" in stated:
        assert J.get("err") == stated["err"], J
        return
    assert "err" not in J, J
    for k, v in stated.items():
        assert (STATED[k](J) if k in STATED else J[k]) == v, k
    L, _ = M.model(c)
    nd, es = c["nd"], M.ES[c["data_type"]]
    for k in ("items", "geom", "item_desc_status", "shards", "mids", "ispec", "ispec2", "stages", "slot_bytes", "n_pools",
              "scatter_mode", "scatter_units", "tiled_p", "origin", "first_path", "sharded", "nested", "alg_bytes_static",
              "bl_direct", "gz_direct", "bl_need", "no_scatter"):
        assert J[k] == L[k], k
    for k, v in L["scatter"].items():
        if v is not None:
            assert J["scatter"][k] == v, k
    assert bytes(J["scatter"]["fill"][:es]) == bytes.fromhex(c["fill"])[:es] and J["leaf_es"] == es
    if L["gz_direct"]:
        assert J["gz"] == L["gz"]
    if L["tiled_p"]:
        assert J["tiled_upi"] == L["scatter_units"]


@pytest.mark.parametrize("kind,n_pools,tag", [(0, 0, "stages_only_layout:checksum"), (1, 1, "stages_only_layout:materialising")])
def test_stages_only_layout(harness, kind, n_pools, tag):
    assert tag in BRANCHES
    J = run(harness, {"stages_only": {"kind": kind, "at_start": 1 - kind, "elementsize": 0, "slot_bytes": 1000,
                                      "items": [[4096, 77], [8192, 99], [12288, 5]]}})
    assert J["stages"] == [[kind, 1 - kind, 0, 0]] and J["n_pools"] == n_pools and J["slot_bytes"] == 1024
    assert J["no_scatter"] == 1 and J["item_desc_status"] == [0, 0, 0]
    assert J["items"] == [[4096, 77, 0, 0, 0, 0], [8192, 99, 1, 0, 0, 0], [12288, 5, 2, 0, 0, 0]]
    assert J["geom"] == [] and J["shards"] == [] and J["sharded"] == 0 and J["scatter"]["nelem"] == 0
