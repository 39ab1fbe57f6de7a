"""tests/plan_replay.py held to its CPU references, and its scripts to the transitions they claim, all
asserted from the bytes the plans will be given. No GPU.

Every variant's statuses and arrays come from one reference (shard_model.read_shard, the oracle over
libzstd and c-blosc, Python's zlib / bz2, the suite's checksum checkers); here a second, independent
one is put beside it wherever there is one: the arrays the shards were built from, the C oracle's own
sharding, the hand-built cases' `expect`, numpy's restatement of a transpose or an unshuffle."""
import bz2
import zlib

import numpy as np
import pytest

import oracle as O
import plan_replay as R
import shard_model as SM
import zstd_frames as Z
from scatter_cases import fill_bytes

ALL = list(R.FAMILIES)


def _sel(a, d):
    return a[tuple(slice(s, s + n) for s, n in zip(d.sel_start, d.sel_shape))]


@pytest.mark.parametrize("name", ALL)
def test_shape_of_every_family(name):
    """Equal descriptor lengths across ALL variants, scripts of at most 8 known variants, expectations of
    the selection's shape and type, the size-mismatch detail where the first failure is one."""
    f = R.family(name)
    assert list(f.modes) == R.MODE_NAMES[name]
    assert 2 <= len(f.script) <= 8 and set(f.script) <= set(f.variants)
    lens = f.lengths()
    for v in f.variants.values():
        assert len(v.enc) == len(v.status) == len(v.expect) == len(f.descs), v.name
        assert [0 if e is None else len(e) for e in v.enc] == lens, v.name
        for d, e, st, x in zip(f.descs, v.enc, v.status, v.expect):
            assert (e is None) == d.null
            if st == R.OK:
                assert x.shape == tuple(d.sel_shape) and x.dtype == f.np_dtype(), v.name
            if d.null:
                assert st == R.OK and x.tobytes() == R.fill_array(d.sel_shape, f.dtype).tobytes()
        first = next((i for i, s in enumerate(v.status) if s), None)
        if first is not None and v.status[first] == R.DECODED_SIZE_MISMATCH:
            assert v.mismatch is not None and v.mismatch[0] == first, v.name
        else:
            assert v.mismatch is None, v.name
    # consecutive executes of a script differ in their bytes unless the script repeats the variant on purpose
    for a, b in zip(f.script, f.script[1:]):
        assert a == b or f.variants[a].enc != f.variants[b].enc


def _built_from(f, v):
    """The arrays a sharded variant was built from, the fill value where an entry is empty"""
    out = []
    for sp in v.facts["specs"]:
        a = sp.a.copy()
        for k, b in enumerate(SM.boxes(a.shape, f.codecs[0]["configuration"]["chunk_shape"])):
            if k in sp.empty:
                a[b] = f.fill()
        out.append(a)
    return out


@pytest.mark.parametrize("name", ["shard_gzip_crc", "shard_gzip_crc_partial", "shard_zlib", "shard_bz2", "checksum_ranges_adler32",
                                  "checksum_ranges_fletcher32", "checksum_ranges_crc32c"])
def test_sharded_expectations_are_the_arrays_they_were_built_from(name):
    f = R.family(name)
    for v in f.variants.values():
        for d, st, x, a in zip(f.descs, v.status, v.expect, _built_from(f, v)):
            if st == R.OK:
                assert x.tobytes() == np.ascontiguousarray(_sel(a, d)).tobytes(), (v.name, d)


@pytest.mark.parametrize("name", ["shard_gzip_crc", "shard_gzip_crc_partial", "nested"])
def test_the_c_oracle_reads_the_same(name):
    """The oracle's own sharding_indexed (index, entries, inner chains, the partial reader's unverified
    crc32c) against shard_model's statuses and arrays."""
    f = R.family(name)
    nd = len(f.chunk_shape)
    oc = O.OracleChain.from_metadata(f.codecs, f.dtype, fill_bytes(f.dtype), nd)
    for v in f.variants.values():
        for d, e, st, x in zip(f.descs, v.enc, v.status, v.expect):
            try:
                got = O.retrieve_array_subset(oc, f.chunk_shape, f.chunk_shape, {(0,) * nd: e}, d.sel_start, d.sel_shape)
                assert st == R.OK and got.tobytes() == x.tobytes(), (v.name, d)
            except O.OracleError as err:
                assert err.status == st, (v.name, d, err.status, st)


def _entries(f, e):
    cfg = f.codecs[0]["configuration"]
    sh = SM.Shard(tuple(cfg["chunk_shape"]), None, location=cfg["index_location"])
    return SM.entries_of(sh, f.chunk_shape, e)


@pytest.mark.parametrize("name", ["shard_gzip_crc", "shard_gzip_crc_partial"])
def test_shard_gzip_crc_transitions(name):
    f = R.family(name)
    partial = name.endswith("partial")
    assert f.script == ["A", "A", "B", "C", "B", "D", "A"]
    ent = {v: [_entries(f, e) for e in f.variants[v].enc] for v in "ABCD"}
    for s in range(2):
        a, b, d = ent["A"][s], ent["B"][s], ent["D"][s]
        assert all(isinstance(x, bytes) for x in a)  # A: all present
        assert [k for k, x in enumerate(b) if x == "empty"] == [3, 7]
        assert [k for k, x in enumerate(d) if x == "empty"] == [0] and isinstance(d[3], bytes) and isinstance(d[7], bytes)
        lens = [len(x) for x in b if isinstance(x, bytes)]
        assert max(lens) > 512 + 18 and min(lens) < 200  # stored members beside compressed ones
    # A in canonical order, B reversed with gaps: read from the index words themselves
    sh = SM.Shard(R.GZ_INNER, None, location="start" if partial else "end")
    x = SM.index_bytes(16, ("end",))

    def offsets(e):
        idx = SM.parse_index(e[:x] if partial else e[len(e) - x:], 16, "little", ("end",))
        return [o for o, n in idx if o != SM.MAX], [n for o, n in idx if o != SM.MAX]
    oa, na = offsets(f.variants["A"].enc[0])
    assert all(o1 + n1 == o2 for o1, n1, o2 in zip(oa, na, oa[1:]))
    ob, nb = offsets(f.variants["B"].enc[0])
    assert all(o2 + n2 + 3 == o1 for o1, o2, n2 in zip(ob, ob[1:], nb[1:]))
    # C: inner 5's crc32c, inner 9's DEFLATE stream, shard 1's index checksum
    c0 = ent["C"][0]
    assert SM.decode_inner(SM.GZ_CRC, c0[5], R.GZ_INNER, "float32", True, False)[0] == R.INVALID_CHECKSUM
    assert SM.decode_inner(SM.GZ_CRC, c0[5], R.GZ_INNER, "float32", True, True)[0] == R.OK
    assert SM.decode_inner(SM.GZ_CRC, c0[9], R.GZ_INNER, "float32", True, False)[0] == R.CORRUPT_STREAM
    assert c0[9][:-4] == R.corrupt_deflate().enc("gz")
    assert ent["C"][1] == R.INVALID_CHECKSUM and isinstance(ent["B"][1], list)
    assert ent["D"][1][6] == R.SHARD_INDEX_OOB
    want = {"A": [0, 0], "B": [0, 0], "C": [R.CORRUPT_STREAM if partial else R.INVALID_CHECKSUM, R.INVALID_CHECKSUM],
            "D": [0, R.SHARD_INDEX_OOB]}
    assert {v: f.variants[v].status for v in "ABCD"} == want
    # what a clean read resolves, for the counters: every inner chunk met, the present entries' sizes
    for v in "AB":
        sizes = sum(len(x) for e in ent[v] for x in e if isinstance(x, bytes))
        assert f.variants[v].counters == {"enc_bytes": sizes, "items": 32}
    assert f.variants["C"].counters is None and f.variants["D"].counters is None
    del sh


def test_shard_zlib_transitions():
    f = R.family("shard_zlib")
    assert f.script == ["A", "B", "C", "A"]
    b, c = _entries(f, f.variants["B"].enc[0]), _entries(f, f.variants["C"].enc[0])
    assert [k for k in range(16) if b[k] != c[k]] == [9] and c[9][:-4] == b[9][:-4]  # only the Adler-32 differs
    zlib.decompress(b[9])
    with pytest.raises(zlib.error):
        zlib.decompress(c[9])
    assert [f.variants[v].status for v in "ABC"] == [[0, 0], [0, 0], [R.CORRUPT_STREAM, 0]]


@pytest.mark.parametrize("kind", ["adler32", "fletcher32", "crc32c"])
def test_checksum_ranges_transitions(kind):
    """Three ranges against under one, from the entries' sizes; the wrong checksum from the checker."""
    f = R.family(f"checksum_ranges_{kind}")
    assert f.script == ["long", "short", "long_bad", "short"]
    size = {v: [len(_entries(f, e)[0]) for e in f.variants[v].enc] for v in f.variants}
    for v in ("long", "long_bad"):
        assert 2 * R.CK_RANGE < size[v][0] <= 3 * R.CK_RANGE and size[v][1] < R.CK_RANGE
    assert size["short"][0] < R.CK_RANGE and 2 * R.CK_RANGE < size["short"][1] <= 3 * R.CK_RANGE
    from test_checksum_models import CK_RANGE
    assert CK_RANGE == R.CK_RANGE
    assert [f.variants[v].status for v in f.script] == [[0, 0], [0, 0], [R.INVALID_CHECKSUM, 0], [0, 0]]
    good, bad = _entries(f, f.variants["long"].enc[0])[0], _entries(f, f.variants["long_bad"].enc[0])[0]
    assert good[:-4] == bad[:-4] and good[-4:] != bad[-4:]


def test_shard_bz2_transitions():
    import bz2_streams as BZ
    f = R.family("shard_bz2")
    assert f.script == ["one", "three", "one"]
    for v, n in (("one", 1), ("three", 3)):
        ent = _entries(f, f.variants[v].enc[0])
        assert len(ent) == 8
        for k, e in enumerate(ent):
            assert BZ._bit_count(e, BZ.BLOCK_MAGIC) == n, (v, k)
            assert bz2.decompress(e) == f.variants[v].expect[0][k].tobytes()
    assert set(f.modes) == {"default", "rounds"} and f.modes["rounds"] == {"ZGPU_BZ2_SCRATCH_MB": "1"}


def test_nested_transitions():
    f = R.family("nested")
    assert f.script == ["present", "empty", "bad_crc", "present"]
    cfg = f.codecs[0]["configuration"]
    mid_cfg = cfg["codecs"][0]["configuration"]
    assert cfg["codecs"][0]["name"] == "sharding_indexed" and tuple(mid_cfg["chunk_shape"]) == R.N_LEAF
    mid = SM.Shard(R.N_LEAF, None, location=mid_cfg["index_location"])
    outer = {v: _entries(f, f.variants[v].enc[0]) for v in f.variants}
    assert isinstance(outer["present"][1], bytes) and outer["empty"][1] == "empty" and isinstance(outer["bad_crc"][1], bytes)
    assert isinstance(SM.entries_of(mid, R.N_MID, outer["present"][1]), list)
    assert SM.entries_of(mid, R.N_MID, outer["bad_crc"][1]) == R.INVALID_CHECKSUM
    assert all(isinstance(SM.entries_of(mid, R.N_MID, outer["bad_crc"][k]), list) for k in (0, 2, 3))
    assert [f.variants[v].status for v in f.script] == [[0, 0], [0, 0], [R.INVALID_CHECKSUM, 0], [0, 0]]
    e = f.variants["empty"].expect[0]
    assert e[0:4, 6:12].tobytes() == R.fill_array((4, 6), "uint16").tobytes()


def test_zstd_chunks_transitions():
    f = R.family("zstd_chunks_u8")
    assert f.script == ["A", "B", "A", "C", "B", "D", "A"] and set(f.modes) == set(R.ZSTD_PATH_NAMES)
    from test_gpu_zstd_frames import PATHS
    assert f.modes == PATHS
    items = R.zstd_items()
    nblk = {v: [len(Z.blocks(e)) for e, _ in it] for v, it in items.items()}
    assert all(len(Z.walk(e)) == 1 and Z.zstd_decompress(e, R.ZN) == Z.text(R.ZN, 70 + i) for i, (e, _) in enumerate(items["A"]))
    for i in range(R.ZK):
        if i == 4:  # the serial item: more blocks than the pipeline's records
            assert not Z.fits_parallel(items["C"][i][0], R.ZN) and nblk["C"][i] == Z.layout(R.ZN)[0] + 1
            continue
        assert nblk["C"][i] < nblk["B"][i], i
        kinds = {t for t, _ in Z.blocks(items["C"][i][0])}
        assert kinds == ({Z.RLE} if i % 2 else {Z.RAW}), i
    assert all(Z.fits_parallel(e, R.ZN) for v in "AB" for e, _ in items[v])
    assert all(n >= 17 and Z.CMP in {t for t, _ in Z.blocks(e)} for n, (e, _) in zip(nblk["B"], items["B"]))  # chains of tiny blocks
    # hand-built frames: the oracle's bytes are the reference executor's
    for v in "BC":
        for i, (_, c) in enumerate(items[v]):
            if c is not None:
                assert f.variants[v].expect[i].tobytes() == c.expect, (v, i)
    # D: libzstd refuses the reserved block type; the short frame is a whole frame of 4000 bytes
    with pytest.raises(RuntimeError):
        Z.zstd_decompress(R.reserved_block_frame(), R.ZN + 64)
    assert len(Z.zstd_decompress(items["D"][1][0], R.ZN)) == 4000 and len(Z.zstd_decompress(items["D2"][2][0], R.ZN)) == 3000
    assert f.variants["D"].status == [0, R.DECODED_SIZE_MISMATCH, 0, R.CORRUPT_STREAM, 0, 0]
    assert f.variants["D2"].status == [0, 0, R.DECODED_SIZE_MISMATCH, 0, 0, 0]
    assert [f.variants[v].status for v in "ABC"] == [[0] * 6] * 3
    # the padding is a trailing skippable frame
    for v in f.variants.values():
        for e, (raw, _) in zip(v.enc, items[v.name]):
            assert e.startswith(raw) and e[len(raw):len(raw) + 4] == Z.skippable(b"")[:4] and len(Z.walk(e)) == len(Z.walk(raw))


def test_zstd_shuffle_chain_is_the_unshuffled_plain_chain():
    u8, u16 = R.family("zstd_chunks_u8"), R.family("zstd_chunks_shuffle_u16")
    three = R.zstd_chunks("u8", 3)
    for name, v in u8.variants.items():
        w, t = u16.variants[name], three.variants[name]
        assert v.enc == w.enc == t.enc and v.status == w.status == t.status and v.mismatch == w.mismatch
        for x, y, z3 in zip(v.expect, w.expect, t.expect):
            if x is not None:
                assert y.view(np.uint8).tobytes() == x.reshape(2, -1).T.tobytes()
                assert z3.shape == (1, 1, R.ZN) and z3.tobytes() == x.tobytes()


def test_blosc_transitions():
    """c-blosc referees every frame (up to its cbytes); A's streams carry alias entries, B's none; lz4's
    block count goes 1, 4, 1."""
    import blosc_inner_streams as I
    for name in ("blosc_zstd", "blosc_lz4"):
        f = R.family(name)
        assert f.script == ["A", "B", "C", "A"]
        oc = O.OracleChain.from_metadata(f.codecs, "uint16", fill_bytes("uint16"), 1)
        for v in f.variants.values():
            for e, st, x in zip(v.enc, v.status, v.expect):
                cbytes = int.from_bytes(e[12:16], "little")  # c-blosc takes the frame alone: the slack is the plan's
                assert cbytes <= len(e) and not any(e[cbytes:])
                try:
                    got = oc.decode(e[:cbytes], f.chunk_shape)
                    assert st == R.OK and got.tobytes() == x.tobytes(), (name, v.name)
                except O.OracleError:
                    assert st == R.CORRUPT_STREAM, (name, v.name)
    cases = R.blosc_zstd_cases()
    assert all(c.alias_count()[0] >= 1 for c in cases["A"]) and all(c.alias_count() == (0, 0) for c in cases["B"])
    assert [c.status for c in cases["C"]] == [I.OK, I.OK, I.CORRUPT, I.OK]
    assert R.family("blosc_zstd").variants["C"].status == [0, 0, R.CORRUPT_STREAM, 0]
    lz = R.family("blosc_lz4")
    nblocks = {v: [-(-int.from_bytes(e[4:8], "little") // int.from_bytes(e[8:12], "little")) for e in lz.variants[v].enc] for v in "ABC"}
    assert nblocks == {"A": [1] * 4, "B": [4] * 4, "C": [1] * 4}
    for d in range(R.BL_K):  # every descriptor has slack after cbytes in all variants but its longest
        assert sum(len(v.enc[d]) > int.from_bytes(v.enc[d][12:16], "little") for v in lz.variants.values()) >= 2


def test_no_stage_is_numpy():
    t = R.family("no_stage_tiled")
    for v in t.variants.values():
        for d, e, x in zip(t.descs, v.enc, v.expect):
            if not d.null:
                assert np.array_equal(np.frombuffer(e, ">f4").reshape(64, 64, 64).transpose(2, 1, 0), x)
    r = R.family("no_stage_rows")
    for v in r.variants.values():
        for d, e, x in zip(r.descs, v.enc, v.expect):
            if not d.null:
                assert np.array_equal(_sel(np.frombuffer(e, "<f4").reshape(r.chunk_shape), d), x)
    for f in (t, r):
        assert sum(d.null for d in f.descs) == 1 and f.variants["A"].enc != f.variants["B"].enc
