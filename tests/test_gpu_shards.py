"""Every reader of a shard index in the library against the hand-built shards of tests/shard_model.py:
shards laid out as no writer of this project lays them out (inner chunks out of order, junk between them,
shared and overlapping ranges, an entry that points into the index), every kind of bad entry and bad
index, and partial reads past poisoned entries they do not touch.

  batch       CodecChain.decode_batch: k_shard_index + k_item_resolve one and two levels deep, the host
              walk of the general path below that; shard in host memory and in HBM; gzip inner chains
              with the direct-rows path on and off
  array       Array.retrieve_array_subset over a 2 x 2 grid of shards with one key missing
  wrapped / transposed / deeper   the same shards with crc32c + gzip after sharding_indexed, a transpose
              before it, and one more sharding level around it (the general path)
  plugin      decode_pinned_into
  cache       ArrayCached, which decodes whole shards
  store       store_array_subset into non-canonical old shards: parse_index and the carry-over

The model gives the status, the bytes, and what a read may look at: ZGPU_CTR_ENC_BYTES must equal the
sizes of the present entries the selection touches (an aliased range once per entry), ZGPU_CTR_ITEMS the
inner chunks it meets, and the output outside the selection keeps its sentinel bytes."""
import ctypes as C
import dataclasses
import struct
import zlib

import numpy as np
import pytest

import shard_model as S
import store_model as M
from scatter_cases import SENTINEL, TYPES, fill_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    return Context(0)


def chain_of(ctx, codecs, dt, validate=True):
    from zarrs_amd import CodecChain
    return CodecChain.from_metadata(codecs, dt, fill_bytes(dt), ctx, validate_checksums=validate)


def source(torch, enc, where):
    """what make_desc takes for the shard's bytes, and what keeps them alive"""
    if enc is None or where == "host":
        return enc, None
    t = torch.frombuffer(bytearray(enc if enc else b"\x00"), dtype=torch.uint8).cuda()
    return (t.data_ptr(), len(enc)), t  # (an empty shard: a valid address and length 0)


def raw_batch(ch, descs, out, out_shape, enc_device):
    """zgpu_decode_batch without the binding's raise: (rc, per-descriptor statuses, counters)"""
    from zarrs_amd import _lib as L
    n = len(descs)
    arr = (L.ChunkDesc * n)(*descs)
    st = (C.c_int32 * n)()
    flags = L.ENC_DEVICE if enc_device else 0
    rc = L.load().zgpu_decode_batch(ch._h, len(out_shape), arr, n, out.ctypes.data, L.u64s(out_shape), flags, st, None)
    ctr = (C.c_uint64 * L.N_COUNTERS)()
    L.load().zgpu_last_counters(ctr, L.N_COUNTERS)
    st = list(st)
    assert rc == next((s for s in st if s), 0)
    return st, {"enc_bytes": int(ctr[L.CTR_ENC_BYTES]), "items": int(ctr[L.CTR_ITEMS])}


def sentinel_array(shape, dt):
    return np.full(int(np.prod(shape)) * TYPES[dt][1], SENTINEL, np.uint8).view(S.np_dtype(dt)).reshape(shape)


def read(ch, torch, dt, shape, enc, sel, where, margin=1):
    """One descriptor decoded into the middle of a larger array of sentinel bytes: (status, the
    selection's box, counters). The bytes around the box must be sentinels still."""
    from zarrs_amd import make_desc
    nd = len(shape)
    start, sub = (list(sel[0]), list(sel[1])) if sel is not None else ([0] * nd, list(shape))
    pad = [1] * (nd - 1) + [margin]
    out_shape = [n + 2 * p for n, p in zip(sub, pad)]
    out = sentinel_array(out_shape, dt)
    src, keep = source(torch, enc, where)
    d = make_desc(src, list(shape), start, sub, out_start=pad)
    st, ctr = raw_batch(ch, [d], out, out_shape, where == "hbm")
    del keep
    box = tuple(slice(p, p + n) for p, n in zip(pad, sub))
    mask = np.ones(out_shape, bool)
    mask[box] = False
    assert (out.view(np.uint8).reshape(out_shape + [-1])[mask] == SENTINEL).all(), "bytes outside the selection"
    return st[0], out[box], ctr


def has_gzip(case):
    return "gzip" in S.leaf_chain(case.shard).b2b


# ---------------------------------------------------------------------------------------------------
# batch: every case, full and partial
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "hbm"])
@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_batch_reader(ctx, torch, case, where, monkeypatch):
    a, enc = case.built()
    ch = chain_of(ctx, case.codecs(), case.dtype, case.validate)
    es = TYPES[case.dtype][1]
    # gzip inner chains: the direct-rows path and the slot path, forced as test_gpu_gzip_direct.py forces
    # them. Only gaps_17_1_3_permuted_{start,end} can take direct rows (float32 inner chunks [2, 4]: rows of
    # 16 bytes, a power of two; plan_layout.cpp gzip_direct), and only with "1" and the 16-byte margin, for
    # the selections that cover whole inner chunks; the uint16 [2, 3] gzip cases have 6-byte rows and decode
    # through slots in all four variants. The library has no counter of direct items, so the path is forced,
    # not asserted. Other chains have one path.
    variants = [("1", 16 // es), ("1", 1), ("0", 16 // es), ("0", 1)] if has_gzip(case) else [(None, 1)]
    for direct, margin in variants:
        if direct is not None:
            monkeypatch.setenv("ZGPU_GZIP_DIRECT", direct)
        for sel in (None,) + case.sels:
            want, exp, stats = case.expect(sel)
            st, got, ctr = read(ch, torch, case.dtype, case.shape, enc, sel, where, margin)
            assert st == want, (sel, direct, margin)
            if want == 0:
                assert got.tobytes() == exp.tobytes(), (sel, direct, margin)
                if case.shard.depth() <= 2:  # the fused plan counts what it resolved
                    assert ctr == stats, (sel, direct, margin)


def test_five_index_checksums_are_refused(ctx, torch):
    """An index chain of five crc32c codecs: more than the index kernel takes. UNSUPPORTED when the
    chain or the plan is made, and nothing else."""
    from zarrs_amd import ZgpuError, make_desc
    from zarrs_amd import _lib as L
    case = S.Case("five", "index", "uint16", (4, 6), S.FIVE_CRCS)
    _, enc = case.built()
    assert case.expect()[0] == 0  # a legal shard
    with pytest.raises(ZgpuError) as e:
        ch = chain_of(ctx, case.codecs(), "uint16")
        ch.decode_batch([make_desc(enc, [4, 6])], np.zeros((4, 6), np.uint16), [4, 6], enc_device=False)
    assert e.value.status == L.UNSUPPORTED


# ---------------------------------------------------------------------------------------------------
# batches: one call, eight shards of one chain (canonical, permuted, aliased, gapped, missing, too short, out
# of bounds, corrupt index), each descriptor its own status
# ---------------------------------------------------------------------------------------------------
BATCH = ["reversed_bytes_crc", "alias_two", "gaps_1_3_17_end", None, "short", "wrapped_sum", "index_1crc_corrupt_0"]


@pytest.mark.parametrize("where", ["host", "hbm"])
def test_batch_of_good_and_bad_shards(ctx, torch, where):
    from zarrs_amd import make_desc
    short = S.Case("short", "batch", "uint16", (4, 6), S.Shard((2, 3), S.LE_CRC, cut=5))
    cases = [None if n is None else short if n == "short" else S.BY_NAME[n] for n in BATCH]
    codecs, dt, shape = cases[0].codecs(), "uint16", (4, 6)
    canon = S.Case("canonical", "batch", dt, shape, S.Shard((2, 3), S.LE_CRC))
    cases[0:0] = [canon]
    assert all(c is None or (c.codecs() == codecs and c.shape == shape) for c in cases)
    ch = chain_of(ctx, codecs, dt)
    for sel in (None, ((1, 2), (2, 2)), ((2, 0), (2, 6))):  # the last one misses the bad entry of wrapped_sum
        start, sub = sel if sel else ((0, 0), shape)
        out_shape = [len(cases) * sub[0], sub[1] + 2]
        out = sentinel_array(out_shape, dt)
        descs, keep, want = [], [], []
        for k, c in enumerate(cases):
            src, t = source(torch, c.built()[1] if c else None, where)
            keep.append(t)
            descs.append(make_desc(src, list(shape), list(start), list(sub), out_start=[k * sub[0], 1]))
            want.append(c.expect(sel) if c else S.read_shard(canon.shard, shape, dt, None, sel))
        st, _ = raw_batch(ch, descs, out, out_shape, where == "hbm")
        assert st == [w[0] for w in want], sel
        assert {0, S.SHARD_TOO_SMALL, S.INVALID_CHECKSUM} <= set(st) and (sel == ((2, 0), (2, 6)) or S.SHARD_INDEX_OOB in st)
        assert st[:5] == [0] * 5  # the canonical, permuted, aliased, gapped and missing shards decode
        for k, w in enumerate(want):
            if w[0] == 0:
                assert out[k * sub[0]:(k + 1) * sub[0], 1:-1].tobytes() == w[1].tobytes(), (sel, k)
        assert (np.ascontiguousarray(out[:, [0, -1]]).view(np.uint8) == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------
# array / cache: every case as shard (0, 1) of a 2 x 2 grid of shards, key (1, 0) missing
# ---------------------------------------------------------------------------------------------------
def refused(case, reader, call):
    """True when the table says `reader` refuses the case's chain by design: then `call` must answer
    UNSUPPORTED (when the chain is made or when it is used), and nothing else is asked of it."""
    from zarrs_amd import ZgpuError
    from zarrs_amd import _lib as L
    why = S.refusal(case, reader)
    if why is None:
        return False
    with pytest.raises(ZgpuError) as e:
        call()
    assert e.value.status == L.UNSUPPORTED, why
    return True


def grid_of(shards):
    """{grid index: Case} -> (the array with fill where a shard is missing, {key: bytes}); the shards share
    chain and shape, and the grid is 2 x 2 over the first two axes"""
    c0 = next(iter(shards.values()))
    sh = c0.shape
    nd = len(sh)
    full = np.empty([2 * sh[0], 2 * sh[1]] + list(sh[2:]), S.np_dtype(c0.dtype))
    full.reshape(-1).view(np.uint8)[:] = np.tile(np.frombuffer(fill_bytes(c0.dtype), np.uint8), full.size)
    store = {}
    for idx, c in shards.items():
        assert c.codecs() == c0.codecs() and c.shape == sh
        a, enc = c.built()
        idx = tuple(idx) + (0,) * (nd - len(idx))
        full[tuple(slice(i * s, (i + 1) * s) for i, s in zip(idx, sh))] = a
        store["c/" + "/".join(map(str, idx))] = enc
    return full, store


def open_array(ctx, case, full, store, where):
    from zarrs_amd import Array, DeviceStore, MemoryStore
    meta = {"shape": list(full.shape), "data_type": case.dtype, "fill_value": fill_bytes(case.dtype),
            "codecs": case.codecs(), "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": list(case.shape)}}}
    ms = MemoryStore(dict(store))
    return Array(DeviceStore.from_store(ms) if where == "hbm" else ms, meta, ctx, validate_checksums=case.validate)


def expect_subset(shards, start, sub, whole):
    """(status, array) of a read of the array's box by the model: shard by shard in grid order, the first
    failing shard's status. whole: every shard the box meets is decoded whole (the cache)."""
    c0 = next(iter(shards.values()))
    sh, nd = c0.shape, len(c0.shape)
    out = np.empty(sub, S.np_dtype(c0.dtype))
    out.reshape(-1).view(np.uint8)[:] = np.tile(np.frombuffer(fill_bytes(c0.dtype), np.uint8), out.size)
    status = 0
    for i in range(2):
        for j in range(2):
            org = [i * sh[0], j * sh[1]] + [0] * (nd - 2)
            lo = [max(o, a) for o, a in zip(org, start)]
            hi = [min(o + s, a + n) for o, s, a, n in zip(org, sh, start, sub)]
            c = shards.get((i, j))
            if any(l >= h for l, h in zip(lo, hi)) or c is None:
                continue
            sel = (tuple(l - o for l, o in zip(lo, org)), tuple(h - l for l, h in zip(lo, hi)))
            full = sel[1] == tuple(sh)
            st, v, _ = c.expect(None if whole or full else sel)
            if st:
                status = status or st
                continue
            if whole and not full:
                v = v[tuple(slice(a, a + n) for a, n in zip(*sel))]
            out[tuple(slice(l - a, h - a) for l, h, a in zip(lo, hi, start))] = v
    return status, out


@pytest.mark.parametrize("where", ["host", "hbm"])
@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_array_and_cache_readers(ctx, torch, case, where):
    """The case's shard at (0, 1) between two clean shards of the same chain. Through the array a subset
    looks only at the entries it touches; the cache decodes and keeps whole shards, so through it a subset
    fails whenever the full read of a shard it meets fails (shard_model.READERS)."""
    from zarrs_amd import ArrayCached, ChunkCacheDecodedLruSizeLimit, ZgpuError
    good = dataclasses.replace(case, shard=S.clean(case.shard))
    shards = {(0, 0): dataclasses.replace(good, seed=11), (0, 1): case, (1, 1): dataclasses.replace(good, seed=12)}
    full, store = grid_of(shards)
    if refused(case, "array", lambda: open_array(ctx, case, full, store, where).retrieve_array_subset()):
        assert S.refusal(case, "cache")
        return
    arr = open_array(ctx, case, full, store, where)
    s0, s1, rest = case.shape[0], case.shape[1], list(case.shape[2:])
    boxes_ = [([0] * len(case.shape), list(full.shape)), ([s0 - 1, s1 - 1] + [0] * len(rest), [2, 2] + rest),
              ([0, s1] + [0] * len(rest), list(case.shape))]
    boxes_ += [([sel[0][0], sel[0][1] + s1] + list(sel[0][2:]), list(sel[1])) for sel in case.sels]
    for reader in ("array", "cache"):
        for start, sub in boxes_:
            # a cache per read: a shard that decoded stays cached, which is not what is under test
            r = arr if reader == "array" else ArrayCached(arr, ChunkCacheDecodedLruSizeLimit(1 << 20, ctx))
            want, exp = expect_subset(shards, start, sub, whole=reader == "cache")
            if want:
                with pytest.raises(ZgpuError) as e:
                    r.retrieve_array_subset(start, sub)
                assert e.value.status == want, (reader, start, sub)
            else:
                assert r.retrieve_array_subset(start, sub).tobytes() == exp.tobytes(), (reader, start, sub)


# ---------------------------------------------------------------------------------------------------
# the general path: every case's shard under three more chains
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "hbm"])
@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_wrapped_reader(ctx, torch, case, where):
    """crc32c, then gzip, after sharding_indexed: the shard is decoded through them first"""
    _, enc = case.built()
    enc = enc + struct.pack("<I", S.crc32c(enc))
    z = zlib.compressobj(1, zlib.DEFLATED, 31)
    enc = z.compress(enc) + z.flush()
    codecs = case.codecs() + [{"name": "crc32c"}, {"name": "gzip", "configuration": {"level": 1}}]
    if refused(case, "wrapped", lambda: chain_of(ctx, codecs, case.dtype).decode(enc, list(case.shape))):
        return
    ch = chain_of(ctx, codecs, case.dtype, case.validate)
    for sel in (None,) + case.sels:
        want, exp, _ = case.expect(sel)
        st, got, _ = read(ch, torch, case.dtype, case.shape, enc, sel, where)
        assert st == want, sel
        assert want or got.tobytes() == exp.tobytes(), sel


@pytest.mark.parametrize("where", ["host", "hbm"])
@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_transposed_reader(ctx, torch, case, where):
    """A transpose before sharding_indexed: the shard holds the transposed array, and a selection is
    its box in the shard's frame (transpose_codec_partial.rs), so it touches the same entries."""
    _, enc = case.built()
    nd = len(case.shape)
    order = list(range(nd))[::-1] if nd < 3 else [1, 2, 0] + list(range(3, nd))
    inv = list(np.argsort(order))
    codecs = [{"name": "transpose", "configuration": {"order": order}}] + case.codecs()
    dec_shape = [case.shape[inv[d]] for d in range(nd)]  # encoded axis a runs along decoded axis order[a]
    if refused(case, "transposed", lambda: chain_of(ctx, codecs, case.dtype).decode(enc, dec_shape)):
        return
    ch = chain_of(ctx, codecs, case.dtype, case.validate)
    for sel in (None,) + case.sels:
        want, exp, _ = case.expect(sel)
        dsel = None if sel is None else ([sel[0][inv[d]] for d in range(nd)], [sel[1][inv[d]] for d in range(nd)])
        st, got, _ = read(ch, torch, case.dtype, dec_shape, enc, dsel, where)
        assert st == want, sel
        assert want or got.tobytes() == np.ascontiguousarray(np.transpose(exp, inv)).tobytes(), sel


@pytest.mark.parametrize("where", ["host", "hbm"])
@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_deeper_reader(ctx, torch, case, where):
    """One more sharding level around the shard (itself non-canonical: junk around its two inner chunks,
    the second one empty): a one-level case becomes the fused plan's two levels with a hand-built middle
    shard, a deeper case goes to the general path, which reads the outer indexes on the host."""
    a, _ = case.built()
    outer = S.Shard(tuple(case.shape), case.shard, location="start", endian="big", crcs=("start",),
                    layout=S.Layout(pre=3, post=1), empty=frozenset((1,)))
    shape = (2 * case.shape[0],) + tuple(case.shape[1:])
    a2 = np.concatenate([a, a]).copy()
    enc = S.encode(outer, a2, case.dtype)
    assert np.array_equal(a2[:case.shape[0]], a)
    if refused(case, "deeper", lambda: chain_of(ctx, outer.codecs(), case.dtype).decode(enc, list(shape))):
        return
    ch = chain_of(ctx, outer.codecs(), case.dtype, case.validate)
    sels = [None] + [s for s in case.sels] + [((case.shape[0] - 1,) + tuple(s[0][1:]), (2,) + tuple(s[1][1:])) for s in case.sels[:1]]
    for sel in sels:
        want, exp, _ = S.read_shard(outer, shape, case.dtype, enc, sel, case.validate)
        st, got, _ = read(ch, torch, case.dtype, shape, enc, sel, where)
        assert st == want, sel
        assert want or got.tobytes() == exp.tobytes(), sel


# ---------------------------------------------------------------------------------------------------
# plugin: zgpu_decode_pinned, full and partial
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_plugin_reader(ctx, torch, case):
    from zarrs_amd import ZgpuError, make_desc
    _, enc = case.built()
    nd = len(case.shape)
    full = (tuple([0] * nd), tuple(case.shape))
    if refused(case, "plugin", lambda: chain_of(ctx, case.codecs(), case.dtype).decode_pinned_into(
            [make_desc(enc, list(case.shape))], sentinel_array(list(case.shape), case.dtype), [0] * nd, list(case.shape))):
        return
    ch = chain_of(ctx, case.codecs(), case.dtype, case.validate)
    for sel in (None,) + case.sels:
        want, exp, _ = case.expect(sel)
        start, sub = sel or full
        view = sentinel_array([n + 3 for n in sub], case.dtype)
        d = make_desc(enc, list(case.shape), list(start), list(sub), out_start=[0] * nd)
        if want:
            with pytest.raises(ZgpuError) as e:
                ch.decode_pinned_into([d], view, [2] * nd, list(sub))
            assert e.value.status == want, sel
            continue
        assert ch.decode_pinned_into([d], view, [2] * nd, list(sub)) == [0]
        win = tuple(slice(2, 2 + n) for n in sub)
        assert view[win].tobytes() == exp.tobytes(), sel
        mask = np.ones(view.shape, bool)
        mask[win] = False
        assert (view.view(np.uint8).reshape(list(view.shape) + [-1])[mask] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------
# store: read-modify-write into non-canonical old shards
# ---------------------------------------------------------------------------------------------------
AS, SS, IS = (8, 12), (4, 6), (2, 3)
OLD_LAYOUTS = {
    "permuted": S.Layout(order=(2, 0, 3, 1)),
    "gapped": S.Layout(order=(3, 2, 1, 0), pre=1, gap=3, post=17),
    "aliased": S.Layout(alias=((2, 1), (3, 1)), pre=3, gap=1),
}
SUBSETS = [((1, 1), (1, 1)),    # inside inner chunk 0 of shard (0, 0): one decoded, the rest carried
           ((2, 3), (2, 3)),    # inner chunk 3 of shard (0, 0) covered: nothing decoded, three carried
           ((1, 2), (5, 8)),    # across all four shards, partly and wholly covered inner chunks
           ((6, 0), (2, 3)),    # an inner chunk of the missing shard (1, 0)
           ((0, 6), (4, 6))]    # shard (0, 1) covered: its old bytes are not read


class StoreRig:
    def __init__(self, ctx, torch, chain, location, layout, where, bad=None):
        self.torch, self.where, self.dt = torch, where, "uint16"
        mk = lambda seed, **kw: S.Case("old", "store", self.dt, SS, S.Shard(IS, chain, location=location, layout=layout, **kw),
                                       seed=seed)
        self.canon = S.Shard(IS, chain, location=location)
        shards = {(0, 0): mk(1, empty=frozenset()), (0, 1): mk(2), (1, 1): mk(3)}
        if bad:
            shards[(0, 1)] = mk(2, patch=((1, bad),))
        full, store = grid_of(shards)
        self.arr = open_array(ctx, shards[(0, 0)], full, store, where)
        self.model = M.StoreModel(AS, SS, S.np_dtype(self.dt), fill_bytes(self.dt), IS)
        self.model.fill_from(full)
        assert len(self.model.present) == 12

    def get(self, idx):
        v = self.arr.store.get(self.arr.chunk_key(idx))
        return None if v is None else (bytes(v.cpu().numpy()) if self.where == "hbm" else bytes(v))

    def snapshot(self):
        return {idx: self.get(idx) for idx in self.model.chunks() if self.get(idx) is not None}

    def give(self, data):
        return self.torch.from_numpy(data.view(np.int16)).cuda() if self.where == "hbm" else data


@pytest.mark.parametrize("where", ["host", "hbm"])
@pytest.mark.parametrize("location", ["start", "end"])
@pytest.mark.parametrize("layout", list(OLD_LAYOUTS))
@pytest.mark.parametrize("chain", [S.LE_CRC, S.GZ_CRC], ids=lambda c: c.name)
def test_store_into_hand_built_shards(ctx, torch, chain, layout, location, where):
    from zarrs_amd import _lib as L
    assert S.refusal(S.Case("x", "store", "uint16", SS, S.Shard(IS, chain)), "store") is None
    rig = StoreRig(ctx, torch, chain, location, OLD_LAYOUTS[layout], where)
    m = rig.model
    leaves = list(m.leaves())
    x = S.index_bytes(4, ("end",))
    for k, (start, shape) in enumerate(SUBSETS):
        data = np.random.default_rng(50 + k).integers(1, 60000, shape, dtype=np.uint16)
        before = rig.snapshot()
        cls = dict(M.classify_brute(m.array_shape, m.chunk_shape, m.leaf_shape, start, shape))
        r = m.store(list(start), data)
        done = rig.arr.store_array_subset(list(start), rig.give(data))
        ctr = L.last_counters()
        assert done == [(rig.arr.chunk_key(idx), L.STORE_SET) for idx in sorted(r["actions"])]
        assert (ctr["store_decoded"], ctr["store_encoded"], ctr["store_carried"]) == (r["decoded"], r["encoded"], r["carried"])
        after = rig.snapshot()
        assert set(after) == m.keys()
        for idx, new in after.items():
            if idx not in r["actions"]:
                assert new == before[idx], idx
                continue
            ent = S.entries_of(rig.canon, SS, new)  # the new shard, parsed by the model
            assert isinstance(ent, list) and [isinstance(e, bytes) for e in ent] == [(idx, j) in m.present for j in leaves]
            # present inner chunks back to back in C order, nothing else in the shard
            assert new == S.build_shard([e if isinstance(e, bytes) else None for e in ent], S.CANON, location,
                                        ("little", ("end",)))[0], idx
            lin = int(np.ravel_multi_index(idx, m.grid))
            if idx in before and M.UNTOUCHED in cls[lin]:
                old = S.entries_of(rig.canon, SS, before[idx])
                for j in range(4):
                    if cls[lin][j] == M.UNTOUCHED:  # carried over byte for byte, or absent as before
                        assert ent[j] == old[j], (idx, j)
            st, got, _ = S.read_shard(rig.canon, SS, rig.dt, new)
            assert st == 0 and got.tobytes() == np.ascontiguousarray(m.padded[m.chunk_box(idx)]).tobytes(), idx
    got = rig.arr.retrieve_array_subset()
    assert got.tobytes() == m.padded.tobytes()


BAD_OLD = {"half_sentinel_offset": lambda n, o, s: (S.MAX, s), "half_sentinel_size": lambda n, o, s: (o, S.MAX),
           "wrapped_sum": lambda n, o, s: (S.MAX - 1, 4), "past_end_by_one": lambda n, o, s: (n - s + 1, s)}


@pytest.mark.parametrize("where", ["host", "hbm"])
@pytest.mark.parametrize("bad", list(BAD_OLD))
def test_store_into_a_shard_with_a_bad_entry(ctx, torch, bad, where):
    """Entry 1 of old shard (0, 1) is out of bounds. A store that meets the shard without covering it
    fails for that shard alone with SHARD_INDEX_OOB, whichever inner chunk it touches, and the store is
    unchanged; a store that covers the shard never reads it."""
    from zarrs_amd import ZgpuError
    from zarrs_amd import _lib as L
    rig = StoreRig(ctx, torch, S.LE_CRC, "end", OLD_LAYOUTS["gapped"], where, bad=BAD_OLD[bad])
    before = rig.snapshot()
    data = np.random.default_rng(9).integers(1, 60000, (2, 8), dtype=np.uint16)
    start = [2, 2]  # rows 2..3, columns 2..9: inner chunks 2 and 3 of shards (0, 0) and (0, 1), never inner chunk 1
    ptrs, lens, keep = rig.arr._tables(start, list(data.shape), skip_covered=True)
    res = rig.arr.codecs.store_array_subset(list(AS), list(SS), ptrs, lens, start, rig.give(data), where == "hbm")
    ents = [(e[0], e[1], e[2]) for e in res.entries]
    res.release()
    assert res.rc == L.SHARD_INDEX_OOB and ents == [(0, L.STORE_SET, 0), (1, 0, L.SHARD_INDEX_OOB)]
    with pytest.raises(ZgpuError) as e:
        rig.arr.store_array_subset(start, rig.give(data))
    assert e.value.status == L.SHARD_INDEX_OOB and rig.snapshot() == before
    whole = np.random.default_rng(10).integers(1, 60000, SS, dtype=np.uint16)
    assert rig.arr.store_array_subset([0, 6], rig.give(whole)) == [(rig.arr.chunk_key((0, 1)), L.STORE_SET)]
    st, got, _ = S.read_shard(rig.canon, SS, rig.dt, rig.get((0, 1)))
    assert st == 0 and got.tobytes() == whole.tobytes()


def test_store_refuses_nested_shards(ctx, torch):
    from zarrs_amd import ZgpuError
    from zarrs_amd import _lib as L
    case = S.BY_NAME["nested2"]
    assert S.refusal(case, "store")
    full, store = grid_of({(0, 0): case})
    arr = open_array(ctx, case, full, store, "host")
    with pytest.raises(ZgpuError) as e:
        arr.store_array_subset([1, 1], np.ones((2, 2), np.uint16))
    assert e.value.status == L.UNSUPPORTED and dict(arr.store) == store
