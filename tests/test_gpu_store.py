"""Array.store_array_subset / store_chunk / erase_chunk on the GPU (zgpu_store_array_subset, store.cpp,
kernels/store.hip) against the numpy model of the rules (tests/store_model.py). After every store the
store's key set equals the model's, every chunk the call wrote is decoded by the CPU oracle (the numpy
value-codec model around it where the chain has a value codec or packbits) and equals the model bit for
bit, every other key holds the bytes it held, and the three store counters equal the model's counts. For
sharded arrays the old and new shard indexes are parsed on the host: untouched inner chunks keep their
presence and their encoded bytes, and the new shard is laid out in C order behind / in front of its index."""
import itertools
import struct

import numpy as np
import pytest

import oracle as O
import store_model as M
import value_codecs as V

pytestmark = pytest.mark.gpu

BYTES = {"name": "bytes", "configuration": {"endian": "little"}}
BYTES_BIG = {"name": "bytes", "configuration": {"endian": "big"}}
CRC = {"name": "crc32c"}
IDX = [BYTES, CRC]
GZIP = {"name": "gzip", "configuration": {"level": 1}}
ZSTD = {"name": "zstd", "configuration": {"level": 3}}
ZSTD_CK = {"name": "zstd", "configuration": {"level": 3, "checksum": True}}
BLOSC = {"name": "blosc", "configuration": {"cname": "lz4", "clevel": 5, "shuffle": "shuffle", "typesize": 4,
                                            "blocksize": 0}}
FSO = {"name": V.FSO, "configuration": {"offset": 0, "scale": 10, "dtype": "f4", "astype": "i2"}}
PACKBITS = {"name": "packbits", "configuration": {"padding_encoding": "none"}}


def tr(order):
    return {"name": "transpose", "configuration": {"order": order}}


def sh(inner_shape, inner, location="end"):
    return {"name": "sharding_indexed", "configuration": {"chunk_shape": inner_shape, "codecs": inner,
                                                          "index_codecs": IDX, "index_location": location}}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    return Context(0)


def random_data(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "b":
        return rng.integers(0, 2, shape, dtype=np.uint8).astype(np.bool_)
    if dt.kind in "ui":
        return rng.integers(1, np.iinfo(dt).max, shape, dtype=dt)
    if dt.kind == "c":
        return (rng.standard_normal(shape) * 100 + 1j * rng.standard_normal(shape)).astype(dt)
    return (rng.standard_normal(shape) * 100).astype(dt)


def to_device(torch, a):
    """a torch device tensor of a's shape and element size (uint16 travels as int16: same bytes)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


class Rig:
    """One array, its store, its model and its CPU decoder."""

    def __init__(self, ctx, torch, codecs, data_type, fill, array_shape, chunk_shape, device, seeded, leaf_shape=None,
                 seed=1, holes=()):
        from zarrs_amd import Array, DeviceStore, MemoryStore, fill_value_bytes
        self.torch, self.device = torch, device
        self.nd = len(array_shape)
        self.meta = {"shape": array_shape, "data_type": data_type, "fill_value": fill, "codecs": codecs,
                     "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": chunk_shape}}}
        fb = fill_value_bytes(data_type, fill)
        modelled = any(c["name"] in (V.FSO, "packbits") for c in codecs)
        self.mc = V.ModelChain(codecs, data_type, fill, self.nd) if modelled else \
            O.OracleChain.from_metadata(codecs, data_type, fb, self.nd)
        self.dtype = np.dtype(V.NP[data_type])
        lossy = any(c["name"] == V.FSO for c in codecs)
        rt = (lambda a: self.mc.decode(self.mc.encode(a), list(a.shape))) if lossy else None
        missing = self.mc.decoded_fill([1])[0] if lossy else None
        self.model = M.StoreModel(array_shape, chunk_shape, self.dtype, fb, leaf_shape, rt, missing)
        self.store = DeviceStore() if device else MemoryStore()
        self.arr = Array(self.store, self.meta, ctx)
        if seeded:
            raw = random_data(self.dtype, self.model.padded.shape, seed)
            for box in holes:  # regions of fill value (absent inner chunks of a seeded shard)
                raw[box] = np.frombuffer(fb, self.dtype)[0]
            self.model.fill_from(raw)
            for idx in self.model.chunks():
                if idx in self.model.keys():
                    self.put(idx, self.mc.encode(raw[self.model.chunk_box(idx)]))

    def key(self, idx):
        return self.arr.chunk_key(idx)

    def put(self, idx, enc):
        enc = bytes(enc)
        self.store.set(self.key(idx), self.torch.frombuffer(bytearray(enc), dtype=self.torch.uint8).cuda()
                       if self.device else enc)

    def get(self, idx):
        v = self.store.get(self.key(idx))
        return None if v is None else (bytes(v.cpu().numpy()) if self.device else bytes(v))

    def snapshot(self):
        return {idx: self.get(idx) for idx in self.model.chunks() if self.key(idx) in self.store}

    def give(self, data):
        return to_device(self.torch, data) if self.device else data

    def apply(self, start, data, store_empty_chunks=False):
        """one store through the library and through the model, and every check that needs no index"""
        from zarrs_amd import _lib as L
        before = self.snapshot()
        r = self.model.store(start, data, store_empty_chunks)
        done = self.arr.store_array_subset(start, self.give(data), store_empty_chunks)
        ctr = L.last_counters()
        want = [(self.key(idx), L.STORE_SET if a == "set" else L.STORE_ERASE) for idx, a in sorted(r["actions"].items())]
        assert done == want, (start, list(data.shape))
        after = self.snapshot()
        assert set(after) == self.model.keys(), (start, list(data.shape))
        for idx, enc in after.items():
            if idx in r["actions"]:
                got = self.mc.decode(enc, self.model.chunk_shape)
                assert got.tobytes() == np.ascontiguousarray(self.model.padded[self.model.chunk_box(idx)]).tobytes(), \
                    (start, list(data.shape), idx)
            else:
                assert enc == before[idx], idx
        assert (ctr["store_decoded"], ctr["store_encoded"], ctr["store_carried"]) == \
            (r["decoded"], r["encoded"], r["carried"]), (start, list(data.shape))
        return r, before, after

    def read_back(self):
        """the whole array through the library's read path equals the model"""
        got = self.arr.retrieve_array_subset()
        want = self.model.padded[tuple(slice(0, s) for s in self.model.array_shape)]
        assert got.tobytes() == np.ascontiguousarray(want).tobytes()


# ---------------------------------------------------------------------------------------------------
# unsharded
# ---------------------------------------------------------------------------------------------------
A3, C3 = [20, 33, 40], [8, 16, 16]
SUBSETS3 = [([0, 0, 0], [20, 33, 40]), ([8, 16, 16], [8, 16, 16]), ([3, 5, 7], [11, 20, 22]), ([0, 0, 0], [20, 33, 17]),
            ([19, 32, 39], [1, 1, 1]), ([0, 0, 1], [20, 33, 3])]
# a rotating pairing of chain and data type (every element size 1, 2, 4, 8, 16; every chain once or twice)
CASES = [
    ("bytes", [BYTES], "uint8", 0),
    ("big_crc", [BYTES_BIG, CRC], "uint16", 0),
    ("tr_gzip", [tr([2, 0, 1]), BYTES, GZIP], "float64", 0.0),
    ("zstd_ck", [BYTES, ZSTD_CK], "complex128", [0.0, 0.0]),
    ("blosc", [BYTES, BLOSC], "float32", 0.0),
    ("fso_zstd", [FSO, BYTES, ZSTD], "float32", 0.0),
    ("packbits", [PACKBITS], "bool", False),
    ("bytes16", [BYTES], "complex128", [1.5, -2.0]),
    ("big_crc8", [BYTES_BIG, CRC], "float64", 7.25),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_unsharded_subsets(ctx, torch_cuda, case, device):
    from zarrs_amd import ZgpuError
    from zarrs_amd import _lib as L
    _, codecs, dt, fill = case
    for seeded in (False, True):
        rig = Rig(ctx, torch_cuda, codecs, dt, fill, A3, C3, device, seeded)
        for k, (start, shape) in enumerate(SUBSETS3):
            if start == C3:  # one covered chunk: its old bytes are garbage and are never read
                rig.put((1, 1, 1), b"\x01\x02garbage that no codec decodes")
            r, _, _ = rig.apply(start, random_data(rig.dtype, shape, 100 + k))
            assert r["actions"]
        rig.read_back()
        # zero volume: nothing happens; out of bounds: refused, by the binding and by the library
        before = rig.snapshot()
        assert rig.arr.store_array_subset([3, 3, 3], rig.give(random_data(rig.dtype, [2, 0, 5], 0))) == []
        for start, shape in (([13, 0, 0], [8, 1, 1]), ([0, 0, 40], [1, 1, 1])):
            data = rig.give(random_data(rig.dtype, shape, 0))
            with pytest.raises(ZgpuError) as e:
                rig.arr.store_array_subset(start, data)
            assert e.value.status == L.INVALID_ARGUMENT
            ptrs, lens, keep = rig.arr._tables([0, 0, 0], [1, 1, 1])
            with pytest.raises(ZgpuError) as e:
                rig.arr.codecs.store_array_subset(A3, C3, ptrs, lens, start, data, device)
            assert e.value.status == L.INVALID_ARGUMENT
        assert rig.snapshot() == before


GEOMETRIES = [
    ("1d_u16", [BYTES_BIG, CRC], "uint16", 0, [4099], [256], ([255], [3585])),
    ("1d_c16", [BYTES], "complex128", [0.0, 0.0], [4099], [256], ([255], [3585])),
    ("1d_bool", [PACKBITS], "bool", False, [4099], [256], ([255], [3585])),
    ("4d_f32", [tr([3, 1, 0, 2]), BYTES, ZSTD], "float32", 0.0, [5, 6, 7, 9], [2, 3, 4, 4], ([1, 1, 1, 1], [3, 4, 5, 7])),
    ("4d_u8", [BYTES, GZIP], "uint8", 0, [5, 6, 7, 9], [2, 3, 4, 4], ([1, 1, 1, 1], [3, 4, 5, 7])),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_other_ranks(ctx, torch_cuda, geo, device):
    _, codecs, dt, fill, array_shape, chunk_shape, (start, shape) = geo
    for seeded in (False, True):
        rig = Rig(ctx, torch_cuda, codecs, dt, fill, array_shape, chunk_shape, device, seeded)
        rig.apply(start, random_data(rig.dtype, shape, 5))
        rig.apply([0] * len(array_shape), random_data(rig.dtype, array_shape, 6))
        rig.apply(start, random_data(rig.dtype, shape, 7))
        rig.read_back()


def test_store_chunk_and_erase_chunk(ctx, torch_cuda):
    from zarrs_amd import ZgpuError
    from zarrs_amd import _lib as L
    rig = Rig(ctx, torch_cuda, [BYTES, ZSTD], "float32", 0.0, A3, C3, False, True)
    new = random_data(rig.dtype, [4, 16, 8], 3)  # the edge chunk (2, 1, 2): the part inside the array
    assert rig.arr.store_chunk((2, 1, 2), new) == [(rig.key((2, 1, 2)), L.STORE_SET)]
    assert rig.arr.retrieve_chunk((2, 1, 2)).tobytes() == new.tobytes()
    with pytest.raises(ZgpuError):
        rig.arr.store_chunk((2, 1, 2), np.zeros([8, 16, 16], np.float32))
    rig.arr.erase_chunk((2, 1, 2))
    rig.arr.erase_chunk((2, 1, 2))
    assert rig.key((2, 1, 2)) not in rig.store and not rig.arr.retrieve_chunk((2, 1, 2)).any()


def test_filesystem_store(ctx, torch_cuda, tmp_path):
    from zarrs_amd import Array, FilesystemStore
    rig = Rig(ctx, torch_cuda, [BYTES, GZIP], "uint16", 0, A3, C3, False, False)
    arr = Array(FilesystemStore(tmp_path), rig.meta, ctx)
    a = random_data(rig.dtype, A3, 1)
    arr.store_array_subset([0, 0, 0], a)
    b = random_data(rig.dtype, [11, 20, 22], 2)
    arr.store_array_subset([3, 5, 7], b)
    a[3:14, 5:25, 7:29] = b
    assert arr.retrieve_array_subset().tobytes() == a.tobytes()
    arr.store_array_subset([8, 16, 16], np.zeros(C3, np.uint16))
    assert arr.store.get(arr.chunk_key((1, 1, 1))) is None


# ---------------------------------------------------------------------------------------------------
# erasure (rule 3)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("store_empty", [False, True], ids=["erase", "store_empty"])
def test_fill_chunks_are_erased_or_stored(ctx, torch_cuda, store_empty, device):
    want = "set" if store_empty else "erase"
    for dt, fill in (("float32", 2.5), ("complex128", [0.0, 0.0]), ("uint8", 9)):
        rig = Rig(ctx, torch_cuda, [BYTES, CRC], dt, fill, A3, C3, device, False)
        fv = np.frombuffer(rig.model.fill_bytes, rig.dtype)[0]
        rig.apply(C3, random_data(rig.dtype, C3, 1))  # chunk (1, 1, 1) present
        r, _, _ = rig.apply(C3, np.full(C3, fv, rig.dtype), store_empty)  # fill over a present covered chunk
        assert r["actions"] == {(1, 1, 1): want}
        part = random_data(rig.dtype, [2, 3, 5], 2)
        rig.apply([9, 17, 18], part)  # a partly fill chunk ...
        r, _, _ = rig.apply([9, 17, 18], np.full([2, 3, 5], fv, rig.dtype), store_empty)  # ... loses its non-fill part
        assert r["actions"] == {(1, 1, 1): want}
        rig.arr.erase_chunk((1, 1, 1))
        rig.model.present.discard(((1, 1, 1), (0, 0, 0)))
        r, _, after = rig.apply([9, 17, 18], np.full([2, 3, 5], fv, rig.dtype), store_empty)  # fill into a missing chunk
        assert r["actions"] == {(1, 1, 1): want} and ((1, 1, 1) in after) == store_empty


def test_fill_comparison_is_bytewise(ctx, torch_cuda):
    # a NaN fill value with a payload: the same NaN is fill, another NaN is data
    rig = Rig(ctx, torch_cuda, [BYTES], "float32", "0x7fc00001", A3, C3, False, False)
    same = np.frombuffer(np.full(int(np.prod(C3)), 0x7FC00001, "<u4").tobytes(), "<f4").reshape(C3)
    other = np.frombuffer(np.full(int(np.prod(C3)), 0x7FC00000, "<u4").tobytes(), "<f4").reshape(C3)
    r, _, _ = rig.apply(C3, same)
    assert r["actions"] == {(1, 1, 1): "erase"}
    r, _, after = rig.apply(C3, other)
    assert r["actions"] == {(1, 1, 1): "set"} and after[(1, 1, 1)] == other.tobytes()
    # +0.0 fill: -0.0 is data
    rig = Rig(ctx, torch_cuda, [BYTES], "float32", 0.0, A3, C3, False, False)
    r, _, _ = rig.apply(C3, np.zeros(C3, np.float32))
    assert r["actions"] == {(1, 1, 1): "erase"}
    r, _, after = rig.apply(C3, np.full(C3, -0.0, np.float32))
    assert r["actions"] == {(1, 1, 1): "set"} and after[(1, 1, 1)] == np.full(C3, -0.0, np.float32).tobytes()


# ---------------------------------------------------------------------------------------------------
# a sequence of stores on one store
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
def test_sequence_of_random_subsets(ctx, torch_cuda, device):
    rng = np.random.default_rng(42)
    for codecs, dt, fill, sharded in (([tr([1, 2, 0]), BYTES, ZSTD], "float32", 0.0, False),
                                      ([sh([4, 8, 8], [BYTES, GZIP, CRC])], "uint16", 0, True)):
        rig = Rig(ctx, torch_cuda, codecs, dt, fill, A3, C3, device, True, leaf_shape=[4, 8, 8] if sharded else None)
        for k in range(8):
            start = [int(rng.integers(0, a)) for a in A3]
            shape = [int(rng.integers(1, a - s + 1)) for a, s in zip(A3, start)]
            data = random_data(rig.dtype, shape, 200 + k)
            if k % 3 == 2:  # every third store writes fill value: chunks and inner chunks disappear
                data[...] = np.frombuffer(rig.model.fill_bytes, rig.dtype)[0]
            rig.apply(start, data)
        rig.read_back()


# ---------------------------------------------------------------------------------------------------
# sharded
# ---------------------------------------------------------------------------------------------------
AS, SS, IS = [24, 40], [16, 16], [4, 8]
N_INNER = 8
SUBSETS2 = [([0, 0], [24, 40]), ([16, 16], [8, 16]), ([0, 0], [16, 16]), ([3, 5], [11, 20]), ([0, 0], [24, 17]),
            ([23, 39], [1, 1]), ([0, 1], [24, 3]), ([5, 9], [2, 3]), ([4, 8], [4, 8])]
INNER = [("bytes", [BYTES]), ("crc", [BYTES, CRC]), ("zstd", [BYTES, ZSTD]), ("tr_gzip", [tr([1, 0]), BYTES, GZIP])]
HOLES = [(slice(0, 4), slice(8, 16)), (slice(20, 24), slice(32, 40)), (slice(16, 32), slice(16, 32))]


def parse_index(shard, n_inner, at_start):
    """[(offset, nbytes) or None] per inner chunk; the index crc32c is checked"""
    x = n_inner * 16 + 4
    raw = shard[:x] if at_start else shard[-x:]
    assert struct.unpack("<I", raw[-4:])[0] == O.crc32c(raw[:-4])
    v = struct.unpack("<%dQ" % (2 * n_inner), raw[:-4])
    return [None if v[2 * k] == v[2 * k + 1] == 2 ** 64 - 1 else (v[2 * k], v[2 * k + 1]) for k in range(n_inner)]


def check_shards(rig, r, before, after, start, shape, at_start, n_inner=N_INNER):
    """the index-level rules for every shard the store met"""
    m = rig.model
    cls = dict(M.classify_brute(m.array_shape, m.chunk_shape, m.leaf_shape, start, shape))
    leaves = list(m.leaves())
    for idx in r["actions"]:
        lin = int(np.ravel_multi_index(idx, m.grid))
        new = parse_index(after[idx], n_inner, at_start) if idx in after else [None] * n_inner
        old = [None] * n_inner  # (a wholly covered shard's old bytes may be garbage: not parsed)
        if idx in before and M.UNTOUCHED in cls[lin]:
            old = parse_index(before[idx], n_inner, at_start)
        assert [e is not None for e in new] == [(idx, j) in m.present for j in leaves], idx
        pos = n_inner * 16 + 4 if at_start else 0  # present inner chunks back to back in C order
        for k, e in enumerate(new):
            if e is not None:
                assert e[0] == pos, (idx, k)
                pos += e[1]
            if cls[lin][k] == M.UNTOUCHED:  # as before, byte for byte
                assert (e is None) == (old[k] is None), (idx, k)
                if e is not None:
                    assert after[idx][e[0]:e[0] + e[1]] == before[idx][old[k][0]:old[k][0] + old[k][1]], (idx, k)
        if idx in after:
            assert len(after[idx]) == pos + (0 if at_start else n_inner * 16 + 4)


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("location", ["start", "end"])
@pytest.mark.parametrize("inner", INNER, ids=[i[0] for i in INNER])
def test_sharded_subsets(ctx, torch_cuda, inner, location, device):
    dt, fill = ("float32", 0.0) if inner[0] in ("bytes", "zstd") else ("uint16", 3)
    for seeded in (False, True):
        rig = Rig(ctx, torch_cuda, [sh(IS, inner[1], location)], dt, fill, AS, SS, device, seeded, leaf_shape=IS,
                  holes=HOLES)
        if seeded:  # the seeded store has absent inner chunks and no key for the all-fill shard (1, 1)
            assert (1, 1) not in rig.snapshot() and ((0, 0), (0, 1)) not in rig.model.present
        for k, (start, shape) in enumerate(SUBSETS2):
            if start == [0, 0] and shape == SS:  # a wholly covered shard: its old bytes are garbage, never read
                rig.put((0, 0), b"\xff" * 40)
            r, before, after = rig.apply(start, random_data(rig.dtype, shape, 300 + k))
            check_shards(rig, r, before, after, start, shape, location == "start")
        # fill value over the part of shard (0, 0) that holds data: the inner chunks go, then the shard
        fv = np.frombuffer(rig.model.fill_bytes, rig.dtype)[0]
        r, before, after = rig.apply([0, 0], np.full([8, 16], fv, rig.dtype))
        check_shards(rig, r, before, after, [0, 0], [8, 16], location == "start")
        assert r["actions"] == {(0, 0): "set"}
        r, before, after = rig.apply([6, 0], np.full([10, 16], fv, rig.dtype), store_empty_chunks=True)
        check_shards(rig, r, before, after, [6, 0], [10, 16], location == "start")
        assert r["actions"] == {(0, 0): "erase"} and (0, 0) not in after
        rig.read_back()


def test_one_inner_chunk_of_sixteen(ctx, torch_cuda):
    from zarrs_amd import _lib as L
    rig = Rig(ctx, torch_cuda, [sh(IS, [BYTES, ZSTD])], "float32", 0.0, [16, 32], [16, 32], False, True, leaf_shape=IS)
    r, before, after = rig.apply([5, 9], random_data(rig.dtype, [2, 3], 1))  # inside inner chunk (1, 1)
    check_shards(rig, r, before, after, [5, 9], [2, 3], False, 16)
    ctr = L.last_counters()
    assert ctr["store_decoded"] == 1 and ctr["store_encoded"] == 1 and ctr["store_carried"] == 15
    r, before, after = rig.apply([4, 8], random_data(rig.dtype, IS, 2))  # the whole inner chunk: nothing decoded
    ctr = L.last_counters()
    assert ctr["store_decoded"] == 0 and ctr["store_encoded"] == 1 and ctr["store_carried"] == 15


def _error_rig(ctx, torch_cuda, device=False):
    return Rig(ctx, torch_cuda, [sh(IS, [BYTES, CRC])], "uint16", 0, AS, SS, device, True, leaf_shape=IS)


def _raw_store(rig, start, data):
    """the chain-level call: the entries with their statuses, nothing applied"""
    ptrs, lens, keep = rig.arr._tables(start, list(data.shape), skip_covered=True)
    res = rig.arr.codecs.store_array_subset(AS, SS, ptrs, lens, start, rig.give(data), rig.device)
    ents = list(res.entries)
    res.release()
    return res.rc, ents


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
def test_sharded_corruption_and_carry_over(ctx, torch_cuda, device):
    from zarrs_amd import ZgpuError
    from zarrs_amd import _lib as L
    rig = _error_rig(ctx, torch_cuda, device)
    good = rig.get((0, 0))
    idx = parse_index(good, N_INNER, False)
    off, n = idx[3]  # inner chunk (1, 1): rows 4..8, columns 8..16
    bad = bytearray(good)
    bad[off + 5] ^= 0x40
    rig.put((0, 0), bad)
    # untouched: the store succeeds and carries the corrupt bytes
    data = random_data(rig.dtype, [2, 3], 1)
    rig.model.store([1, 1], data)
    done = rig.arr.store_array_subset([1, 1], rig.give(data))
    assert done == [(rig.key((0, 0)), L.STORE_SET)]
    new = rig.get((0, 0))
    o2, n2 = parse_index(new, N_INNER, False)[3]
    assert n2 == n and new[o2:o2 + n2] == bytes(bad[off:off + n])
    # partly covered: its entry fails alone, ZgpuError is raised and the store is unchanged
    before = rig.snapshot()
    data = random_data(rig.dtype, [4, 20], 2)  # rows 5..9, columns 9..29: shards (0, 0) and (0, 1)
    rc, ents = _raw_store(rig, [5, 9], data)
    assert rc == L.INVALID_CHECKSUM
    assert [(e[0], e[1], e[2]) for e in ents] == [(0, 0, L.INVALID_CHECKSUM), (1, L.STORE_SET, 0)]
    with pytest.raises(ZgpuError) as e:
        rig.arr.store_array_subset([5, 9], rig.give(data))
    assert e.value.status == L.INVALID_CHECKSUM and rig.snapshot() == before
    # wholly covered: the corrupt inner chunk is replaced without being read
    rig.put((0, 0), new)
    data = random_data(rig.dtype, IS, 3)
    rig.model.store([4, 8], data)
    assert rig.arr.store_array_subset([4, 8], rig.give(data)) == [(rig.key((0, 0)), L.STORE_SET)]
    sh_chain = O.OracleChain.from_metadata(rig.meta["codecs"], "uint16", rig.model.fill_bytes, 2)
    assert sh_chain.decode(rig.get((0, 0)), SS).tobytes() == \
        np.ascontiguousarray(rig.model.padded[rig.model.chunk_box((0, 0))]).tobytes()


def test_sharded_bad_old_index(ctx, torch_cuda):
    from zarrs_amd import ZgpuError
    from zarrs_amd import _lib as L
    rig = _error_rig(ctx, torch_cuda)
    good = rig.get((0, 0))
    x = N_INNER * 16 + 4
    data = random_data(rig.dtype, [2, 3], 1)
    # a flipped byte in the index
    bad = bytearray(good)
    bad[len(good) - x + 9] ^= 1
    rig.put((0, 0), bad)
    before = rig.snapshot()
    with pytest.raises(ZgpuError) as e:
        rig.arr.store_array_subset([1, 1], data)
    assert e.value.status == L.INVALID_CHECKSUM and rig.snapshot() == before
    # the entry of an untouched inner chunk points past the shard; the crc32c matches, so the range check fires
    entries = list(struct.unpack("<%dQ" % (2 * N_INNER), good[-x:-4]))
    entries[2 * 7] = len(good) - 3  # inner chunk (3, 1): offset + nbytes beyond the shard
    raw = struct.pack("<%dQ" % (2 * N_INNER), *entries)
    rig.put((0, 0), good[:-x] + raw + struct.pack("<I", O.crc32c(raw)))
    before = rig.snapshot()
    rc, ents = _raw_store(rig, [1, 1], data)
    assert rc == L.SHARD_INDEX_OOB and [(e[0], e[1], e[2]) for e in ents] == [(0, 0, L.SHARD_INDEX_OOB)]
    with pytest.raises(ZgpuError) as e:
        rig.arr.store_array_subset([1, 1], data)
    assert e.value.status == L.SHARD_INDEX_OOB and rig.snapshot() == before
    # a shard too short for its index
    rig.put((0, 0), good[-20:])
    with pytest.raises(ZgpuError) as e:
        rig.arr.store_array_subset([1, 1], data)
    assert e.value.status == L.SHARD_TOO_SMALL
    # the same shard wholly covered: never read
    whole = random_data(rig.dtype, SS, 4)
    assert rig.arr.store_array_subset([0, 0], whole) == [(rig.key((0, 0)), L.STORE_SET)]
    assert rig.arr.retrieve_chunk((0, 0)).tobytes() == whole.tobytes()


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codecs,chunk", [
    ([BYTES, {"name": "numcodecs.bz2", "configuration": {"level": 1}}], [8, 16, 16]),
    ([sh([4, 8, 8], [BYTES]), GZIP], [8, 16, 16]),
    ([tr([2, 1, 0]), sh([4, 8, 8], [BYTES])], [8, 16, 16]),
    ([sh([4, 8, 8], [sh([2, 4, 4], [BYTES])])], [8, 16, 16]),
], ids=["bz2", "gzip_after_sharding", "transpose_before_sharding", "nested_sharding"])
def test_refused_chains(ctx, torch_cuda, codecs, chunk):
    from zarrs_amd import Array, MemoryStore, ZgpuError
    from zarrs_amd import _lib as L
    meta = {"shape": A3, "data_type": "uint8", "fill_value": 0, "codecs": codecs,
            "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": chunk}}}
    arr = Array(MemoryStore(), meta, ctx)
    with pytest.raises(ZgpuError) as e:
        arr.store_array_subset([0, 0, 0], np.ones(A3, np.uint8))
    assert e.value.status == L.UNSUPPORTED and not arr.store


def test_non_regular_grid_is_refused_at_open(ctx):
    from zarrs_amd import Array, MemoryStore, ZgpuError
    from zarrs_amd import _lib as L
    meta = {"shape": A3, "data_type": "uint8", "fill_value": 0, "codecs": [BYTES],
            "chunk_grid": {"name": "rectangular", "configuration": {"chunk_shape": [[8, 12], 16, 16]}}}
    with pytest.raises(ZgpuError) as e:
        Array(MemoryStore(), meta, ctx)
    assert e.value.status == L.UNSUPPORTED
