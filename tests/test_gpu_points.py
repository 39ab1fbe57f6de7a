"""Array.retrieve_elements / ArrayCached.retrieve_elements on the GPU (zgpu_retrieve_elements,
zgpu_cache_retrieve_elements: zarrs_amd/csrc/points.cpp, kernels/points.hip) against numpy fancy indexing on
the source array. The encoded chunks come from the CPU oracle (the numpy value-codec model for the
fixedscaleoffset chain). Every chain, element size and point count runs through host and device indices,
host and device outputs, and host- and device-resident stores."""
import itertools

import numpy as np
import pytest

import oracle as O
import value_codecs as V

pytestmark = pytest.mark.gpu

BYTES = {"name": "bytes", "configuration": {"endian": "little"}}
BYTES_BIG = {"name": "bytes", "configuration": {"endian": "big"}}
CRC = {"name": "crc32c"}
GZIP = {"name": "gzip", "configuration": {"level": 1}}
# data on a grid of 1/4: the codec's int16 round trip is exact, so the source array is the expected value
FSO = {"name": V.FSO, "configuration": {"offset": 0, "scale": 4, "dtype": "f4", "astype": "i2"}}


def tr(order):
    return {"name": "transpose", "configuration": {"order": order}}


def sh(inner_shape, inner, location="end"):
    return {"name": "sharding_indexed", "configuration": {"chunk_shape": inner_shape, "codecs": inner,
                                                          "index_codecs": [BYTES, CRC], "index_location": location}}


# name -> (codecs, data type, array shape, chunk shape, leaf shape, boxes of fill value)
CHAINS = {
    "bytes": ([BYTES], "float32", [20, 33, 40], [8, 16, 16], [8, 16, 16], ()),
    "transpose_big_gzip_crc": ([tr([2, 0, 1]), BYTES_BIG, GZIP, CRC], "float32", [20, 33, 40], [8, 16, 16],
                               [8, 16, 16], ()),
    "sharded_2d": ([sh([4, 8], [BYTES, CRC])], "uint16", [24, 40], [16, 16], [4, 8], ()),
    # the C3-style chain of test_gpu_plugin_paths.py: one inner chunk equal to the fill value, omitted
    "c3": ([sh([8, 8, 8], [BYTES, GZIP, CRC])], "float32", [32, 32, 32], [32, 32, 32], [8, 8, 8],
           ((slice(8, 16), slice(0, 8), slice(16, 24)),)),
    # the inner chunk [4, 8] of the transposed frame is the leaf [8, 4] of the chunk's frame
    "transpose_sharded": ([tr([1, 0]), sh([4, 8], [BYTES, CRC], "start")], "float32", [24, 40], [16, 16], [8, 4], ()),
    # order [2, 0, 1] is not its own inverse: the inner chunk [8, 4, 4] of the transposed frame [16, 8, 16] is
    # the leaf [4, 4, 8] of the chunk's frame (the inverse permutation would make it [4, 8, 4], and the
    # items planned would no longer be the leaves counted here)
    "transpose3_sharded": ([tr([2, 0, 1]), sh([8, 4, 4], [BYTES_BIG, GZIP, CRC])], "float32", [20, 33, 40],
                           [8, 16, 16], [4, 4, 8], ()),
    "fixedscaleoffset": ([FSO, BYTES], "float32", [20, 33, 40], [8, 16, 16], [8, 16, 16], ()),
}
DTYPES = ["uint8", "uint16", "float32", "float64", "complex128"]  # element sizes 1, 2, 4, 8, 16
COUNTS = [0, 1, 63, 64, 65, 257, 3000]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    c = Context(0)
    yield c
    c.close()


def source(data_type, shape, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(V.NP[data_type])
    if dt.kind in "ui":
        return rng.integers(1, np.iinfo(dt).max, shape, dtype=dt)
    if dt.kind == "c":
        return (rng.standard_normal(shape) * 100 + 1j * rng.standard_normal(shape)).astype(dt)
    return (np.round(rng.standard_normal(shape) * 32) / 4 + 0.0).astype(dt)  # on a grid of 1/4, no negative zero


class Rig:
    """One array: its source values, its encoded chunks in a MemoryStore and in a DeviceStore."""

    def __init__(self, ctx, codecs, data_type, array_shape, chunk_shape, fill=0, seed=1, missing=(), holes=()):
        from zarrs_amd import Array, DeviceStore, MemoryStore, fill_value_bytes
        self.shape, self.chunk_shape, self.nd = array_shape, chunk_shape, len(array_shape)
        self.meta = {"shape": array_shape, "data_type": data_type, "fill_value": fill, "codecs": codecs,
                     "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": chunk_shape}}}
        fb = fill_value_bytes(data_type, fill)
        self.dtype = np.dtype(V.NP[data_type])
        fv = np.frombuffer(fb, self.dtype)[0]
        mc = V.ModelChain(codecs, data_type, fill, self.nd) if any(c["name"] == V.FSO for c in codecs) else \
            O.OracleChain.from_metadata(codecs, data_type, fb, self.nd)
        self.grid = [-(-a // c) for a, c in zip(array_shape, chunk_shape)]
        padded = np.full([g * c for g, c in zip(self.grid, chunk_shape)], fv, self.dtype)
        inside = tuple(slice(0, a) for a in array_shape)
        padded[inside] = source(data_type, array_shape, seed)
        for box in holes:
            padded[box] = fv
        self.mem = MemoryStore()
        arr = Array(self.mem, self.meta, ctx)
        for idx in itertools.product(*[range(g) for g in self.grid]):
            box = tuple(slice(i * c, (i + 1) * c) for i, c in zip(idx, chunk_shape))
            if idx in missing:
                padded[box] = fv
            else:
                self.mem.set(arr.chunk_key(idx), bytes(mc.encode(np.ascontiguousarray(padded[box]))))
        self.a = np.ascontiguousarray(padded[inside])  # the expected values: a[tuple(points.T)]
        self.dev = DeviceStore.from_store(self.mem)
        self.arr = {False: arr, True: Array(self.dev, self.meta, ctx)}

    def points(self, n, seed=3):
        """n points: the corners first ([0, ...], the array's last element, the last valid element of an
        edge chunk on each axis), then uniform ones, a third of them repeated."""
        rng = np.random.default_rng(seed)
        last = [a - 1 for a in self.shape]
        pts = [[0] * self.nd, last]
        for d in range(self.nd):
            p = [min(c, a) - 1 for a, c in zip(self.shape, self.chunk_shape)]
            p[d] = last[d]
            pts.append(p)
        more = np.stack([rng.integers(0, a, size=max(n, 1)) for a in self.shape], axis=1)
        pts = np.concatenate([np.asarray(pts, np.int64), more])[:n]
        if n >= 9:
            pts[n - n // 3:] = pts[:n // 3]  # duplicates
        return pts.reshape(n, self.nd)

    def expect(self, pts):
        return self.a[tuple(np.asarray(pts, np.int64).reshape(-1, self.nd).T)]


def tdtype(torch, dt):
    """the torch dtype that carries dt's bytes (uint16 travels as int16)"""
    return {"u1": torch.uint8, "u2": torch.int16, "f4": torch.float32, "f8": torch.float64,
            "c16": torch.complex128}[np.dtype(dt).str[1:]]


def read(torch, rig, pts, dev_store, dev_idx, dev_out, arr=None, sentinel=0xA5):
    """one retrieve_elements; the output as a numpy array of the rig's dtype"""
    arr = arr or rig.arr[dev_store]
    n = len(pts)
    idx = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.int64)).cuda() if dev_idx else pts
    es = rig.dtype.itemsize
    if dev_out:
        raw = torch.full((max(n * es, 1),), sentinel, dtype=torch.uint8, device="cuda")
        out = raw[:n * es].view(tdtype(torch, rig.dtype))
        got = arr.retrieve_elements(idx, out)
        assert got is out
        torch.cuda.synchronize()
        return raw[:n * es].cpu().numpy().view(rig.dtype)
    out = np.full(n * es, sentinel, np.uint8).view(rig.dtype)
    assert arr.retrieve_elements(idx, out) is out
    return out


def counters():
    import ctypes as C
    from zarrs_amd import _lib as L
    ctr = (C.c_uint64 * L.N_COUNTERS)()
    L.load().zgpu_last_counters(ctr, L.N_COUNTERS)
    return list(ctr)


def leaves_of(pts, leaf_shape):
    return {tuple(int(x) // l for x, l in zip(p, leaf_shape)) for p in pts}


PATHS = list(itertools.product([False, True], repeat=3))  # (device store, device indices, device out)


@pytest.fixture(scope="module")
def rigs(ctx):
    return {name: Rig(ctx, c, dt, a, cs, holes=holes) for name, (c, dt, a, cs, _, holes) in CHAINS.items()}


@pytest.mark.parametrize("name", list(CHAINS))
def test_chains_counts_and_paths(torch, rigs, name):
    from zarrs_amd import _lib as L
    rig, leaf = rigs[name], CHAINS[name][4]
    for n in COUNTS:
        pts = rig.points(n)
        exp = rig.expect(pts)
        for dev_store, dev_idx, dev_out in (PATHS if n in (0, 65, 3000) else [(False, False, False), (True, True, True)]):
            got = read(torch, rig, pts, dev_store, dev_idx, dev_out)
            assert got.shape == (n,) and np.array_equal(got.view(np.uint8), exp.view(np.uint8)), \
                (name, n, dev_store, dev_idx, dev_out)
            ctr = counters()
            assert ctr[L.CTR_POINT_LEAVES] == len(leaves_of(pts, leaf))
            assert ctr[L.CTR_POINT_ROUNDS] == (1 if n else 0)
            assert ctr[L.CTR_ITEMS] == len(leaves_of(pts, leaf))  # each touched leaf once, no other
    # without out, a numpy array comes back
    pts = rig.points(65)
    got = rig.arr[False].retrieve_elements(pts)
    assert isinstance(got, np.ndarray) and got.dtype == rig.dtype and np.array_equal(got, rig.expect(pts))


@pytest.mark.parametrize("data_type", DTYPES)
def test_element_sizes(torch, ctx, data_type):
    """element sizes 1, 2, 4, 8 and 16, unsharded ([20,33,40] / [8,16,16]: edge chunks reach past the array)
    and through inner chunks"""
    for codecs, a, c in (([BYTES], [20, 33, 40], [8, 16, 16]), ([sh([4, 8], [BYTES_BIG, CRC])], [24, 40], [16, 16])):
        rig = Rig(ctx, codecs, data_type, a, c, seed=7)
        for n in (65, 3000):
            pts = rig.points(n)
            for dev_store, dev_idx, dev_out in PATHS:
                got = read(torch, rig, pts, dev_store, dev_idx, dev_out)
                assert np.array_equal(got.view(np.uint8), rig.expect(pts).view(np.uint8)), (data_type, n)


def test_missing_chunk_and_missing_inner_chunk_read_as_fill(torch, ctx):
    from zarrs_amd import _lib as L
    # a missing chunk key: nothing is decoded for it, its points read the fill value
    rig = Rig(ctx, [BYTES, GZIP], "float32", [20, 33, 40], [8, 16, 16], fill=-2.5, missing={(1, 1, 1), (2, 2, 2)})
    pts = np.concatenate([rig.points(257), [[8, 16, 16], [15, 31, 31], [19, 32, 39]]])
    for dev_store, dev_idx, dev_out in PATHS:
        got = read(torch, rig, pts, dev_store, dev_idx, dev_out)
        assert np.array_equal(got, rig.expect(pts))
        assert np.all(got[-3:] == np.float32(-2.5))
        ctr = counters()
        touched = leaves_of(pts, [8, 16, 16])
        assert {(1, 1, 1), (2, 2, 2)} <= touched
        assert ctr[L.CTR_POINT_LEAVES] == len(touched)
        assert ctr[L.CTR_ITEMS] == len(touched) - 2  # the two missing keys are not decoded
    # only points of missing chunks: nothing decoded at all
    got = read(torch, rig, pts[-3:], False, False, False)
    assert np.all(got == np.float32(-2.5)) and counters()[L.CTR_ITEMS] == 0


def test_c3_decodes_touched_inner_chunks_only(torch, rigs):
    """50 points in the [32,32,32] shard, as test_gpu_plugin_paths.py's generic-indexer test: the items
    planned are the distinct inner chunks, fewer than the points; the omitted inner chunk reads as fill."""
    from zarrs_amd import _lib as L
    rig = rigs["c3"]
    rng = np.random.default_rng(9)
    pts = rng.integers(0, 32, size=(50, 3))
    pts[:5] = [[9, 3, 17], [10, 4, 18], [0, 0, 0], [31, 31, 31], [9, 3, 17]]  # repeats + the empty inner chunk
    distinct = len(leaves_of(pts, [8, 8, 8]))
    for dev_store, dev_idx, dev_out in PATHS:
        got = read(torch, rig, pts, dev_store, dev_idx, dev_out)
        assert np.array_equal(got, rig.expect(pts))
        assert got[0] == 0.0 and got[1] == 0.0 and got[4] == 0.0
        ctr = counters()
        assert ctr[L.CTR_ITEMS] == distinct < 50
        assert ctr[L.CTR_POINT_LEAVES] == distinct


def test_rounds(torch, ctx, monkeypatch):
    """1 MiB leaves against a 2 MiB budget: five touched leaves take three rounds, same output"""
    from zarrs_amd import _lib as L
    rig = Rig(ctx, [BYTES], "float32", [64, 64, 320], [64, 64, 64], seed=11)
    pts = rig.points(3000)
    assert len(leaves_of(pts, [64, 64, 64])) == 5
    monkeypatch.delenv("ZGPU_POINTS_SCRATCH_MB", raising=False)
    one = read(torch, rig, pts, True, True, True)
    assert counters()[L.CTR_POINT_ROUNDS] == 1
    assert np.array_equal(one, rig.expect(pts))
    monkeypatch.setenv("ZGPU_POINTS_SCRATCH_MB", "2")
    for dev_store, dev_idx, dev_out in ((True, True, True), (False, False, False)):
        cut = read(torch, rig, pts, dev_store, dev_idx, dev_out)
        ctr = counters()
        assert ctr[L.CTR_POINT_ROUNDS] >= 3 and ctr[L.CTR_POINT_LEAVES] == 5 and ctr[L.CTR_ITEMS] == 5
        assert np.array_equal(cut.view(np.uint8), one.view(np.uint8))
    monkeypatch.setenv("ZGPU_POINTS_SCRATCH_MB", "0")  # at least one leaf per round
    cut = read(torch, rig, pts, True, True, True)
    assert counters()[L.CTR_POINT_ROUNDS] == 5 and np.array_equal(cut.view(np.uint8), one.view(np.uint8))


def raw_retrieve(torch, rig, pts, dev_idx, out):
    """zgpu_retrieve_elements itself over the device store, every chunk's pointer in the table (the Python
    surface checks host indices on the host first)"""
    import ctypes as C
    from zarrs_amd import _lib as L
    arr = rig.arr[True]
    ptrs, lens, keep = arr._tables([0] * rig.nd, rig.shape)
    pts = np.ascontiguousarray(pts, dtype=np.int64)
    idx = torch.from_numpy(pts).cuda() if dev_idx else pts
    torch.cuda.synchronize()
    odev = isinstance(out, torch.Tensor)
    flags = L.ENC_DEVICE | (L.IDX_DEVICE if dev_idx else 0) | (L.OUT_DEVICE if odev else 0)
    rc = L.load().zgpu_retrieve_elements(arr.codecs._h, rig.nd, L.u64s(rig.shape), L.u64s(rig.chunk_shape), ptrs, lens,
                                         idx.data_ptr() if dev_idx else pts.ctypes.data, len(pts),
                                         out.data_ptr() if odev else out.ctypes.data, flags, None)
    del keep
    return rc, L.last_error()


@pytest.mark.parametrize("dev_idx", [False, True], ids=["host_indices", "device_indices"])
def test_out_of_bounds_point_fails_the_call(torch, rigs, dev_idx):
    """nothing is decoded or written: out keeps its sentinel. (The bounds check rejects the point; it is
    never dereferenced.)"""
    from zarrs_amd import _lib as L
    rig = rigs["bytes"]
    for at, axis, bad in ((0, 0, 20), (256, 1, 33), (128, 2, 2 ** 40), (7, 2, 40), (5, 0, -1)):
        pts = rig.points(257)
        pts[at, axis] = bad
        for dev_out in (False, True):
            out = torch.full((257,), -7.0, dtype=torch.float32, device="cuda") if dev_out else \
                np.full(257, -7.0, np.float32)
            # the entry itself: the mark kernel finds the point, for host indices too
            rc, msg = raw_retrieve(torch, rig, pts, dev_idx, out)
            assert rc == L.INVALID_ARGUMENT
            assert f"point {at} " in msg and f"axis {axis}" in msg, msg
            assert counters()[L.CTR_ITEMS] == 0
            assert np.all((out.cpu().numpy() if dev_out else out) == np.float32(-7.0))
            if bad < 0:
                continue  # (the Python surface's own check of negative host indices: test_python_surface)
            for dev_store in (False, True):
                idx = torch.from_numpy(pts).cuda() if dev_idx else pts
                with pytest.raises(L.ZgpuError) as e:
                    rig.arr[dev_store].retrieve_elements(idx, out)
                assert e.value.status == L.INVALID_ARGUMENT
                assert f"point {at} " in str(e.value) and f"axis {axis}" in str(e.value), str(e.value)
                assert np.all((out.cpu().numpy() if dev_out else out) == np.float32(-7.0))
    # two offending points: the smallest index is the one named
    pts = rig.points(3000)
    pts[2999, 0] = 20
    pts[1234, 2] = 40
    rc, msg = raw_retrieve(torch, rig, pts, dev_idx, np.full(3000, -7.0, np.float32))
    assert rc == L.INVALID_ARGUMENT and "point 1234 " in msg, msg
    # a negative coordinate in a device tensor is a coordinate >= 2^63 to the bounds check
    if dev_idx:
        pts = rig.points(65)
        pts[64, 1] = -1
        with pytest.raises(L.ZgpuError) as e:
            rig.arr[True].retrieve_elements(torch.from_numpy(pts).cuda())
        assert e.value.status == L.INVALID_ARGUMENT and "point 64 " in str(e.value)


def _flip(store_bytes, inner_lin, n_inner):
    """the shard with one byte flipped in the middle of inner chunk inner_lin (index at the end, + crc32c)"""
    enc = np.frombuffer(store_bytes, np.uint8).copy()
    index = np.frombuffer(enc[len(enc) - (16 * n_inner + 4):len(enc) - 4].tobytes(), np.uint64).reshape(-1, 2)
    off, nb = (int(v) for v in index[inner_lin])
    enc[off + nb // 2] ^= 0x5A
    return bytes(enc)


def test_corrupt_inner_chunk(torch, ctx):
    """a flipped byte in a touched gzip inner chunk gives the status the box read gives for the same
    shard; in an untouched one it does not matter"""
    from zarrs_amd import Array, DeviceStore, MemoryStore
    from zarrs_amd import _lib as L
    codecs, dt, a, cs, leaf, holes = CHAINS["c3"]
    rig = Rig(ctx, codecs, dt, a, cs, holes=holes)
    key = rig.arr[False].chunk_key((0, 0, 0))
    bad_ci = (2, 1, 3)
    mem = MemoryStore()
    mem.set(key, _flip(rig.mem[key], (bad_ci[0] * 4 + bad_ci[1]) * 4 + bad_ci[2], 64))
    stores = {False: mem, True: DeviceStore.from_store(mem)}
    pts = rig.points(257)
    inside = np.all(pts // 8 == np.asarray(bad_ci), axis=1)
    touching = np.concatenate([pts, [[16 + 3, 8 + 2, 24 + 1]]])
    avoiding = pts[~inside]
    assert len(avoiding) > 200
    for dev_store in (False, True):
        arr = Array(stores[dev_store], rig.meta, ctx)
        with pytest.raises(L.ZgpuError) as box:
            arr.retrieve_array_subset([16, 8, 24], [8, 8, 8])
        assert box.value.status != L.OK
        for dev_idx, dev_out in itertools.product([False, True], repeat=2):
            with pytest.raises(L.ZgpuError) as e:
                read(torch, rig, touching, dev_store, dev_idx, dev_out, arr=arr)
            assert e.value.status == box.value.status, (e.value.status, box.value.status)
            got = read(torch, rig, avoiding, dev_store, dev_idx, dev_out, arr=arr)
            assert np.array_equal(got, rig.expect(avoiding))


def test_cache(torch, ctx):
    from zarrs_amd import ArrayCached, ChunkCacheDecodedLruSizeLimit
    from zarrs_amd import _lib as L
    rig = Rig(ctx, [BYTES, GZIP, CRC], "float32", [20, 33, 40], [8, 16, 16], fill=1.5, missing={(0, 1, 2)}, seed=4)
    chunk_bytes = 8 * 16 * 16 * 4
    n_chunks = int(np.prod(rig.grid))
    for dev_store in (False, True):
        cache = ChunkCacheDecodedLruSizeLimit(n_chunks * chunk_bytes, ctx)
        ac = ArrayCached(rig.arr[dev_store], cache)
        # points in three chunks (one of them a missing key): one miss per touched chunk
        first = np.asarray([[0, 0, 0], [1, 2, 3], [7, 15, 15], [0, 16, 32], [7, 31, 39], [3, 20, 35], [19, 32, 39],
                            [0, 0, 0]])
        got = ac.retrieve_elements(first)
        assert np.array_equal(got, rig.expect(first)) and got[3] == np.float32(1.5)
        st = cache.stats()
        assert (st["hits"], st["misses"], st["entries"]) == (0, 3, 3)
        ctr = counters()
        assert ctr[L.CTR_ITEMS] == 2 and ctr[L.CTR_POINT_LEAVES] == 3 and ctr[L.CTR_POINT_ROUNDS] == 1
        # other points in the same chunks: hits only, nothing decoded
        for dev_idx, dev_out in itertools.product([False, True], repeat=2):
            second = np.asarray([[5, 5, 5], [2, 17, 38], [16, 32, 32], [18, 32, 33], [5, 5, 5]])
            before = cache.stats()
            got = read(torch, rig, second, dev_store, dev_idx, dev_out, arr=ac)
            assert np.array_equal(got, rig.expect(second))
            st = cache.stats()
            assert (st["hits"] - before["hits"], st["misses"], st["entries"]) == (3, 3, 3)
            assert counters()[L.CTR_ITEMS] == 0
        # a subset read of a cached chunk hits what the point read cached
        before = cache.stats()
        assert np.array_equal(ac.retrieve_chunk((0, 0, 0)), rig.a[:8, :16, :16])
        assert cache.stats()["hits"] == before["hits"] + 1 and cache.stats()["misses"] == before["misses"]
        # every point count through the cache
        for n in COUNTS:
            pts = rig.points(n)
            assert np.array_equal(ac.retrieve_elements(pts), rig.expect(pts)), n
        # a cache of one chunk, points in three chunks: the direct path, nothing new cached
        small = ChunkCacheDecodedLruSizeLimit(chunk_bytes, ctx)
        asmall = ArrayCached(rig.arr[dev_store], small)
        three = np.asarray([[0, 0, 0], [9, 1, 1], [17, 30, 20], [9, 1, 2]])
        got = asmall.retrieve_elements(three)
        assert np.array_equal(got, rig.expect(three))
        assert small.stats()["entries"] == 0 and small.stats()["bytes_used"] == 0
        ctr = counters()
        assert ctr[L.CTR_ITEMS] == 3 and ctr[L.CTR_POINT_LEAVES] == 3
        one = np.asarray([[9, 1, 1], [9, 2, 2]])  # one chunk fits
        assert np.array_equal(asmall.retrieve_elements(one), rig.expect(one))
        assert small.stats()["entries"] == 1 and small.stats()["bytes_used"] == chunk_bytes


def test_python_surface(torch, rigs):
    from zarrs_amd import _lib as L
    rig = rigs["bytes"]
    pts = rig.points(257)
    exp = rig.expect(pts)
    # the tuple-of-arrays form, numpy and device tensors, and other integer types
    cols = tuple(pts[:, d].copy() for d in range(3))
    assert np.array_equal(rig.arr[False].retrieve_elements(cols), exp)
    assert np.array_equal(rig.arr[True].retrieve_elements(tuple(torch.from_numpy(c).cuda() for c in cols)), exp)
    assert np.array_equal(rig.arr[False].retrieve_elements(pts.astype(np.uint16)), exp)
    assert np.array_equal(rig.arr[True].retrieve_elements(torch.from_numpy(pts.astype(np.int32)).cuda()), exp)
    # device indices over a host store go through the host
    assert np.array_equal(rig.arr[False].retrieve_elements(torch.from_numpy(pts).cuda()), exp)
    # negative indices are rejected: no wrap-around
    for dev_store in (False, True):
        neg = pts.copy()
        neg[3, 2] = -1
        with pytest.raises(L.ZgpuError) as e:
            rig.arr[dev_store].retrieve_elements(neg)
        assert e.value.status == L.INVALID_ARGUMENT
        with pytest.raises(L.ZgpuError) as e:
            rig.arr[dev_store].retrieve_elements((cols[0], -cols[1] - 1, cols[2]))
        assert e.value.status == L.INVALID_ARGUMENT
    # a list of ndim arrays is a list of points, as numpy reads it; only a tuple is the column form
    three = [np.array([1, 2, 3]), np.array([4, 5, 6]), np.array([7, 8, 9])]
    assert np.array_equal(rig.arr[False].retrieve_elements(three), rig.a[[1, 4, 7], [2, 5, 8], [3, 6, 9]])
    assert np.array_equal(rig.arr[False].retrieve_elements(tuple(three)), rig.a[[1, 2, 3], [4, 5, 6], [7, 8, 9]])
    # an out of another element size, or one that is not contiguous, is refused before anything is written
    for bad_out in (np.zeros(257, np.float64), np.zeros(257, np.uint16), np.zeros(514, np.float32)[::2],
                    torch.zeros(257, dtype=torch.float16, device="cuda"),
                    torch.zeros(514, dtype=torch.float32, device="cuda")[::2]):
        with pytest.raises(L.ZgpuError) as e:
            rig.arr[True].retrieve_elements(pts, bad_out)
        assert e.value.status == L.INVALID_ARGUMENT
        assert not np.any(bad_out.cpu().numpy() if isinstance(bad_out, torch.Tensor) else bad_out)
    # shapes that are no list of points, and an out of another length
    for bad in (pts[:, :2], pts.reshape(-1), (cols[0], cols[1])):
        with pytest.raises(L.ZgpuError) as e:
            rig.arr[False].retrieve_elements(bad)
        assert e.value.status == L.INVALID_ARGUMENT
    with pytest.raises(L.ZgpuError) as e:
        rig.arr[False].retrieve_elements(pts, np.empty(256, np.float32))
    assert e.value.status == L.INVALID_ARGUMENT


def test_filesystem_store(torch, ctx, tmp_path):
    """a FilesystemStore is read through store.get: only the touched keys"""
    from zarrs_amd import Array, FilesystemStore
    rig = Rig(ctx, [BYTES, GZIP], "uint16", [24, 40], [16, 16], seed=2)
    fs = FilesystemStore(tmp_path)
    for k, v in rig.mem.items():
        fs.set(k, v)
    arr = Array(fs, rig.meta, ctx)
    pts = rig.points(257)
    assert np.array_equal(arr.retrieve_elements(pts), rig.expect(pts))
    got = arr.retrieve_elements(pts, torch.empty(257, dtype=torch.int16, device="cuda"))
    assert np.array_equal(got.cpu().numpy().view(np.uint16), rig.expect(pts))


def test_wide_geometry(torch, ctx):
    """an array extent above 2^32 takes the kernels' 64-bit instantiations: [2^33 + 5, 6] uint16 in chunks of
    [2^20, 4], three keys present (the first chunk, one in the middle, the last, which reaches past the
    array), every other point reads the fill value"""
    from zarrs_amd import Array, DeviceStore, MemoryStore
    from zarrs_amd import _lib as L
    shape, chunk, fill = [2 ** 33 + 5, 6], [2 ** 20, 4], 7
    assert L.points_geometry(shape, chunk) == (8193 * 2, True)
    meta = {"shape": shape, "data_type": "uint16", "fill_value": fill, "codecs": [BYTES, CRC],
            "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": chunk}}}
    oc = O.OracleChain.from_metadata([BYTES, CRC], "uint16", np.uint16(fill).tobytes(), 2)
    rng = np.random.default_rng(21)
    mem, data = MemoryStore(), {}
    arr = Array(mem, meta, ctx)
    for idx in ((0, 0), (5000, 1), (8192, 1)):
        data[idx] = rng.integers(8, 60000, chunk, dtype=np.uint16)
        mem.set(arr.chunk_key(idx), bytes(oc.encode(data[idx])))
    arrs = {False: arr, True: Array(DeviceStore.from_store(mem), meta, ctx)}
    n = 3000
    pts = np.stack([rng.integers(0, shape[0], size=n), rng.integers(0, shape[1], size=n)], axis=1).astype(np.int64)
    for k, (ci, cj) in enumerate(data):  # a third of the points in each present chunk, inside the array
        sel = slice(k * 500, (k + 1) * 500)
        pts[sel, 0] = ci * chunk[0] + rng.integers(0, min(chunk[0], shape[0] - ci * chunk[0]), size=500)
        pts[sel, 1] = cj * chunk[1] + rng.integers(0, min(chunk[1], shape[1] - cj * chunk[1]), size=500)
    pts[1500:1506] = [[0, 0], [shape[0] - 1, shape[1] - 1], [2 ** 32, 0], [2 ** 32 - 1, 5], [2 ** 33 + 4, 4],
                      [5000 * 2 ** 20, 4]]
    pts[2000:2500] = pts[:500]  # duplicates
    exp = np.full(n, fill, np.uint16)
    for i, (x, y) in enumerate(pts):
        d = data.get((int(x) // chunk[0], int(y) // chunk[1]))
        if d is not None:
            exp[i] = d[int(x) % chunk[0], int(y) % chunk[1]]
    assert np.count_nonzero(exp != fill) > 1500
    leaves = leaves_of(pts, chunk)
    for dev_store, dev_idx, dev_out in PATHS:
        idx = torch.from_numpy(pts).cuda() if dev_idx else pts
        out = torch.zeros(n, dtype=torch.int16, device="cuda") if dev_out else np.zeros(n, np.uint16)
        arrs[dev_store].retrieve_elements(idx, out)
        got = out.cpu().numpy().view(np.uint16) if dev_out else out
        assert np.array_equal(got, exp), (dev_store, dev_idx, dev_out)
        ctr = counters()
        assert ctr[L.CTR_POINT_LEAVES] == len(leaves) and ctr[L.CTR_ITEMS] == 3
    # out of bounds above 2^32, found by the 64-bit mark kernel
    bad = pts.copy()
    bad[2999, 0] = shape[0]
    with pytest.raises(L.ZgpuError) as e:
        arrs[True].retrieve_elements(torch.from_numpy(bad).cuda())
    assert e.value.status == L.INVALID_ARGUMENT and "point 2999 " in str(e.value) and "axis 0" in str(e.value)


def test_bitmap_limit(torch, ctx):
    """more leaves than the dense bitmap's limit holds: ZGPU_UNSUPPORTED with a message that says so; the
    limit itself is accepted. (Inner chunks of one element in shards of 2^20 keep the chunk grid, and so
    the pointer tables, small; no shard is present, so nothing is decoded.)"""
    import ctypes as C
    from zarrs_amd import CodecChain
    from zarrs_amd import _lib as L
    chain = CodecChain.from_metadata([sh([1], [BYTES])], "uint8", 3, ctx)
    limit = L.POINTS_BITMAP_MAX_BYTES * 8
    shard = 2 ** 20
    pts = np.asarray([[5], [limit - 1]], np.uint64)
    ptrs, lens = (C.c_void_p * (limit // shard + 1))(), (C.c_uint64 * (limit // shard + 1))()
    for extent, leaves, want in ((limit + 1, limit + shard, L.UNSUPPORTED), (limit, limit, L.OK)):
        assert L.points_geometry([extent], [shard], [1]) == (leaves, False)
        out = np.full(2, 9, np.uint8)
        rc = L.load().zgpu_retrieve_elements(chain._h, 1, L.u64s([extent]), L.u64s([shard]), ptrs, lens,
                                             pts.ctypes.data, 2, out.ctypes.data, 0, None)
        assert rc == want, L.last_error()
        if want == L.UNSUPPORTED:
            assert str(L.POINTS_BITMAP_MAX_BYTES) in L.last_error() and np.all(out == 9)
        else:
            assert np.all(out == 3) and counters()[L.CTR_POINT_LEAVES] == 2 and counters()[L.CTR_ITEMS] == 0
