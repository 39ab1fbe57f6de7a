"""Array.store_elements on the GPU (zgpu_store_elements: store.cpp, k_points_claim / k_points_scatter in
kernels/points.hip) against the numpy model of its rules (tests/store_points_model.py, which
test_store_points_model.py holds to brute force). After every store the store's key set equals the
model's, every chunk the call wrote is decoded by the CPU oracle (the cast_value model for that chain)
and equals the model bit for bit, every other key holds the bytes it held, and the counters equal the
model's counts. Old shards are laid out by tests/shard_model.py."""
import ctypes as C

import numpy as np
import pytest

import cast_value_model as CM
import oracle as O
import shard_model as SH
import store_model as M
import store_points_model as PM
import test_gpu_store as S
import value_codecs as V

pytestmark = pytest.mark.gpu

BYTES, BYTES_BIG, CRC, GZIP, ZSTD = S.BYTES, S.BYTES_BIG, S.CRC, S.GZIP, S.ZSTD
CAST = {"name": CM.NAME, "configuration": {"data_type": "int16"}}
CHAINS = {
    "bytes": [BYTES],
    "big_crc": [BYTES_BIG, CRC],
    "gzip": [BYTES, GZIP],
    "tr_zstd": [S.tr([1, 0]), BYTES, ZSTD],
}
DTYPES = [("uint8", 0), ("int16", -3), ("float32", 2.5), ("float64", 0.0), ("complex128", [0.0, 0.0])]  # ES 1 .. 16
A2, C2 = [10, 13], [4, 5]  # a 3 x 3 grid whose last row and column reach past the array


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    return Context(0)


class Rig(S.Rig):
    """test_gpu_store.Rig with missing chunks in the seeded store and the cast_value model as a decoder."""

    def __init__(self, ctx, torch, codecs, data_type, fill, array_shape, chunk_shape, device, seeded=True,
                 leaf_shape=None, seed=1, missing=()):
        from zarrs_amd import Array, DeviceStore, MemoryStore, fill_value_bytes
        self.torch, self.device, self.nd = torch, device, len(array_shape)
        self.meta = {"shape": array_shape, "data_type": data_type, "fill_value": fill, "codecs": codecs,
                     "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": chunk_shape}}}
        fb = fill_value_bytes(data_type, fill)
        cast = any(c["name"] == CM.NAME for c in codecs)
        self.mc = CM.CastModelChain(codecs, data_type, fill, self.nd) if cast else \
            O.OracleChain.from_metadata(codecs, data_type, fb, self.nd)
        self.dtype = np.dtype(V.NP[data_type])
        rt = (lambda a: self.mc.decode(self.mc.encode(a), list(a.shape))) if cast else None
        self.model = M.StoreModel(array_shape, chunk_shape, self.dtype, fb, leaf_shape, rt,
                                  self.mc.decoded_fill([1])[0] if cast else None)
        self.store = DeviceStore() if device else MemoryStore()
        self.arr = Array(self.store, self.meta, ctx)
        if seeded:
            raw = S.random_data(self.dtype, self.model.padded.shape, seed)
            self.model.fill_from(raw)
            for idx in self.model.chunks():
                if idx in missing:
                    self.model.present -= {(idx, j) for j in self.model.leaves()}
                    self.model.padded[self.model.chunk_box(idx)] = self.model.missing
                elif idx in self.model.keys():
                    self.put(idx, self.mc.encode(raw[self.model.chunk_box(idx)]))

    def give_points(self, pts):
        pts = np.ascontiguousarray(pts, dtype=np.int64).reshape(-1, self.nd)
        return self.torch.from_numpy(pts).cuda() if self.device else pts

    def apply_points(self, pts, data, store_empty_chunks=False):
        """one store through the library and through the model, and every check that needs no index"""
        from zarrs_amd import _lib as L
        before = self.snapshot()
        r = PM.store_elements(self.model, pts, data, store_empty_chunks)
        done = self.arr.store_elements(self.give_points(pts), self.give(np.ascontiguousarray(data)), store_empty_chunks)
        ctr = L.last_counters()
        want = [(self.key(idx), L.STORE_SET if a == "set" else L.STORE_ERASE) for idx, a in sorted(r["actions"].items())]
        assert done == want
        after = self.snapshot()
        assert set(after) == self.model.keys()
        for idx, enc in after.items():
            if idx in r["actions"]:
                got = self.mc.decode(enc, self.model.chunk_shape)
                assert got.tobytes() == np.ascontiguousarray(self.model.padded[self.model.chunk_box(idx)]).tobytes(), idx
            else:
                assert enc == before[idx], idx
        assert (ctr["store_decoded"], ctr["store_encoded"], ctr["store_carried"], ctr["point_leaves"]) == \
            (r["decoded"], r["encoded"], r["carried"], r["leaves"])
        return r, before, after

    def raw(self, pts, data, dev_idx, dev_data, store_empty_chunks=False):
        """zgpu_store_elements itself, every chunk's pointer in the tables: (rc, [(chunk, action, status,
        encoded bytes or None)]); nothing is applied to the store"""
        from zarrs_amd import _lib as L
        ptrs, lens, keep = self.arr._tables([0] * self.nd, self.arr.shape)
        pts = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, self.nd)
        idx = self.torch.from_numpy(pts.view(np.int64)).cuda() if dev_idx else pts
        d = S.to_device(self.torch, data) if dev_data else np.ascontiguousarray(data)
        self.torch.cuda.synchronize()
        res = self.arr.codecs.store_elements(self.arr.shape, self.arr.chunk_shape, ptrs, lens,
                                             idx.data_ptr() if dev_idx else idx.ctypes.data, len(pts), dev_idx, d,
                                             self.device, store_empty_chunks)
        del keep
        ents = []
        for i, (lin, action, status, _, _) in enumerate(res.entries):
            enc = res.encoded(i) if action == L.STORE_SET else None
            ents.append((lin, action, status, enc if enc is None or not self.device else bytes(enc.cpu().numpy())))
        res.release()
        return res.rc, ents


def counters():
    from zarrs_amd import _lib as L
    ctr = (C.c_uint64 * L.N_COUNTERS)()
    L.load().zgpu_last_counters(ctr, L.N_COUNTERS)
    return list(ctr)


def points40(seed=5):
    """40 points in [10, 13] / [4, 5]: chunks (0, 2) and (2, 0) untouched, chunk (2, 2) touched by one point,
    every other chunk by several; four points repeat earlier coordinates"""
    rng = np.random.default_rng(seed)
    chunks = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 1)]
    pts = []
    while len(pts) < 35:
        c = chunks[len(pts) % len(chunks)]
        p = [c[0] * 4 + int(rng.integers(4)), c[1] * 5 + int(rng.integers(5))]
        if p[0] < 10 and p[1] < 13:
            pts.append(p)
    pts += [[9, 12], pts[3], pts[7], pts[3], pts[20]]
    return np.asarray(pts, np.int64)


# ---------------------------------------------------------------------------------------------------
# unsharded chains and element sizes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_unsharded_chains_and_dtypes(ctx, torch_cuda, chain, device):
    pts = points40()
    for k, (dt, fill) in enumerate(DTYPES):
        rig = Rig(ctx, torch_cuda, CHAINS[chain], dt, fill, A2, C2, device, missing={(1, 1)})
        assert (1, 1) not in rig.snapshot()
        r, _, after = rig.apply_points(pts, S.random_data(rig.dtype, [40], 30 + k))
        assert set(r["actions"]) == {(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2)}
        assert set(r["actions"].values()) == {"set"} and r["decoded"] == 6 and (1, 1) in after
        rig.read_back()


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
def test_unsharded_cast_value_chain(ctx, torch_cuda, device):
    rig = Rig(ctx, torch_cuda, [CAST, BYTES, ZSTD], "float32", 0.0, A2, C2, device, missing={(1, 1)})
    r, _, _ = rig.apply_points(points40(), S.random_data(rig.dtype, [40], 3))
    assert len(r["actions"]) == 7
    rig.read_back()


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("dt", ["uint8", "int16"])
def test_neighbours_in_one_dword(ctx, torch_cuda, dt, device):
    """every element of a 64-element chunk written by its own point, in shuffled order: a store wider than
    the element (a read-modify-write of the dword) would lose neighbours"""
    rig = Rig(ctx, torch_cuda, [BYTES], dt, 0, [64], [64], device)
    perm = np.random.default_rng(8).permutation(64)
    data = (perm + 100).astype(rig.dtype)
    _, _, after = rig.apply_points(perm.reshape(-1, 1), data)
    assert after[(0,)] == (np.arange(64) + 100).astype(rig.dtype).tobytes()


# ---------------------------------------------------------------------------------------------------
# duplicates: the last point wins
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("dt,fill", [("float32", 0.0), ("complex128", [0.0, 0.0])])
def test_duplicates_last_wins(ctx, torch_cuda, dt, fill, device):
    rig = Rig(ctx, torch_cuda, [BYTES], dt, fill, [8, 8], [8, 8], device)
    pts = [[1, 1], [3, 4], [0, 7], [1, 1], [7, 7], [6, 2], [1, 1], [3, 4]]
    data = np.arange(10, 90, 10).astype(rig.dtype)
    _, _, after = rig.apply_points(pts, data)
    got = np.frombuffer(after[(0, 0)], rig.dtype).reshape(8, 8)
    assert got[1, 1] == 70 and got[3, 4] == 80 and got[0, 7] == 30 and got[7, 7] == 50
    # contended: 70,000 points over the 64 elements, about 1,100 claimants each, spread over blocks and
    # grid-stride iterations. Once, not in a loop.
    n = 70000
    i = np.arange(n)
    pts = np.stack([i % 64 // 8, i % 8], axis=1)
    data = i.astype(rig.dtype)
    want = np.empty(64, rig.dtype)
    want[i % 64] = data  # numpy assigns in order: the highest i of every element stays
    assert np.array_equal(want, np.asarray([max(j for j in range(n - 64, n) if j % 64 == e) for e in range(64)]))
    done = rig.arr.store_elements(rig.give_points(pts), rig.give(data))
    assert len(done) == 1
    assert rig.get((0, 0)) == want.tobytes()


# ---------------------------------------------------------------------------------------------------
# sharded
# ---------------------------------------------------------------------------------------------------
AS, SS, IS = [16, 16], [8, 8], [4, 4]
INNER = [BYTES, GZIP, CRC]  # shard_model.GZ_CRC
X = 4 * 16 + 4


def sharded_rig(ctx, torch, location, device, seeded=True):
    """[16, 16] float32 in shards [8, 8] of inner chunks [4, 4]. Seeded: shard (0, 0) stored out of order
    with gaps and inner chunk 2 absent, shards (0, 1) and (1, 1) in other orders, shard (1, 0) missing."""
    rig = Rig(ctx, torch, [S.sh(IS, INNER, location)], "float32", 0.0, AS, SS, device, seeded=False, leaf_shape=IS)
    if not seeded:
        return rig
    raw = S.random_data(rig.dtype, AS, 4)
    raw[4:8, 0:4] = 0.0  # inner chunk 2 of shard (0, 0)
    raw[8:16, 0:8] = 0.0  # shard (1, 0)
    rig.model.fill_from(raw)
    layouts = {(0, 0): SH.Layout(order=(3, 0, 1), pre=2, gap=5, post=3), (0, 1): SH.Layout(order=(2, 0, 3, 1)),
               (1, 1): SH.Layout(order=(1, 3, 2, 0), gap=1)}
    for idx, lay in layouts.items():
        part = raw[rig.model.chunk_box(idx)]
        inner = [None if (idx, j) not in rig.model.present else SH.encode_inner(SH.GZ_CRC, part[b])
                 for j, b in zip(rig.model.leaves(), SH.boxes(SS, IS))]
        shard, _ = SH.build_shard(inner, lay, location, ("little", ("end",)))
        rig.put(idx, shard)
    assert len(rig.model.present) == 11 and rig.model.keys() == set(layouts)
    return rig


def check_carried(rig, r, before, after, touched, at_start):
    """untouched inner chunks of every rewritten shard: as present as before, the same bytes at their new
    offsets; the new shard's inner chunks back to back in C order"""
    leaves = list(rig.model.leaves())
    for idx in r["actions"]:
        new = S.parse_index(after[idx], 4, at_start) if idx in after else [None] * 4
        old = S.parse_index(before[idx], 4, at_start) if idx in before else [None] * 4
        assert [e is not None for e in new] == [(idx, j) in rig.model.present for j in leaves]
        pos = X if at_start else 0
        for k, e in enumerate(new):
            if e is not None:
                assert e[0] == pos, (idx, k)
                pos += e[1]
            if (idx, leaves[k]) not in touched:
                assert (e is None) == (old[k] is None), (idx, k)
                if e is not None:
                    assert after[idx][e[0]:e[0] + e[1]] == before[idx][old[k][0]:old[k][0] + old[k][1]], (idx, k)


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("location", ["end", "start"])
def test_sharded(ctx, torch_cuda, location, device):
    rig = sharded_rig(ctx, torch_cuda, location, device)
    # three inner chunks of shard (0, 0) (0, the absent 2, and 3; 1 is carried), one of shard (1, 1);
    # shards (0, 1) and the missing (1, 0) get no entry
    pts = np.asarray([[0, 0], [1, 3], [5, 1], [7, 7], [4, 4], [0, 0], [13, 9], [15, 8], [5, 1]])
    data = S.random_data(rig.dtype, [9], 6)
    touched = PM.touched_leaves(rig.model, pts)
    r, before, after = rig.apply_points(pts, data)
    assert r["actions"] == {(0, 0): "set", (1, 1): "set"} and len(touched) == 4
    assert (r["decoded"], r["encoded"], r["carried"], r["leaves"]) == (3, 4, 4, 4)
    check_carried(rig, r, before, after, touched, location == "start")
    # a point into the missing shard: a new shard of one inner chunk
    pts = np.asarray([[9, 6]])
    r, before, after = rig.apply_points(pts, np.asarray([7.5], rig.dtype))
    assert r["actions"] == {(1, 0): "set"} and (r["decoded"], r["encoded"], r["carried"]) == (0, 1, 0)
    check_carried(rig, r, before, after, PM.touched_leaves(rig.model, pts), location == "start")
    rig.read_back()


# ---------------------------------------------------------------------------------------------------
# erasure
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
@pytest.mark.parametrize("store_empty", [False, True], ids=["erase", "store_empty"])
def test_erase_unsharded(ctx, torch_cuda, store_empty, device):
    want = "set" if store_empty else "erase"
    for dt, fill in (("float32", 2.5), ("uint8", 9), ("complex128", [0.0, 0.0])):
        rig = Rig(ctx, torch_cuda, [BYTES, CRC], dt, fill, A2, C2, device, seeded=False)
        fv = np.frombuffer(rig.model.fill_bytes, rig.dtype)[0]
        r, _, _ = rig.apply_points([[1, 1], [2, 3], [9, 12]], np.asarray([11, 12, 13]).astype(rig.dtype))
        assert r["actions"] == {(0, 0): "set", (2, 2): "set"}
        # every non-fill element of chunk (0, 0) takes the fill value; chunk (1, 1) is missing and gets fill only
        r, _, after = rig.apply_points([[2, 3], [1, 1], [5, 6]], np.full(3, fv, rig.dtype), store_empty)
        assert r["actions"] == {(0, 0): want, (1, 1): want}
        assert ((0, 0) in after) == store_empty and ((1, 1) in after) == store_empty and (2, 2) in after
        rig.read_back()


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
def test_erase_sharded(ctx, torch_cuda, device):
    rig = sharded_rig(ctx, torch_cuda, "end", device)
    # all 16 elements of inner chunk 3 of shard (0, 0) take the fill value: omitted from its shard
    pts = np.asarray([[r, c] for r in range(4, 8) for c in range(4, 8)])
    r, before, after = rig.apply_points(pts, np.zeros(16, rig.dtype), store_empty_chunks=True)
    assert r["actions"] == {(0, 0): "set"} and (r["decoded"], r["encoded"], r["carried"]) == (1, 0, 2)
    assert ((0, 0), (1, 1)) not in rig.model.present
    check_carried(rig, r, before, after, PM.touched_leaves(rig.model, pts), False)
    # a shard that loses its last inner chunk is erased
    rig = sharded_rig(ctx, torch_cuda, "end", device, seeded=False)
    r, _, _ = rig.apply_points([[9, 1], [10, 2]], np.asarray([1.0, 2.0], rig.dtype))
    assert r["actions"] == {(1, 0): "set"}
    r, _, after = rig.apply_points([[10, 2], [9, 1], [0, 12]], np.zeros(3, rig.dtype))
    assert r["actions"] == {(0, 1): "erase", (1, 0): "erase"} and not after


# ---------------------------------------------------------------------------------------------------
# host and device sides
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sharded", [False, True], ids=["unsharded", "sharded"])
def test_sides_give_identical_bytes(ctx, torch_cuda, sharded):
    """the same store with every input on the host, every input on the device, and two mixtures"""
    from zarrs_amd import _lib as L
    got = []
    for enc_dev, dev_idx, dev_data in ((False, False, False), (True, True, True), (False, True, False),
                                       (True, False, True)):
        if sharded:
            rig = sharded_rig(ctx, torch_cuda, "end", enc_dev)
            pts = np.asarray([[0, 0], [1, 3], [5, 1], [7, 7], [0, 0], [13, 9], [9, 9]])
        else:
            rig = Rig(ctx, torch_cuda, [BYTES, GZIP], "int16", -3, A2, C2, enc_dev, missing={(1, 1)})
            pts = points40()
        rc, ents = rig.raw(pts, S.random_data(rig.dtype, [len(pts)], 12), dev_idx, dev_data)
        assert rc == 0 and ents and all(e[1] == L.STORE_SET and e[2] == 0 for e in ents)
        got.append(ents)
    assert got[0] == got[1] == got[2] == got[3]


# ---------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
def test_out_of_bounds_point_fails_the_call(ctx, torch_cuda, device):
    from zarrs_amd import ZgpuError
    from zarrs_amd import _lib as L
    rig = Rig(ctx, torch_cuda, [BYTES, CRC], "float32", 0.0, A2, C2, device)
    before = rig.snapshot()
    data = S.random_data(rig.dtype, [40], 2)
    for at, axis, bad in ((17, 0, 10), (39, 1, 13), (0, 1, 2 ** 40), (20, 0, 2 ** 63 + 5)):
        pts = points40().astype(np.uint64)
        pts[at, axis] = bad
        for dev_idx, dev_data in ((False, False), (True, True)):
            # the entry itself: the mark kernel finds the point, for host indices too; no entries, no result
            with pytest.raises(ZgpuError) as e:
                rig.raw(pts, data, dev_idx, dev_data)
            assert e.value.status == L.INVALID_ARGUMENT
            assert f"point {at} " in str(e.value) and f"axis {axis}" in str(e.value), str(e.value)
            assert counters()[L.CTR_ITEMS] == 0 and counters()[L.CTR_STORE_ENCODED] == 0
        if bad < 2 ** 63:
            with pytest.raises(ZgpuError) as e:
                rig.arr.store_elements(rig.give_points(pts.astype(np.int64)), rig.give(data))
            assert e.value.status == L.INVALID_ARGUMENT
            assert f"point {at} " in str(e.value) and f"axis {axis}" in str(e.value), str(e.value)
        assert rig.snapshot() == before
    # two offending points: the smallest index is the one named
    pts = points40().astype(np.uint64)
    pts[31, 0] = 10
    pts[12, 1] = 13
    with pytest.raises(ZgpuError) as e:
        rig.raw(pts, data, device, device)
    assert e.value.status == L.INVALID_ARGUMENT and "point 12 " in str(e.value) and "axis 1" in str(e.value)
    # a negative host index is refused by the Python surface: no wrap-around
    neg = points40()
    neg[5, 1] = -1
    with pytest.raises(ZgpuError) as e:
        rig.arr.store_elements(neg, data)
    assert e.value.status == L.INVALID_ARGUMENT and rig.snapshot() == before


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
def test_no_points(ctx, torch_cuda, device):
    rig = Rig(ctx, torch_cuda, [BYTES, CRC], "float32", 0.0, A2, C2, device)
    before = rig.snapshot()
    assert rig.arr.store_elements(rig.give_points(np.zeros((0, 2), np.int64)), rig.give(np.zeros(0, rig.dtype))) == []
    assert rig.raw(np.zeros((0, 2), np.uint64), np.zeros(0, rig.dtype), device, device) == (0, [])
    assert rig.snapshot() == before
    # data of another length or element size is refused before anything is written
    from zarrs_amd import ZgpuError
    from zarrs_amd import _lib as L
    for bad in (np.zeros(39, np.float32), torch_cuda.zeros(40, dtype=torch_cuda.float64)):
        with pytest.raises(ZgpuError) as e:
            rig.arr.store_elements(points40(), bad)
        assert e.value.status == L.INVALID_ARGUMENT
    assert rig.snapshot() == before


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
def test_corrupt_old_chunk(ctx, torch_cuda, device):
    """a flipped byte under the crc32c of a touched chunk: its entry carries the status, the others are
    valid, and Array.store_elements applies nothing"""
    from zarrs_amd import ZgpuError
    from zarrs_amd import _lib as L
    rig = Rig(ctx, torch_cuda, [BYTES, CRC], "float32", 0.0, A2, C2, device)
    bad = bytearray(rig.get((1, 0)))
    bad[7] ^= 0x20
    rig.put((1, 0), bad)
    before = rig.snapshot()
    pts, data = points40(), S.random_data(rig.dtype, [40], 2)
    rc, ents = rig.raw(pts, data, device, device)
    assert rc == L.INVALID_CHECKSUM
    assert [(e[0], e[1], e[2]) for e in ents] == \
        [(lin, 0, L.INVALID_CHECKSUM) if lin == 3 else (lin, L.STORE_SET, 0) for lin in (0, 1, 3, 4, 5, 7, 8)]
    # the valid entries hold what the model says (the failed chunk's points were dropped, nothing else)
    m = rig.model
    PM.store_elements(m, pts, data)
    for lin, _, _, enc in ents:
        if lin != 3:
            idx = tuple(int(v) for v in np.unravel_index(lin, m.grid))
            assert rig.mc.decode(enc, C2).tobytes() == np.ascontiguousarray(m.padded[m.chunk_box(idx)]).tobytes()
    with pytest.raises(ZgpuError) as e:
        rig.arr.store_elements(rig.give_points(pts), rig.give(data))
    assert e.value.status == L.INVALID_CHECKSUM and rig.snapshot() == before
    # an untouched corrupt chunk does not matter
    keep = ~((pts[:, 0] // 4 == 1) & (pts[:, 1] // 5 == 0))
    rc, ents = rig.raw(pts[keep], data[keep], device, device)
    assert rc == 0 and [e[0] for e in ents] == [0, 1, 4, 5, 7, 8]


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
def test_corrupt_shard_index(ctx, torch_cuda, device):
    from zarrs_amd import ZgpuError
    from zarrs_amd import _lib as L
    rig = sharded_rig(ctx, torch_cuda, "end", device)
    good = rig.get((0, 0))
    bad = bytearray(good)
    bad[len(good) - X + 9] ^= 1
    rig.put((0, 0), bad)
    before = rig.snapshot()
    pts, data = np.asarray([[0, 0], [13, 9], [5, 1]]), np.asarray([1.0, 2.0, 3.0], np.float32)
    rc, ents = rig.raw(pts, data, device, device)
    assert rc == L.INVALID_CHECKSUM
    assert [(e[0], e[1], e[2]) for e in ents] == [(0, 0, L.INVALID_CHECKSUM), (3, L.STORE_SET, 0)]
    with pytest.raises(ZgpuError) as e:
        rig.arr.store_elements(rig.give_points(pts), rig.give(data))
    assert e.value.status == L.INVALID_CHECKSUM and rig.snapshot() == before
    # a shard too short for its index
    rig.put((0, 0), good[-20:])
    rc, ents = rig.raw(pts, data, device, device)
    assert rc == L.SHARD_TOO_SMALL and [(e[0], e[2]) for e in ents] == [(0, L.SHARD_TOO_SMALL), (3, 0)]


@pytest.mark.parametrize("codecs,chunk", [
    ([BYTES, {"name": "numcodecs.bz2", "configuration": {"level": 1}}], [8, 16, 16]),
    ([S.sh([4, 8, 8], [BYTES]), GZIP], [8, 16, 16]),
    ([S.tr([2, 1, 0]), S.sh([4, 8, 8], [BYTES])], [8, 16, 16]),
    ([S.sh([4, 8, 8], [S.sh([2, 4, 4], [BYTES])])], [8, 16, 16]),
], ids=["bz2", "gzip_after_sharding", "transpose_before_sharding", "nested_sharding"])
def test_refused_chains(ctx, torch_cuda, codecs, chunk):
    """the chains test_gpu_store.py::test_refused_chains shows refused, refused here before any GPU work"""
    from zarrs_amd import Array, MemoryStore, ZgpuError
    from zarrs_amd import _lib as L
    meta = {"shape": S.A3, "data_type": "uint8", "fill_value": 0, "codecs": codecs,
            "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": chunk}}}
    arr = Array(MemoryStore(), meta, ctx)
    for idx in (np.asarray([[1, 2, 3], [19, 32, 39]]), torch_cuda.tensor([[1, 2, 3], [19, 32, 39]]).cuda()):
        with pytest.raises(ZgpuError) as e:
            arr.store_elements(idx, np.ones(2, np.uint8))
        assert e.value.status == L.UNSUPPORTED and not arr.store
        ctr = counters()
        assert ctr[L.CTR_ITEMS] == 0 and ctr[L.CTR_POINT_LEAVES] == 0 and ctr[L.CTR_STORE_ENCODED] == 0


def test_value_codecs_inside_sharding_are_refused(ctx, torch_cuda):
    from zarrs_amd import Array, MemoryStore, ZgpuError
    from zarrs_amd import _lib as L
    meta = {"shape": S.A3, "data_type": "float32", "fill_value": 0.0, "codecs": [S.sh([4, 8, 8], [S.FSO, BYTES])],
            "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": [8, 16, 16]}}}
    arr = Array(MemoryStore(), meta, ctx)
    with pytest.raises(ZgpuError) as e:
        arr.store_elements([[1, 2, 3]], np.ones(1, np.float32))
    assert e.value.status == L.UNSUPPORTED and counters()[L.CTR_ITEMS] == 0


# ---------------------------------------------------------------------------------------------------
# 64-bit arithmetic
# ---------------------------------------------------------------------------------------------------
def test_wide_arithmetic(ctx, torch_cuda):
    """a 1-D uint8 array of 2^32 + 64 elements in chunks of 64, nothing stored: four points in the last
    chunk and one in the first take the kernels' 64-bit instantiations"""
    from zarrs_amd import Array, MemoryStore
    from zarrs_amd import _lib as L
    shape, chunk = [2 ** 32 + 64], [64]
    assert L.points_geometry(shape, chunk) == (2 ** 26 + 1, True)
    meta = {"shape": shape, "data_type": "uint8", "fill_value": 0, "codecs": [BYTES],
            "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": chunk}}}
    arr = Array(MemoryStore(), meta, ctx)
    pts = np.asarray([[2 ** 32 + 63], [5], [2 ** 32], [2 ** 32 + 17], [2 ** 32 + 63]], np.uint64)
    data = np.asarray([1, 2, 3, 4, 5], np.uint8)
    first, last = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    first[5], last[0], last[17], last[63] = 2, 3, 4, 5
    done = arr.store_elements(pts, data)
    assert done == [("c/0", L.STORE_SET), (f"c/{2 ** 26}", L.STORE_SET)]
    assert arr.store["c/0"] == first.tobytes() and arr.store[f"c/{2 ** 26}"] == last.tobytes()
    assert L.last_counters()["point_leaves"] == 2
    # device indices and data, the old (empty) store's tables as device tables
    n_grid = 2 ** 26 + 1
    ptrs, lens = (C.c_void_p * n_grid)(), (C.c_uint64 * n_grid)()
    idx = torch_cuda.from_numpy(pts.view(np.int64)).cuda()
    d = torch_cuda.from_numpy(data).cuda()
    torch_cuda.cuda.synchronize()
    res = arr.codecs.store_elements(shape, chunk, ptrs, lens, idx.data_ptr(), 5, True, d, True)
    assert res.rc == 0 and [(e[0], e[1], e[2], e[4]) for e in res.entries] == \
        [(0, L.STORE_SET, 0, 64), (2 ** 26, L.STORE_SET, 0, 64)]
    assert bytes(res.encoded(0).cpu().numpy()) == first.tobytes()
    assert bytes(res.encoded(1).cpu().numpy()) == last.tobytes()
    res.release()
    # out of bounds above 2^32
    bad = pts.copy()
    bad[3, 0] = 2 ** 32 + 64
    with pytest.raises(L.ZgpuError) as e:
        arr.codecs.store_elements(shape, chunk, ptrs, lens, bad.ctypes.data, 5, False, data, True)
    assert e.value.status == L.INVALID_ARGUMENT and "point 3 " in str(e.value) and "axis 0" in str(e.value)


def test_too_many_points_is_unsupported(ctx, torch_cuda):
    """n >= 2^32 - 1 is refused before any device work (nothing is read: the pointers are never used)"""
    from zarrs_amd import _lib as L
    rig = Rig(ctx, torch_cuda, [BYTES], "uint8", 0, [64], [64], False, seeded=False)
    ptrs, lens = (C.c_void_p * 1)(), (C.c_uint64 * 1)()
    one = np.zeros(8, np.uint64)
    ents, ne, res = C.POINTER(L.StoreEntry)(), C.c_uint64(), C.c_void_p()
    rc = L.load().zgpu_store_elements(rig.arr.codecs._h, 1, L.u64s([64]), L.u64s([64]), ptrs, lens, one.ctypes.data,
                                      2 ** 32 - 1, one.ctypes.data, 0, C.byref(ents), C.byref(ne), C.byref(res), None)
    assert rc == L.UNSUPPORTED and "2^32" in L.last_error() and not res and not ents and ne.value == 0


# ---------------------------------------------------------------------------------------------------
# the public API, both ways
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
def test_round_trip_through_the_public_api(ctx, torch_cuda, device):
    for rig in (Rig(ctx, torch_cuda, CHAINS["tr_zstd"], "float64", 0.0, A2, C2, device, missing={(1, 1)}),
                sharded_rig(ctx, torch_cuda, "start", device)):
        shape = rig.model.array_shape
        rng = np.random.default_rng(13)
        pts = np.stack([rng.integers(0, a, size=300) for a in shape], axis=1)
        pts[200:] = pts[:100]  # duplicates
        data = S.random_data(rig.dtype, [300], 14)
        PM.store_elements(rig.model, pts, data)
        rig.arr.store_elements(rig.give_points(pts), rig.give(data))
        winners = rig.model.padded[tuple(pts.T)]
        last = {tuple(p): i for i, p in enumerate(pts.tolist())}  # the last point on a coordinate stays
        assert np.array_equal(winners, data[[last[tuple(p)] for p in pts.tolist()]]) and len(last) < 200
        got = rig.arr.retrieve_elements(rig.give_points(pts))
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(winners).view(np.uint8))
        # the tuple-of-columns form stores the same
        done = rig.arr.store_elements(tuple(pts[:, d].copy() for d in range(len(shape))), data)
        assert done and all(a == 1 for _, a in done)
        rig.read_back()
