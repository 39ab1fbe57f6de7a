"""The store path on the CPU: the library's classifier (zgpu_store_classify, zarrs_amd/csrc/store_layout.cpp:
no device behind it) against brute force over element masks, the ctypes mirror of zgpu_store_entry against
the header, the Python surface, and the model (tests/store_model.py) against a few cases worked by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import store_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (array shape, chunk shape, leaf shape or None, [(start, shape)])
U3 = ([20, 33, 40], [8, 16, 16], None, [
    ([0, 0, 0], [20, 33, 40]), ([8, 16, 16], [8, 16, 16]), ([3, 5, 7], [11, 20, 22]), ([0, 0, 0], [20, 33, 17]),
    ([19, 32, 39], [1, 1, 1]), ([0, 0, 1], [20, 33, 3]), ([0, 0, 0], [16, 32, 32]), ([16, 32, 32], [4, 1, 8]),
    ([5, 5, 5], [0, 3, 3])])
U1 = ([4099], [256], None, [([255], [3585]), ([0], [4099]), ([256], [256]), ([4096], [3])])
U4 = ([5, 6, 7, 9], [2, 3, 4, 4], None, [([1, 1, 1, 1], [3, 4, 5, 7]), ([0, 0, 0, 0], [5, 6, 7, 9]),
                                         ([2, 3, 4, 4], [2, 3, 3, 4])])
S2 = ([24, 40], [16, 16], [4, 8], [
    ([0, 0], [24, 40]), ([16, 16], [8, 16]), ([0, 0], [16, 16]), ([3, 5], [11, 20]), ([0, 0], [24, 17]),
    ([23, 39], [1, 1]), ([0, 1], [24, 3]), ([4, 8], [4, 8]), ([5, 9], [2, 3]), ([16, 32], [8, 8]), ([2, 2], [0, 5])])
GEOMETRIES = [(a, c, l, st, sh) for a, c, l, subs in (U3, U1, U4, S2) for st, sh in subs]


@pytest.mark.parametrize("array_shape,chunk_shape,leaf_shape,start,shape", GEOMETRIES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_classifier_against_brute_force(array_shape, chunk_shape, leaf_shape, start, shape):
    from zarrs_amd import _lib as L
    got = L.store_classify(array_shape, chunk_shape, leaf_shape, start, shape)
    exp = M.classify_brute(array_shape, chunk_shape, leaf_shape or chunk_shape, start, shape)
    assert got == exp
    assert (M.UNTOUCHED, M.PARTIAL, M.COVERED) == (L.LEAF_UNTOUCHED, L.LEAF_PARTIAL, L.LEAF_COVERED)
    # a chunk that reaches past the array's edge is never covered as a whole
    grid = [-(-a // c) for a, c in zip(array_shape, chunk_shape)]
    for lin, cls in got:
        idx = np.unravel_index(lin, grid)
        if any((i + 1) * c > a for i, c, a in zip(idx, chunk_shape, array_shape)):
            assert not all(k == M.COVERED for k in cls), (lin, cls)


def test_classifier_sees_every_class():
    """The geometries above reach covered, partial and untouched leaves, and edge chunks."""
    from zarrs_amd import _lib as L
    seen = set()
    for a, c, l, st, sh in GEOMETRIES:
        for _, cls in L.store_classify(a, c, l, st, sh):
            seen |= set(cls)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("start,shape", [([0, 0], [25, 40]), ([24, 0], [1, 1]), ([0, 41], [0, 0]), ([2 ** 63, 0], [2 ** 63, 1])])
def test_classifier_refuses_subsets_outside_the_array(start, shape):
    from zarrs_amd import _lib as L
    with pytest.raises(L.ZgpuError) as e:
        L.store_classify([24, 40], [16, 16], [4, 8], start, shape)
    assert e.value.status == L.INVALID_ARGUMENT


def test_classifier_sizing_call_and_zero_volume():
    from zarrs_amd import _lib as L
    assert L.store_classify([24, 40], [16, 16], [4, 8], [3, 3], [0, 7]) == []
    n = C.c_uint64(99)
    rc = L.load().zgpu_store_classify(2, L.u64s([24, 40]), L.u64s([16, 16]), None, L.u64s([0, 0]), L.u64s([24, 40]),
                                      None, None, 0, C.byref(n))
    assert rc == 0 and n.value == 6


def test_store_entry_mirror_matches_header(tmp_path):
    """sizeof / offsetof of zgpu_store_entry as a C compiler lays it out against the ctypes mirror; the
    flag and action values against the header."""
    from zarrs_amd import _lib as L
    src = tmp_path / "entry.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n'
                   '  printf("%%zu %%zu %%zu %%zu %%zu %%zu %%u %%d %%d\\n", sizeof(zgpu_store_entry),\n'
                   '         offsetof(zgpu_store_entry, chunk), offsetof(zgpu_store_entry, action),\n'
                   '         offsetof(zgpu_store_entry, status), offsetof(zgpu_store_entry, enc),\n'
                   '         offsetof(zgpu_store_entry, enc_len), ZGPU_STORE_EMPTY_CHUNKS, ZGPU_STORE_SET,\n'
                   '         ZGPU_STORE_ERASE);\n  return 0;\n}\n' % os.path.join(ROOT, "include", "zgpu.h"))
    exe = tmp_path / "entry"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    E = L.StoreEntry
    assert got == [C.sizeof(E), E.chunk.offset, E.action.offset, E.status.offset, E.enc.offset, E.enc_len.offset,
                   L.STORE_EMPTY_CHUNKS, L.STORE_SET, L.STORE_ERASE]
    # the flag shares its word with the decode flags: no overlap
    assert L.STORE_EMPTY_CHUNKS & (L.ENC_DEVICE | L.OUT_DEVICE | L.NO_VALIDATE | L.DIRECT_IO | L.ONE_STREAM |
                                   L.COALESCE | L.ZSTD_LITS_FIRST) == 0


def test_python_surface():
    from zarrs_amd import Array, DeviceStore, FilesystemStore, MemoryStore
    from zarrs_amd import _lib as L
    for name in ("store_array_subset", "store_chunk", "erase_chunk"):
        assert callable(getattr(Array, name))
    for cls in (MemoryStore, DeviceStore, FilesystemStore):
        assert callable(cls.get) and callable(cls.set) and callable(cls.erase)
    assert {"store_decoded", "store_encoded", "store_carried"} <= set(L.last_counters())
    assert (L.CTR_STORE_DECODED, L.CTR_STORE_ENCODED, L.CTR_STORE_CARRIED) == (9, 10, 11)


def test_stores_erase_missing_key_is_no_error(tmp_path):
    from zarrs_amd import FilesystemStore, MemoryStore
    m = MemoryStore()
    m.set("c/0", b"ab")
    m.erase("c/0")
    m.erase("c/0")
    assert m.get("c/0") is None
    f = FilesystemStore(tmp_path)
    f.set("c/0/1", b"ab")
    assert f.get("c/0/1") == b"ab"
    f.erase("c/0/1")
    f.erase("c/0/1")
    f.erase("c/9/9")
    assert f.get("c/0/1") is None


# ---- the model, on cases small enough to state the answer outright ----
def test_model_unsharded_by_hand():
    m = M.StoreModel([5, 6], [4, 4], "<i4", np.int32(0).tobytes())
    r = m.store([0, 0], np.ones((4, 4), np.int32))  # one covered chunk
    assert r == {"actions": {(0, 0): "set"}, "decoded": 0, "encoded": 1, "carried": 0} and m.keys() == {(0, 0)}
    r = m.store([3, 3], np.full((2, 2), 7, np.int32))  # a corner of all four chunks; three were missing
    assert r["actions"] == {(0, 0): "set", (0, 1): "set", (1, 0): "set", (1, 1): "set"}
    assert (r["decoded"], r["encoded"]) == (1, 4)
    assert m.padded[3, 3] == 7 and m.padded[4, 4] == 7 and m.padded[0, 0] == 1 and m.padded[5, 5] == 0
    r = m.store([4, 4], np.zeros((1, 1), np.int32))  # the only non-fill element of chunk (1, 1) goes
    assert r["actions"] == {(1, 1): "erase"} and (r["decoded"], r["encoded"]) == (1, 0) and (1, 1) not in m.keys()
    r = m.store([4, 4], np.zeros((1, 1), np.int32), store_empty_chunks=True)
    assert r["actions"] == {(1, 1): "set"} and (r["decoded"], r["encoded"]) == (0, 1)
    r = m.store([0, 0], np.zeros((0, 3), np.int32))
    assert r["actions"] == {}


def test_model_sharded_by_hand():
    m = M.StoreModel([8, 8], [8, 8], "<u1", b"\0", leaf_shape=[4, 4])
    r = m.store([0, 0], np.ones((4, 4), np.uint8))
    assert r == {"actions": {(0, 0): "set"}, "decoded": 0, "encoded": 1, "carried": 0}
    r = m.store([4, 5], np.ones((1, 1), np.uint8))  # one element of inner chunk (1, 1); (0, 0) is carried
    assert (r["decoded"], r["encoded"], r["carried"]) == (0, 1, 1)
    assert m.present == {((0, 0), (0, 0)), ((0, 0), (1, 1))}
    r = m.store([0, 0], np.zeros((4, 4), np.uint8), store_empty_chunks=True)  # inner chunks are omitted all the same
    assert m.present == {((0, 0), (1, 1))} and r["actions"] == {(0, 0): "set"} and r["carried"] == 1
    r = m.store([4, 5], np.zeros((1, 1), np.uint8))
    assert r["actions"] == {(0, 0): "erase"} and m.keys() == set() and r["decoded"] == 1


def test_model_fill_is_bytewise():
    nan_a = np.frombuffer(np.uint32(0x7FC00001).tobytes(), "<f4")[0]
    assert M.is_fill(np.full(3, nan_a, "<f4"), np.uint32(0x7FC00001).tobytes())
    assert not M.is_fill(np.full(3, np.nan, "<f4"), np.uint32(0x7FC00001).tobytes())
    assert not M.is_fill(np.full(3, -0.0, "<f4"), np.float32(0.0).tobytes())
