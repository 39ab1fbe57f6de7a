"""The read by coordinates on the CPU: zgpu_points_chunks (zarrs_amd/csrc/points_layout.cpp: no device behind
it) against brute force, on the geometries of test_store_model.py, and the ctypes mirror of the new flag
against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (array shape, chunk shape): test_store_model.py's U3, U1, U4 and S2
GEOMETRIES = [([20, 33, 40], [8, 16, 16]), ([4099], [256]), ([5, 6, 7, 9], [2, 3, 4, 4]), ([24, 40], [16, 16])]
IDS = ["x".join(map(str, a)) for a, _ in GEOMETRIES]


def brute(array_shape, chunk_shape, pts):
    grid = [-(-a // c) for a, c in zip(array_shape, chunk_shape)]
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, len(array_shape))
    if not len(pts):
        return []
    return np.unique(np.ravel_multi_index((pts // np.asarray(chunk_shape)).T, grid)).tolist()


def corner_points(array_shape, chunk_shape):
    """[0, ...], the array's last element, and the last valid element of an edge chunk on each axis."""
    last = [a - 1 for a in array_shape]
    pts = [[0] * len(array_shape), last]
    for d in range(len(array_shape)):
        p = [min(c - 1, a - 1) for a, c in zip(array_shape, chunk_shape)]  # last element of chunk 0 ...
        p[d] = last[d]                                                     # ... of the edge chunk on axis d
        pts.append(p)
    return pts


def raw_points_chunks(array_shape, chunk_shape, pts, cap):
    """One zgpu_points_chunks call: (status, n_chunks, the cap entries as written)."""
    from zarrs_amd import _lib as L
    nd = len(array_shape)
    idx = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, nd)
    buf = (C.c_uint64 * max(cap, 1))(*([2 ** 64 - 1] * max(cap, 1)))
    n = C.c_uint64(2 ** 64 - 1)
    rc = L.load().zgpu_points_chunks(nd, L.u64s(array_shape), L.u64s(chunk_shape), idx.ctypes.data, idx.shape[0],
                                     buf if cap else None, cap, C.byref(n))
    return rc, n.value, list(buf)[:cap]


@pytest.mark.parametrize("array_shape,chunk_shape", GEOMETRIES, ids=IDS)
def test_points_chunks_against_brute_force(array_shape, chunk_shape):
    from zarrs_amd import _lib as L
    rng = np.random.default_rng(len(array_shape))
    for n in (1, 2, 63, 64, 65, 257, 3000):
        pts = np.stack([rng.integers(0, a, size=n) for a in array_shape], axis=1)
        pts[: n // 3] = pts[n // 3: 2 * (n // 3)][::-1][: n // 3]  # duplicates
        got = L.points_chunks(array_shape, chunk_shape, pts)
        assert got == brute(array_shape, chunk_shape, pts), n
        assert got == sorted(set(got))
    # a few points touch a few chunks only; every point of the array touches every chunk
    grid = [-(-a // c) for a, c in zip(array_shape, chunk_shape)]
    every = np.stack(np.meshgrid(*[np.arange(a) for a in array_shape], indexing="ij"), axis=-1).reshape(-1, len(grid))
    assert L.points_chunks(array_shape, chunk_shape, every) == list(range(int(np.prod(grid))))


@pytest.mark.parametrize("array_shape,chunk_shape", GEOMETRIES, ids=IDS)
def test_points_chunks_corners_and_duplicates(array_shape, chunk_shape):
    from zarrs_amd import _lib as L
    grid = [-(-a // c) for a, c in zip(array_shape, chunk_shape)]
    pts = corner_points(array_shape, chunk_shape)
    got = L.points_chunks(array_shape, chunk_shape, pts)
    assert got == brute(array_shape, chunk_shape, pts)
    assert got[0] == 0 and got[-1] == int(np.prod(grid)) - 1  # the first and the last chunk of the grid
    # the same point many times is one chunk
    assert L.points_chunks(array_shape, chunk_shape, [pts[1]] * 100) == [int(np.prod(grid)) - 1]
    assert L.points_chunks(array_shape, chunk_shape, pts + pts[::-1]) == got


def test_points_chunks_no_points():
    from zarrs_amd import _lib as L
    for array_shape, chunk_shape in GEOMETRIES:
        assert L.points_chunks(array_shape, chunk_shape, np.zeros((0, len(array_shape)), np.uint64)) == []
    lib = L.load()
    n = C.c_uint64(7)
    assert lib.zgpu_points_chunks(2, L.u64s([24, 40]), L.u64s([16, 16]), None, 0, None, 0, C.byref(n)) == L.OK
    assert n.value == 0


def test_points_chunks_sizing_convention():
    """cap 0 sizes the array; a cap below the count writes the first cap entries only, and still counts."""
    from zarrs_amd import _lib as L
    a, c = [20, 33, 40], [8, 16, 16]
    pts = corner_points(a, c) + [[9, 17, 20], [9, 17, 21]]
    exp = brute(a, c, pts)
    assert len(exp) >= 4
    rc, n, got = raw_points_chunks(a, c, pts, 0)
    assert (rc, n, got) == (L.OK, len(exp), [])
    rc, n, got = raw_points_chunks(a, c, pts, 2)
    assert (rc, n, got) == (L.OK, len(exp), exp[:2])
    rc, n, got = raw_points_chunks(a, c, pts, len(exp) + 3)
    assert (rc, n) == (L.OK, len(exp)) and got[:len(exp)] == exp
    assert got[len(exp):] == [2 ** 64 - 1] * 3  # nothing written past the count


OOB = [(a, c, d, where) for a, c in GEOMETRIES for d in range(len(a)) for where in ("first", "last")]


@pytest.mark.parametrize("array_shape,chunk_shape,axis,where", OOB,
                         ids=["x".join(map(str, a)) + f"-axis{d}-{w}" for a, _, d, w in OOB])
def test_points_chunks_refuses_out_of_bounds_points(array_shape, chunk_shape, axis, where):
    from zarrs_amd import _lib as L
    rng = np.random.default_rng(5)
    n = 40
    pts = np.stack([rng.integers(0, a, size=n) for a in array_shape], axis=1).astype(np.uint64)
    at = 0 if where == "first" else n - 1
    for bad in (array_shape[axis], array_shape[axis] + 1, 2 ** 63, 2 ** 64 - 1):
        p = pts.copy()
        p[at, axis] = bad
        with pytest.raises(L.ZgpuError) as e:
            L.points_chunks(array_shape, chunk_shape, p)
        assert e.value.status == L.INVALID_ARGUMENT
        msg = str(e.value)
        assert f"point {at} " in msg and f"axis {axis}" in msg, msg
        assert raw_points_chunks(array_shape, chunk_shape, p, 0)[0] == L.INVALID_ARGUMENT
    # two offending points: the first one is named
    if n > 2:
        p = pts.copy()
        p[at, axis] = array_shape[axis]
        p[n // 2, axis] = array_shape[axis]
        with pytest.raises(L.ZgpuError) as e:
            L.points_chunks(array_shape, chunk_shape, p)
        assert f"point {min(at, n // 2)} " in str(e.value)


def test_points_chunks_refuses_bad_geometry():
    from zarrs_amd import _lib as L
    lib = L.load()
    n = C.c_uint64()
    pts = np.zeros((1, 2), np.uint64)
    assert lib.zgpu_points_chunks(2, L.u64s([24, 40]), L.u64s([16, 0]), pts.ctypes.data, 1, None, 0,
                                  C.byref(n)) == L.INVALID_ARGUMENT
    assert lib.zgpu_points_chunks(0, L.u64s([24, 40]), L.u64s([16, 16]), pts.ctypes.data, 1, None, 0,
                                  C.byref(n)) == L.INVALID_ARGUMENT
    assert lib.zgpu_points_chunks(2, L.u64s([24, 40]), L.u64s([16, 16]), pts.ctypes.data, 1, None, 0,
                                  None) == L.INVALID_ARGUMENT


WIDE = [  # (array shape, chunk shape, leaf shape, leaves, 64-bit indexing)
    ([20, 33, 40], [8, 16, 16], None, 27, False),
    ([24, 40], [16, 16], [4, 8], 8 * 6, False),
    ([2 ** 32 - 1], [256], None, 2 ** 24, False),
    ([2 ** 32], [256], None, 2 ** 24, True),                 # an extent of the array
    ([2 ** 33 + 5, 6], [2 ** 20, 4], None, 8193 * 2, True),
    ([100], [2 ** 32], None, 1, True),                       # a chunk extent over a smaller array
    ([100], [2 ** 32 + 7], None, 1, True),
    ([100, 100], [2 ** 33, 64], [2 ** 32, 64], 2 * 2, True),  # an inner-chunk extent
    ([100, 100], [2 ** 33, 64], [2 ** 31, 64], 4 * 2, False),
    ([2 ** 20, 2 ** 20], [16, 16], None, 2 ** 32, True),      # the number of leaves alone
    ([2 ** 20, 2 ** 20 - 16], [16, 16], None, 2 ** 32 - 2 ** 16, False),
]


@pytest.mark.parametrize("array_shape,chunk_shape,leaf_shape,leaves,wide", WIDE,
                         ids=[f"{a}-{c}-{l}".replace(" ", "") for a, c, l, _, _ in WIDE])
def test_geometry_decides_the_index_width(array_shape, chunk_shape, leaf_shape, leaves, wide):
    """The kernels divide coordinates below array_shape by leaf_shape and form keys below the number of
    leaves: 32-bit arithmetic is taken only when all three fit."""
    from zarrs_amd import _lib as L
    assert L.points_geometry(array_shape, chunk_shape, leaf_shape) == (leaves, wide)
    fits = all(a <= 2 ** 32 - 1 for a in array_shape) and leaves <= 2 ** 32 - 1 and \
        all(v <= 2 ** 32 - 1 for v in (leaf_shape or chunk_shape))
    assert wide == (not fits)


def test_geometry_refuses():
    from zarrs_amd import _lib as L
    for a, c, l in (([24, 40], [16, 0], None), ([24, 40], [16, 16], [4, 0]), ([24, 40], [16, 16], [5, 8]),
                    ([2 ** 40, 2 ** 40], [1, 1], None)):
        with pytest.raises(L.ZgpuError) as e:
            L.points_geometry(a, c, l)
        assert e.value.status == L.INVALID_ARGUMENT


def test_mirror_follows_the_header():
    """The flag, the bitmap limit and the new counters of the ctypes mirror are the header's."""
    from zarrs_amd import _lib as L
    txt = open(os.path.join(ROOT, "include", "zgpu.h")).read()
    assert int(re.search(r"#define ZGPU_IDX_DEVICE (0x[0-9a-f]+)u", txt).group(1), 16) == L.IDX_DEVICE
    flags = {k: int(v, 16) for k, v in re.findall(r"#define (ZGPU_[A-Z_]+) (0x[0-9a-f]+)u", txt)}
    assert [k for k, v in flags.items() if v == L.IDX_DEVICE] == ["ZGPU_IDX_DEVICE"]  # a bit of its own
    m = re.search(r"#define ZGPU_POINTS_BITMAP_MAX_BYTES \((\d+)u << (\d+)\)", txt)
    assert int(m.group(1)) << int(m.group(2)) == L.POINTS_BITMAP_MAX_BYTES
    assert {"point_leaves", "point_rounds"} <= set(L.last_counters())
    assert (L.CTR_POINT_LEAVES, L.CTR_POINT_ROUNDS) == (12, 13)
