"""tests/store_points_model.py (the numpy model of Array.store_elements) held to brute force: the same
points fed one at a time, in order, through store_model.StoreModel.store as one-element boxes -- what
zarrs gives for a sharded array, where its partial encoder has no path for a list of coordinates. No
GPU, no library: this pins the checker tests/test_gpu_store_points.py uses, on that file's shapes."""
import copy

import numpy as np
import pytest

import store_model as M
import store_points_model as PM

F4, U1, C16 = np.dtype("<f4"), np.dtype("u1"), np.dtype("<c16")


def fill_of(dtype, v=0):
    return np.asarray([v], dtype).tobytes()


def seeded(array_shape, chunk_shape, dtype, fill, leaf_shape=None, seed=1, holes=(), missing=()):
    m = M.StoreModel(array_shape, chunk_shape, dtype, fill, leaf_shape)
    rng = np.random.default_rng(seed)
    raw = rng.integers(1, 200, m.padded.shape).astype(dtype)
    for box in holes:
        raw[box] = np.frombuffer(fill, dtype)[0]
    for idx in missing:
        raw[m.chunk_box(idx)] = np.frombuffer(fill, dtype)[0]
    m.fill_from(raw)
    if not m.sharded:  # (fill_from keeps an unsharded all-fill chunk present: a missing key is made here)
        for idx in missing:
            m.present.discard((idx, tuple([0] * len(array_shape))))
    return m


def brute(m, pts, data, store_empty_chunks=False):
    """the points one after another as 1-element subsets; the last action of every chunk"""
    actions = {}
    for p, v in zip(pts, data):
        r = m.store([int(x) for x in p], np.asarray(v, m.dtype).reshape([1] * len(p)), store_empty_chunks)
        actions.update(r["actions"])
    return actions


def check(m, pts, data, store_empty_chunks=False):
    pts = np.asarray(pts, np.int64).reshape(len(data), -1)
    b = copy.deepcopy(m)
    before = set(m.present)
    touched = PM.touched_leaves(m, pts)
    r = PM.store_elements(m, pts, data, store_empty_chunks)
    want = brute(b, pts, data, store_empty_chunks)
    assert r["actions"] == want
    assert m.present == b.present
    assert m.padded.tobytes() == b.padded.tobytes()
    # the counts, from the two states
    chunks = {c for c, _ in touched}
    assert r["leaves"] == len(touched) and set(r["actions"]) == chunks
    assert r["decoded"] == len(touched & before)
    kept = store_empty_chunks and not m.sharded
    assert r["encoded"] == len([t for t in touched if t in m.present or kept])
    assert r["carried"] == (len([t for t in before if t[0] in chunks and t not in touched]) if m.sharded else 0)
    return r


def scattered(m, n, seed, chunks):
    """n points inside the array, in the given chunks only, the last tenth repeating the first"""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n:
        c = chunks[int(rng.integers(len(chunks)))]
        p = [i * s + int(rng.integers(s)) for i, s in zip(c, m.chunk_shape)]
        if all(x < a for x, a in zip(p, m.array_shape)):
            pts.append(p)
    pts = np.asarray(pts, np.int64)
    pts[n - n // 10:] = pts[:n // 10]
    return pts


@pytest.mark.parametrize("dtype", [U1, F4, C16], ids=str)
def test_unsharded_edge_chunks(dtype):
    fill = fill_of(dtype, 3)
    m = seeded([10, 13], [4, 5], dtype, fill, missing=[(1, 1)])
    assert (1, 1) not in m.keys() and (0, 0) in m.keys()
    pts = np.concatenate([scattered(m, 39, 5, [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 1)]), [[9, 12]]])
    data = np.arange(1, 41).astype(dtype)
    r = check(m, pts, data)
    assert (0, 2) not in r["actions"] and (2, 0) not in r["actions"] and r["actions"][(2, 2)] == "set"
    assert r["actions"][(1, 1)] == "set" and r["decoded"] == len(r["actions"]) - 1
    assert m.padded[9, 12] == data[39]


def test_last_point_wins():
    m = seeded([8, 8], [8, 8], F4, fill_of(F4))
    pts = [[1, 1], [3, 4], [1, 1], [7, 7], [1, 1], [3, 4]]
    check(m, pts, np.asarray([10, 20, 30, 40, 50, 60], F4))
    assert m.padded[1, 1] == 50 and m.padded[3, 4] == 60 and m.padded[7, 7] == 40
    # many claimants per element
    n = 2000
    m = seeded([8, 8], [8, 8], F4, fill_of(F4))
    pts = np.stack([np.arange(n) % 64 // 8, np.arange(n) % 8], axis=1)
    check(m, pts, np.arange(n).astype(F4))
    assert np.array_equal(m.padded.reshape(-1), np.arange(n - 64, n).astype(F4)[np.argsort(np.arange(n - 64, n) % 64)])


def test_permutation_1d():
    for dtype in (U1, np.dtype("<i2")):
        m = seeded([64], [64], dtype, fill_of(dtype))
        perm = np.random.default_rng(2).permutation(64)
        check(m, perm.reshape(-1, 1), (perm + 100).astype(dtype))
        assert np.array_equal(m.padded, (np.arange(64) + 100).astype(dtype))


@pytest.mark.parametrize("store_empty", [False, True])
def test_sharded(store_empty):
    fill = fill_of(F4)
    holes = [(slice(4, 8), slice(0, 4))]  # an absent inner chunk of shard (0, 0)
    m = seeded([16, 16], [8, 8], F4, fill, [4, 4], holes=holes, missing=[(1, 1)])
    assert ((0, 0), (1, 0)) not in m.present and (1, 1) not in m.keys()
    # three inner chunks of shard (0, 0) (one of them the absent one), one of shard (1, 1), which is missing
    pts = [[0, 0], [1, 2], [5, 1], [3, 7], [0, 0], [13, 13], [5, 1]]
    r = check(m, pts, np.asarray([1, 2, 3, 4, 5, 6, 7], F4), store_empty)
    assert r["actions"] == {(0, 0): "set", (1, 1): "set"} and r["leaves"] == 4
    assert r["decoded"] == 2 and r["encoded"] == 4 and r["carried"] == 1
    # fill values over everything an inner chunk holds: it goes; over a missing shard: erased
    m2 = M.StoreModel([16, 16], [8, 8], F4, fill, [4, 4])
    PM.store_elements(m2, [[9, 1], [9, 2]], np.asarray([5, 6], F4))
    r = check(m2, [[9, 1], [9, 2], [0, 9]], np.zeros(3, F4), store_empty)
    assert r["actions"] == {(1, 0): "erase", (0, 1): "erase"} and not m2.present


@pytest.mark.parametrize("store_empty", [False, True])
def test_unsharded_erase(store_empty):
    fill = fill_of(F4, 2.5)
    m = M.StoreModel([10, 13], [4, 5], F4, fill)
    PM.store_elements(m, [[0, 0], [1, 1]], np.asarray([1, 2], F4))
    assert m.keys() == {(0, 0)}
    want = "set" if store_empty else "erase"
    r = check(m, [[1, 1], [0, 0], [9, 12]], np.full(3, 2.5, F4), store_empty)
    assert r["actions"] == {(0, 0): want, (2, 2): want}
    assert m.keys() == ({(0, 0), (2, 2)} if store_empty else set())


def test_out_of_bounds_is_the_models_assertion():
    m = M.StoreModel([10, 13], [4, 5], F4, fill_of(F4))
    with pytest.raises(AssertionError):
        PM.store_elements(m, [[0, 0], [10, 0]], np.ones(2, F4))
