"""Plain numpy model of Array.store_elements (zgpu_store_elements), written from its rules on top of
tests/store_model.py's StoreModel (the padded array of what every chunk decodes to, the set of present
leaves, the fill comparison), not from the library's code:

  data[i] becomes the element at indices[i], the points applied in order, so of several points on one
  coordinate the last one stays (update_array_bytes_indexer, zarrs_codec/src/array_bytes.rs:685-726);
  every leaf (chunk, or inner chunk of a shard) that holds a point is touched: its old content (a
  missing one reads as `missing`) takes its points, and store_model's leaf rule decides what it becomes
  -- all fill: absent (an unsharded chunk is stored all the same with store_empty_chunks), else present
  and reading back as roundtrip(new content);
  the other leaves of a touched chunk are untouched: left as they are, carried when present;
  a chunk is SET iff one of its leaves is present afterwards, else ERASEd; chunks without a touched leaf
  get no entry.

For a sharded array this is what storing the points one after another as one-element subsets gives
(test_store_points_model.py holds the model to exactly that, through StoreModel.store)."""
import numpy as np

from store_model import is_fill


def touched_leaves(m, indices):
    """{(chunk index tuple, leaf index tuple)} of the leaves the points lie in"""
    out = set()
    for p in np.asarray(indices, np.int64).reshape(-1, len(m.array_shape)):
        ci = tuple(int(x) // c for x, c in zip(p, m.chunk_shape))
        j = tuple(int(x) % c // l for x, c, l in zip(p, m.chunk_shape, m.leaf_shape))
        out.add((ci, j))
    return out


def store_elements(m, indices, data, store_empty_chunks=False):
    """Apply the points to the StoreModel m. Returns {"actions": {chunk index: "set" | "erase"},
    "decoded", "encoded", "carried", "leaves"}: the entries and the counts the library reports."""
    nd = len(m.array_shape)
    idx = np.asarray(indices, np.int64).reshape(-1, nd)
    data = np.asarray(data).reshape(-1)
    assert len(data) == len(idx)
    for p in idx:
        assert all(0 <= int(x) < a for x, a in zip(p, m.array_shape)), p
    res = {"actions": {}, "decoded": 0, "encoded": 0, "carried": 0, "leaves": 0}
    touched = touched_leaves(m, idx)
    res["leaves"] = len(touched)
    new = m.padded.copy()
    for i in range(len(idx)):  # in order: the last point on a coordinate stays
        new[tuple(int(x) for x in idx[i])] = data[i]
    for ci in sorted({c for c, _ in touched}):
        for j in m.leaves():
            was = (ci, j) in m.present
            if (ci, j) not in touched:
                res["carried"] += 1 if was and m.sharded else 0
                continue
            res["decoded"] += 1 if was else 0
            box = m.leaf_box(ci, j)
            if is_fill(new[box], m.fill_bytes) and (m.sharded or not store_empty_chunks):
                m.present.discard((ci, j))
                m.padded[box] = m.missing
            else:
                m.present.add((ci, j))
                m.padded[box] = m.roundtrip(new[box])
                res["encoded"] += 1
        res["actions"][ci] = "set" if ci in m.keys() else "erase"
    return res
