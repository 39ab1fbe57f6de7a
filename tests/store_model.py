"""Plain numpy model of Array.store_array_subset, written from the rules of the store path (not from
its code): a padded array that holds what every chunk decodes to (elements past the array's edge
included), and the set of leaf chunks that are present. The leaf chunk is the chunk, or the inner chunk
of a sharded array.

For every chunk of the regular grid that the subset S meets, and every leaf chunk of it:
  covered  (the leaf's whole box lies inside S)  new content = the data's part of it; old not read
  partly covered                                 new content = the old leaf (a missing one reads as
                                                 `missing`) with the overlap pasted in
  untouched (inner chunks only)                  left as it is, present or absent
A touched leaf whose new content equals the fill value bytewise in every element becomes absent (with
store_empty_chunks an unsharded chunk is stored all the same); otherwise it is present and reads back
as roundtrip(new content) (the identity unless the chain is lossy). A chunk is a key of the store iff
one of its leaves is present.

classify_brute() is the classification by brute force over element masks, for the C classifier."""
import itertools

import numpy as np

UNTOUCHED, PARTIAL, COVERED = 0, 1, 2


def classify_brute(array_shape, chunk_shape, leaf_shape, start, shape):
    """[(linear chunk index, [class per leaf, C order])] of the chunks S meets, by element masks: S is
    painted into a boolean array padded to whole chunks, and every leaf box is looked at."""
    nd = len(array_shape)
    grid = [-(-a // c) for a, c in zip(array_shape, chunk_shape)]
    mask = np.zeros([g * c for g, c in zip(grid, chunk_shape)], bool)
    mask[tuple(slice(s, s + n) for s, n in zip(start, shape))] = True
    lpc = [c // l for c, l in zip(chunk_shape, leaf_shape)]
    out = []
    for idx in itertools.product(*[range(g) for g in grid]):
        box = mask[tuple(slice(i * c, (i + 1) * c) for i, c in zip(idx, chunk_shape))]
        if not box.any():
            continue
        cls = []
        for j in itertools.product(*[range(n) for n in lpc]):
            leaf = box[tuple(slice(k * l, (k + 1) * l) for k, l in zip(j, leaf_shape))]
            cls.append(COVERED if leaf.all() else PARTIAL if leaf.any() else UNTOUCHED)
        out.append((int(np.ravel_multi_index(idx, grid)) if nd else 0, cls))
    return out


def is_fill(a, fill_bytes):
    """every element of `a` equals the fill value byte for byte"""
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).reshape(-1, len(fill_bytes))
    return bool((raw == np.frombuffer(fill_bytes, np.uint8)).all())


class StoreModel:
    def __init__(self, array_shape, chunk_shape, dtype, fill_bytes, leaf_shape=None, roundtrip=None, missing=None):
        self.array_shape, self.chunk_shape = list(array_shape), list(chunk_shape)
        self.leaf_shape = list(leaf_shape or chunk_shape)
        self.sharded = self.leaf_shape != self.chunk_shape
        self.dtype, self.fill_bytes = np.dtype(dtype), bytes(fill_bytes)
        self.grid = [-(-a // c) for a, c in zip(array_shape, chunk_shape)]
        self.lpc = [c // l for c, l in zip(self.chunk_shape, self.leaf_shape)]
        self.roundtrip = roundtrip or (lambda a: a)
        fill = np.frombuffer(self.fill_bytes, self.dtype)[0]
        self.missing = fill if missing is None else missing  # what an absent leaf reads as
        self.padded = np.full([g * c for g, c in zip(self.grid, chunk_shape)], self.missing, self.dtype)
        self.present = set()  # (chunk index tuple, leaf index tuple)

    # ---- geometry ----
    def chunks(self):
        return itertools.product(*[range(g) for g in self.grid])

    def leaves(self):
        return itertools.product(*[range(n) for n in self.lpc])

    def leaf_box(self, idx, j):
        return tuple(slice(i * c + k * l, i * c + (k + 1) * l)
                     for i, c, k, l in zip(idx, self.chunk_shape, j, self.leaf_shape))

    def chunk_box(self, idx):
        return tuple(slice(i * c, (i + 1) * c) for i, c in zip(idx, self.chunk_shape))

    def keys(self):
        return {idx for idx, _ in self.present}

    def fill_from(self, padded):
        """every leaf takes its part of `padded` (all-fill leaves stay absent), as an encoder of whole
        chunks leaves the store"""
        for idx in self.chunks():
            for j in self.leaves():
                new = padded[self.leaf_box(idx, j)]
                if self.sharded and is_fill(new, self.fill_bytes):
                    continue
                self.padded[self.leaf_box(idx, j)] = self.roundtrip(new)
                self.present.add((idx, j))

    # ---- the store ----
    def store(self, start, data, store_empty_chunks=False):
        """Apply the rules; returns {"actions": {chunk index: "set" | "erase"}, "decoded", "encoded",
        "carried"} (the counts the library reports)."""
        data = np.asarray(data)
        shape = list(data.shape)
        res = {"actions": {}, "decoded": 0, "encoded": 0, "carried": 0}
        if any(n == 0 for n in shape):
            return res
        s_lo, s_hi = list(start), [s + n for s, n in zip(start, shape)]
        for idx in self.chunks():
            c_lo = [i * c for i, c in zip(idx, self.chunk_shape)]
            if any(max(a, b) >= min(a + c, e) for a, b, c, e in zip(c_lo, s_lo, self.chunk_shape, s_hi)):
                continue
            for j in self.leaves():
                box = self.leaf_box(idx, j)
                lo = [max(b.start, a) for b, a in zip(box, s_lo)]
                hi = [min(b.stop, e) for b, e in zip(box, s_hi)]
                was = (idx, j) in self.present
                if any(a >= b for a, b in zip(lo, hi)):
                    res["carried"] += 1 if was and self.sharded else 0
                    continue
                covered = all(a == b.start and e == b.stop for a, e, b in zip(lo, hi, box))
                if covered:
                    new = data[tuple(slice(b.start - a, b.stop - a) for b, a in zip(box, s_lo))].copy()
                else:
                    new = self.padded[box].copy()
                    res["decoded"] += 1 if was else 0
                    new[tuple(slice(a - b.start, e - b.start) for a, e, b in zip(lo, hi, box))] = \
                        data[tuple(slice(a - s, e - s) for a, e, s in zip(lo, hi, s_lo))]
                if is_fill(new, self.fill_bytes) and (self.sharded or not store_empty_chunks):
                    self.present.discard((idx, j))
                    self.padded[box] = self.missing
                else:
                    self.present.add((idx, j))
                    self.padded[box] = self.roundtrip(new)
                    res["encoded"] += 1
            res["actions"][idx] = "set" if idx in self.keys() else "erase"
        return res
