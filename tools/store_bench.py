"""Array.store_array_subset of one inner chunk of a C3-shaped shard (256^3 float32, 32^3 inner chunks of
[bytes, gzip 1, crc32c], index at the end) against the same update composed from the calls the library
had before the store path: decode the whole shard, paste on the host, zgpu_encode_pinned the whole shard
(DESIGN.md section 4). Host-resident store, both ways alternating in one run, synchronous calls timed with
the host clock, median of the repeats after warm-up.

  python tools/store_bench.py [--reps 7]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zarrs_amd import Array, Context, MemoryStore, make_desc  # noqa: E402
from zarrs_amd import _lib as L  # noqa: E402

S, I = 256, 32
CODECS = [{"name": "sharding_indexed", "configuration": {
    "chunk_shape": [I, I, I],
    "codecs": [{"name": "bytes", "configuration": {"endian": "little"}},
               {"name": "gzip", "configuration": {"level": 1}}, {"name": "crc32c"}],
    "index_codecs": [{"name": "bytes", "configuration": {"endian": "little"}}, {"name": "crc32c"}],
    "index_location": "end"}}]


def composed(arr, start, data):
    """the update by whole-shard calls: decode, paste, encode, set"""
    key = arr.chunk_key((0, 0, 0))
    shard = np.empty([S, S, S], np.float32)
    enc = np.frombuffer(arr.store[key], np.uint8)  # (zero-copy, as Array._tables passes host chunks)
    arr.codecs.decode_batch([make_desc(enc, [S, S, S])], shard, [S, S, S], enc_device=False)
    shard[tuple(slice(a, a + n) for a, n in zip(start, data.shape))] = data
    p, n, r = C.c_void_p(), C.c_uint64(), C.c_void_p()
    L.check(L.load().zgpu_encode_pinned(arr.codecs._h, 3, L.u64s([S, S, S]), shard.ctypes.data, C.byref(p),
                                        C.byref(n), C.byref(r)))
    arr.store.set(key, C.string_at(p.value, n.value))
    L.load().zgpu_result_release(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    meta = {"shape": [S, S, S], "data_type": "float32", "fill_value": 0.0, "codecs": CODECS,
            "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": [S, S, S]}}}
    arr = Array(MemoryStore(), meta, Context(0))
    rng = np.random.default_rng(0)
    base = np.cumsum(rng.standard_normal((S, S, S)).astype(np.float32), axis=2).round(1)
    arr.store_array_subset([0, 0, 0], base)
    print("shard: %.1f MiB encoded of %.0f MiB" % (len(arr.store[arr.chunk_key((0, 0, 0))]) / 2 ** 20, S ** 3 * 4 / 2 ** 20))
    for name, start, shape in (("one whole inner chunk", [32, 64, 96], [I, I, I]),
                               ("inside one inner chunk", [33, 65, 97], [30, 30, 30])):
        t = {"store_array_subset": [], "composed": []}
        for it in range(2 + args.reps):
            data = rng.standard_normal(shape).astype(np.float32)
            for how in t:
                t0 = time.perf_counter()
                if how == "composed":
                    composed(arr, start, data)
                else:
                    arr.store_array_subset(start, data)
                if it >= 2:
                    t[how].append(time.perf_counter() - t0)
            base[tuple(slice(a, a + n) for a, n in zip(start, shape))] = data
        assert np.array_equal(arr.retrieve_array_subset(), base)
        a, b =(sorted(v)[len(v) // 2] * 1e3 for v in (t["store_array_subset"], t["composed"]))
        print("%s: store_array_subset %.2f ms (min %.2f max %.2f), composed %.2f ms (min %.2f max %.2f), %.1fx" %
              (name, a, min(t["store_array_subset"]) * 1e3, max(t["store_array_subset"]) * 1e3, b,
               min(t["composed"]) * 1e3, max(t["composed"]) * 1e3, b / a))


if __name__ == "__main__":
    main()
