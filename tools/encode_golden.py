"""The write path's golden cases: small seeded arrays through zgpu_encode_chunks (and one
zgpu_store_array_subset), recorded as the encoded length and the SHA-256 of every encoded chunk.
tests/test_gpu_encode_golden.py rebuilds the same inputs and compares with tests/golden/encode_digests.json,
which holds this script's output at the commit before the write path got its host layout (encode_layout.cpp):
a refactor of the host side must not move one encoded byte. The file is recorded, never regenerated from the
code under test.

  python tools/encode_golden.py OUT.json
"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BYTES = {"name": "bytes", "configuration": {"endian": "little"}}
BIG = {"name": "bytes", "configuration": {"endian": "big"}}
CRC = {"name": "crc32c"}
CRC_START = {"name": "crc32c", "configuration": {"location": "start"}}
GZIP = {"name": "gzip", "configuration": {"level": 1}}
ZLIB = {"name": "numcodecs.zlib", "configuration": {"level": 1}}
ZSTD = {"name": "zstd", "configuration": {"level": 3, "checksum": True}}
SHUFFLE4 = {"name": "numcodecs.shuffle", "configuration": {"elementsize": 4}}
FSO = {"name": "numcodecs.fixedscaleoffset", "configuration": {"offset": 0, "scale": 10, "dtype": "f4", "astype": "i2"}}
PACKBITS = {"name": "packbits", "configuration": {"first_bit": 1, "last_bit": 5}}


def blosc(cname, shuffle="shuffle", typesize=4):
    return {"name": "blosc", "configuration": {"cname": cname, "clevel": 5, "shuffle": shuffle, "typesize": typesize,
                                               "blocksize": 0}}


def tr(*order):
    return {"name": "transpose", "configuration": {"order": list(order)}}


def shard(inner, location, index):
    return {"name": "sharding_indexed", "configuration": {"chunk_shape": [4, 4], "codecs": inner, "index_codecs": index,
                                                          "index_location": location}}


F32 = ("float32", [12, 10], [8, 6])      # edge chunks take fill
SH = ("float32", [12, 10], [8, 8])       # [8, 8] shards of [4, 4] inner chunks, some wholly past the edge
U8 = ("uint8", [70000], [70000])         # one 1-D chunk past the encoders' small-size terms
PB = ("uint8", [12, 10], [8, 6])
# name -> (codecs, (data type, array shape, chunk shape), fill value)
ENCODE_CASES = {
    "fixed_tr_crc_both_ends": ([tr(1, 0), BIG, CRC_START, CRC], F32, 2.5),
    "fixed_shuffle_crc": ([BYTES, SHUFFLE4, CRC], F32, 2.5),
    "gzip": ([BYTES, GZIP], F32, 2.5),
    "zlib": ([BYTES, ZLIB], F32, 2.5),
    "zstd": ([BYTES, ZSTD], F32, 2.5),
    "blosc_lz4_shuffle": ([BYTES, blosc("lz4")], F32, 2.5),
    "blosc_blosclz": ([BYTES, blosc("blosclz", "noshuffle")], F32, 2.5),
    "blosc_zstd_bitshuffle": ([BYTES, blosc("zstd", "bitshuffle")], F32, 2.5),
    "gzip_crc_zstd": ([BYTES, GZIP, CRC, ZSTD], F32, 2.5),
    "u8_70000_gzip": ([BYTES, GZIP], U8, 0),
    "u8_70000_zlib_crc": ([BYTES, ZLIB, CRC], U8, 0),
    "u8_70000_zstd": ([BYTES, ZSTD], U8, 0),
    "u8_70000_blosc_lz4": ([BYTES, blosc("lz4", "noshuffle", 1)], U8, 0),
    "packbits_direct": ([PACKBITS], PB, 0),
    "packbits_gzip": ([PACKBITS, GZIP], PB, 0),
    "packbits_crc": ([PACKBITS, CRC_START], PB, 0),
    "value_fso_gzip": ([FSO, BYTES, GZIP], F32, 0.0),
    "value_fso_crc": ([FSO, tr(1, 0), BYTES, CRC], F32, 0.0),
    "sharded_fixed_index_start": ([shard([BYTES, CRC], "start", [BYTES, CRC])], SH, 2.5),
    "sharded_fixed_index_end_two_crc": ([shard([tr(1, 0), BIG], "end", [BIG, CRC_START, CRC])], SH, 2.5),
    "sharded_gzip_index_start": ([shard([BYTES, GZIP, CRC], "start", [BYTES, CRC])], SH, 2.5),
    "sharded_gzip_index_end_no_crc": ([shard([BYTES, GZIP], "end", [BYTES])], SH, 2.5),
}
# one zgpu_store_array_subset over a sharded array: inner chunk (1, 0) of shard (0, 0) is partly covered and
# encoded again, the shard's other inner chunks are carried over
STORE_CASES = {
    "store_sharded_fixed": [shard([BYTES, CRC], "end", [BYTES, CRC])],
    "store_sharded_gzip": [shard([BYTES, GZIP], "start", [BYTES, CRC])],
}
# the chains that are the same bytes on every run by construction: their digests must be recorded
DETERMINISTIC = ("fixed_tr_crc_both_ends", "fixed_shuffle_crc", "packbits_direct", "packbits_crc", "value_fso_crc",
                 "sharded_fixed_index_start", "sharded_fixed_index_end_two_crc", "store_sharded_fixed")


def make_array(dt, shape, seed):
    """compressible, seeded: a rounded random walk (float32), small values with runs (uint8)"""
    rng = np.random.default_rng(seed)
    if dt == "float32":
        return np.cumsum(rng.standard_normal(shape), axis=-1).round(1).astype(np.float32) + np.float32(3)
    return np.repeat(rng.integers(0, 64, (int(np.prod(shape)) + 2) // 3, dtype=np.uint8), 3)[:int(np.prod(shape))].reshape(shape)


def chunk_starts(shape, chunk):
    grid = [-(-s // c) for s, c in zip(shape, chunk)]
    return [[i * c for i, c in zip(idx, chunk)] for idx in np.ndindex(*grid)]


def digest(chunks):
    return {"lens": [len(c) for c in chunks], "sha256": [hashlib.sha256(c).hexdigest() for c in chunks]}


def encode_case(ctx, torch, name):
    """the encoded chunks of one case, as bytes, in chunk-grid order"""
    from zarrs_amd import CodecChain
    codecs, (dt, shape, chunk), fill = ENCODE_CASES[name]
    a = make_array(dt, shape, sorted(ENCODE_CASES).index(name))
    ch = CodecChain.from_metadata(codecs, dt, fill, ctx)
    enc = ch.encode_chunks(torch.from_numpy(a).cuda(), chunk, chunk_starts(shape, chunk))
    return [bytes(e.cpu().numpy()) for e in enc]


def store_case(ctx, name):
    """the shards after a whole-array store and after the partial store, as bytes"""
    from zarrs_amd import Array, MemoryStore
    dt, shape, chunk = SH
    meta = {"shape": shape, "data_type": dt, "fill_value": 2.5, "codecs": STORE_CASES[name],
            "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": chunk}}}
    arr = Array(MemoryStore(), meta, ctx)
    arr.store_array_subset([0, 0], make_array(dt, shape, 100))
    arr.store_array_subset([5, 1], make_array(dt, [2, 2], 101))
    from zarrs_amd import _lib as L
    ctr = L.last_counters()
    assert (ctr["store_decoded"], ctr["store_encoded"], ctr["store_carried"]) == (1, 1, 3), ctr
    return [bytes(arr.store[arr.chunk_key(idx)]) for idx in np.ndindex(*arr.chunk_grid_shape())]


def run_all(ctx, torch):
    out = {name: digest(encode_case(ctx, torch, name)) for name in ENCODE_CASES}
    out.update({name: digest(store_case(ctx, name)) for name in STORE_CASES})
    return out


if __name__ == "__main__":
    import torch
    from zarrs_amd import Context
    with open(sys.argv[1], "w") as f:
        json.dump(run_all(Context(0), torch), f, indent=1, sort_keys=True)
        f.write("\n")
