"""A model of the write path's host layout (zarrs_amd/csrc/encode_layout.hpp), written from the rules rather
than from the C++. tests/test_encode_layout.py holds the library to it.

A case is the dictionary tests/c/encode_layout_harness.cpp reads: codecs, data_type, fill, nd, chunk_shape.
model(case) gives the layout as the harness prints it, or raises LayoutError; sizes(case) the three size queries.

The rules:
 * sizes (chain.hpp; zarrs' encoded_representation of each codec): the array->bytes codec gives nelem x
   element size (packbits: the packed bits rounded up to bytes, plus a padding byte if one is encoded); a
   checksum adds 4; gzip is zlib's deflateBound plus the gzip wrapper (gzip_codec.rs:122-136), numcodecs.zlib
   zlib's compressBound, zstd the frame overhead of 22 plus 3 per 1000 bytes begun (zstd_codec.rs:132-147),
   bz2 n + n/8 + 1024, blosc n + 16 (BLOSC_MAX_OVERHEAD); shuffle keeps the size. A chain is fixed-size when
   only checksums and shuffles follow the array->bytes codec. A shard is bounded by every inner chunk at its
   bound plus the index (sharding_codec.rs:924-945); bz2 is bounded but has no encoder.
 * refusals, in order: the array->bytes codec, a transpose of another rank, the bytes->bytes codecs in
   metadata order (a shuffle that is not first or not over the element size, bz2, an unknown blosc cname,
   blosc behind a compressor, more than 14 checksums around a compressor); for sharding_indexed: codecs around
   it, an index chain other than bytes + crc32c, rank, divisibility, then the inner chain's own.
 * fixed path: the data sits behind the checksums located at the start, 4 bytes each; every checksum covers
   the data and the checksums written before it.
 * variable path (the slot rule): a slot has 64 bytes of headroom, then room for the largest size any stage
   reaches, 4 bytes per checksum and 16 for the encoders' wide stores, rounded up to 256; two pools, the gather
   into pool 0 and each compressor into the pool the one before it did not write.
 * sharding: the shard grid, the index as a fixed-size chain over 2 x n_inner uint64; a fixed-size inner
   chain goes through temporary slots of its size rounded up to 256.
 * packbits: native elements in slots rounded up to 16 bytes, packed chunks in slots rounded up to 16,
   straight into the destinations when no bytes->bytes codec follows; the packed chunks then are 1-D uint8
   chunks through [bytes, the bytes->bytes codecs].
"""
import math

INVALID_ARGUMENT, UNSUPPORTED = 10, 6
FIXED, VAR, PACKBITS, SHARD_FIXED, SHARD_VAR = range(5)
ST = {"crc32c": 0, "gzip": 1, "zstd": 2, "blosc": 4, "numcodecs.adler32": 5, "numcodecs.fletcher32": 6,
      "numcodecs.zlib": 7}
CHECKSUMS = {"crc32c": "end", "numcodecs.adler32": "start", "numcodecs.fletcher32": "end"}  # default location
BLOSC_COMP = {"blosclz": 0, "lz4": 1, "lz4hc": 1, "snappy": 2, "zlib": 3, "zstd": 4}
BLOSC_SHUFFLE = {"noshuffle": 0, "shuffle": 1, "bitshuffle": 2}
ES = {"bool": 1, "uint8": 1, "int8": 1, "uint16": 2, "int16": 2, "float32": 4, "int32": 4, "uint32": 4, "float64": 8,
      "uint64": 8, "complex128": 16}
BOUNDS = {
    "gzip": lambda n: n + 18 + -(-n // 8) + -(-n // 64) + 5,
    "numcodecs.zlib": lambda n: n + (n >> 12) + (n >> 14) + (n >> 25) + 13,
    "zstd": lambda n: n + 22 + 3 * -(-n // 1000),
    "numcodecs.bz2": lambda n: n + n // 8 + 1024,
    "blosc": lambda n: n + 16,
}


class LayoutError(Exception):
    def __init__(self, status, why):
        super().__init__(why)
        self.status = status


def up(n, a):
    return -(-n // a) * a


def split(codecs):
    k = next(i for i, c in enumerate(codecs) if c["name"] in ("bytes", "sharding_indexed", "packbits"))
    return codecs[:k], codecs[k], codecs[k + 1:]


def cfg(c):
    return c.get("configuration") or {}


def packed_size(pb, nelem, data_type):
    bits = 1 if data_type == "bool" else 8 * ES[data_type]
    first, last = cfg(pb).get("first_bit", 0), cfg(pb).get("last_bit", bits - 1)
    return -(-nelem * (last - first + 1) // 8) + (cfg(pb).get("padding_encoding", "none") != "none")


def b2b_size(b2b, n):
    """(size after the bytes->bytes codecs or None, whether it is exact)"""
    exact = True
    for c in b2b:
        if c["name"] in CHECKSUMS:
            n += 4
        elif c["name"] in BOUNDS:
            n, exact = BOUNDS[c["name"]](n), False
        elif c["name"] != "numcodecs.shuffle":
            return None, False
    return n, exact


def sizes(case):
    """what zgpu_chain_encoded_size's and zgpu_chain_encoded_bound's C++ functions return: fixed, chain_bound, bound"""
    a2a, a2b, b2b = split(case["codecs"])
    shape, dt = case["chunk_shape"], case["data_type"]
    nelem = math.prod(shape)
    if a2b["name"] != "sharding_indexed":
        n0 = packed_size(a2b, nelem, dt) if a2b["name"] == "packbits" else nelem * ES[dt]
        n, exact = b2b_size(b2b, n0)
        n = -1 if n is None else n
        return {"fixed": n if exact else -1, "chain_bound": n, "bound": n}
    inner_shape = cfg(a2b)["chunk_shape"]
    bound = -1
    if not a2a and not b2b and len(inner_shape) == len(shape) and all(s % i == 0 for s, i in zip(shape, inner_shape)):
        n_inner = math.prod(s // i for s, i in zip(shape, inner_shape))
        _, ib, ibb = split(cfg(a2b)["codecs"])
        e = b2b_size(ibb, math.prod(inner_shape) * ES[dt])[0] if ib["name"] == "bytes" else None
        _, _, xbb = split(cfg(a2b)["index_codecs"])
        x = b2b_size(xbb, 16 * n_inner)
        bound = -1 if e is None or not x[1] else n_inner * e + x[0]
    return {"fixed": -1, "chain_bound": -1, "bound": bound}


EMPTY = {"shuffle": 0, "data_bytes": 0, "data_off": 0, "stages": [], "headroom": 0, "pitch": 0, "n_pools": 0, "fixed": 0,
         "cps": [], "n_inner": 0, "inner_n": 0, "index_at_start": 0, "index_big_endian": 0, "inner": None, "index": None,
         "native": None, "packed": None, "packed_len": 0, "upitch": 0, "ppitch": 0, "direct": 0}


def check_transposes(a2a, nd):
    for c in a2a:
        if c["name"] == "transpose" and len(cfg(c)["order"]) != nd:
            raise LayoutError(INVALID_ARGUMENT, "transpose rank")


def bytes_layout(a2a, a2b, b2b, es, shape):
    if a2b["name"] != "bytes":
        raise LayoutError(UNSUPPORTED, "array->bytes codec")
    check_transposes(a2a, len(shape))
    nelem = math.prod(shape)
    L = dict(EMPTY, es=es, nelem=nelem, data_bytes=nelem * es)
    if b2b and b2b[0]["name"] == "numcodecs.shuffle" and cfg(b2b[0]).get("elementsize", 4) == es:
        L["shuffle"], b2b = 1, b2b[1:]
    size, reached, compressors, stages = L["data_bytes"], [L["data_bytes"]], 0, []
    for c in b2b:
        name, k = c["name"], cfg(c)
        st = {"at_start": 0, "in": size, "lo": 0, "pool": 0, "level": 0, "zstd_checksum": 0, "zlib": 0, "zlib_bounded": 0,
              "blosc": [0, 0, 0, 0]}
        if name == "numcodecs.shuffle":
            raise LayoutError(UNSUPPORTED, "shuffle not innermost, or not over the element size")
        if name == "numcodecs.bz2":
            raise LayoutError(UNSUPPORTED, "bz2 is decode-only")
        if name in CHECKSUMS:
            st["at_start"] = int(k.get("location", CHECKSUMS[name]) == "start")
            size += 4
        else:
            if name == "blosc":
                if k.get("cname", "lz4") not in BLOSC_COMP:
                    raise LayoutError(UNSUPPORTED, "blosc cname")
                if compressors:
                    raise LayoutError(UNSUPPORTED, "blosc behind a compressor")
                ts = k.get("typesize") or 0
                sh = BLOSC_SHUFFLE[k["shuffle"]] if "shuffle" in k else (2 if ts else 0)  # (zarrs' default)
                st["blosc"] = [BLOSC_COMP[k.get("cname", "lz4")], sh, max(ts, 1), k.get("blocksize") or 0]
                st["level"] = k.get("clevel", 5)
            elif name == "zstd":
                st["level"], st["zstd_checksum"] = k.get("level", 0), int(bool(k.get("checksum", False)))
            else:
                st["level"] = k.get("level", 5)
                st["zlib"] = st["zlib_bounded"] = int(name == "numcodecs.zlib")
            compressors += 1
            st["pool"] = compressors % 2
            size = BOUNDS[name](size)
        st["kind"], st["out"] = ST[name], size
        reached.append(size)
        stages.append(st)
    n_sums = sum(s["kind"] in (0, 5, 6) for s in stages)
    L.update(stages=stages, size=size, fixed=int(not compressors))
    if not compressors:
        L["path"] = FIXED
        L["data_off"] = 4 * sum(s["at_start"] for s in stages)
        for j, st in enumerate(stages):  # the bytes before the data that are still free when stage j runs
            st["lo"] = 4 * sum(s["at_start"] for s in stages[j:])
    else:
        if n_sums > 14:
            raise LayoutError(UNSUPPORTED, "more than 14 checksums around a compressor")
        L.update(path=VAR, headroom=64, pitch=up(64 + max(reached) + 4 * n_sums + 16, 256), n_pools=2)
    return L


def model(case):
    a2a, a2b, b2b = split(case["codecs"])
    shape, dt = case["chunk_shape"], case["data_type"]
    es, nd, nelem = ES[dt], len(case["chunk_shape"]), math.prod(case["chunk_shape"])
    if a2b["name"] == "bytes":
        return bytes_layout(a2a, a2b, b2b, es, shape)
    if a2b["name"] == "packbits":
        check_transposes(a2a, nd)
        plen = packed_size(a2b, nelem, dt)
        native = bytes_layout(a2a, {"name": "bytes"}, [], es, shape)
        packed = bytes_layout([], {"name": "bytes"}, b2b, 1, [plen])
        return dict(EMPTY, path=PACKBITS, es=es, nelem=nelem, data_bytes=nelem * es, packed_len=plen, upitch=up(nelem * es, 16),
                    ppitch=up(plen, 16), direct=int(not b2b), native=native, packed=packed, fixed=packed["fixed"],
                    size=packed["size"])
    k = cfg(a2b)
    if a2a or b2b:
        raise LayoutError(UNSUPPORTED, "codecs around sharding_indexed")
    xa, xb, xbb = split(k["index_codecs"])
    if xa or xb["name"] != "bytes" or any(c["name"] != "crc32c" for c in xbb):
        raise LayoutError(UNSUPPORTED, "index_codecs")
    inner_shape = k["chunk_shape"]
    if len(inner_shape) != nd:
        raise LayoutError(INVALID_ARGUMENT, "rank")
    if any(s % i for s, i in zip(shape, inner_shape)):
        raise LayoutError(INVALID_ARGUMENT, "not divisible")
    cps = [s // i for s, i in zip(shape, inner_shape)]
    inner = bytes_layout(*split(k["codecs"]), es, inner_shape)
    index = bytes_layout(xa, xb, xbb, 8, [2 * math.prod(cps)])
    return dict(EMPTY, path=SHARD_FIXED if inner["fixed"] else SHARD_VAR, es=es, nelem=nelem, cps=cps, n_inner=math.prod(cps),
                inner_n=math.prod(inner_shape), index_at_start=int(k.get("index_location", "end") == "start"),
                index_big_endian=int(cfg(xb).get("endian") == "big"), inner=inner, index=index,
                pitch=up(inner["size"], 256) if inner["fixed"] else 0, size=math.prod(cps) * inner["size"] + index["size"])
