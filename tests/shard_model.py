"""The sharding_indexed layer (the shard index, what an entry means, which entries a read looks at) as a
plain Python model, a builder of shards no writer of this project lays out, and the table of cases made
with them. numpy and pure Python; no GPU, no oracle.

Written from the Zarr v3 sharding specification and the zarrs lines that fix what the specification
leaves open (zarrs/src/array/codec/array_to_bytes/sharding/):
  sharding_codec.rs:424-439, 680-690  an entry is empty only when BOTH words are 2^64-1; any other entry
                                      with offset + size > len(shard) is out of bounds
  sharding_codec.rs:1262-1298         the index is the first / last index_bytes bytes of the shard, a
                                      shorter shard is an error; the index chain is decoded whole
                                      (bytes->bytes codecs in reverse, checksums verified)
  sharding_partial_decoder_sync.rs:290-370  a partial read decodes the index, then looks only at the
                                      entries of the inner chunks its selection meets
Offsets are absolute in the shard wherever the index lies; entries are in C order of the inner grid; the
first failing inner chunk in C order gives the shard's status (try_for_each, sharding_codec.rs:702-704).
offset + size is computed by zarrs in u64 and overflows for offset = 2^64-2, size = 4 (a panic in a debug
build, a wrapped sum in a release build); the model defines a wrapped sum as SHARD_INDEX_OOB.

Inner chunks are encoded by independent means: `bytes` and transposes by numpy, crc32c by the bytewise
table below, gzip by Python's zlib, zstd by libzstd through ctypes (zstd_frames.libzstd). The expected
decode of any selection is the slice of the numpy array the shard was built from, the fill value where
an entry is empty or the shard is missing.

test_shard_model.py holds the model to the reference's own sharded fixture and the C oracle to the model;
test_gpu_shards.py holds every reader of the library to the model.
"""
from __future__ import annotations

import dataclasses
import functools
import itertools
import struct
import zlib
from dataclasses import dataclass

import numpy as np

import zstd_frames as ZF
from scatter_cases import TYPES, fill_bytes

MAX = 2 ** 64 - 1
OK, INVALID_CHECKSUM, DECODED_SIZE_MISMATCH, SHARD_INDEX_OOB, CORRUPT_STREAM = 0, 1, 2, 3, 4
UNSUPPORTED, CRC_INPUT_TOO_SHORT, SHARD_TOO_SMALL = 6, 7, 8


# ---------------------------------------------------------------------------------------------------
# crc32c (Castagnoli, reflected 0x82F63B78), one byte at a time
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _crc_table():
    t = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        t.append(c)
    return t


def crc32c(data: bytes) -> int:
    t, c = _crc_table(), 0xFFFFFFFF
    for b in bytes(data):
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def junk(n: int, salt: int = 0) -> bytes:
    """n bytes, none of them zero"""
    return bytes((salt * 7 + i * 37) % 255 + 1 for i in range(n))


# ---------------------------------------------------------------------------------------------------
# the index
# ---------------------------------------------------------------------------------------------------
def index_bytes(n_inner: int, crcs) -> int:
    return 16 * n_inner + 4 * len(crcs)


def pack_index(entries, endian: str, crcs) -> bytes:
    """entries: (offset, size) per inner chunk, C order. crcs: the `location` of every crc32c codec after
    the index's `bytes` codec, in codec order (the order they encode in)."""
    fmt = (">" if endian == "big" else "<") + "Q"
    data = b"".join(struct.pack(fmt, w) for e in entries for w in e)
    for loc in crcs:
        c = struct.pack("<I", crc32c(data))
        data = c + data if loc == "start" else data + c
    return data


def crc_positions(n_inner: int, crcs) -> list:
    """the byte position in the encoded index of every stored checksum, in codec order"""
    pos, n = [], 16 * n_inner
    for loc in crcs:
        if loc == "start":
            pos = [p + 4 for p in pos] + [0]
        else:
            pos.append(n)
        n += 4
    return pos


def parse_index(raw: bytes, n_inner: int, endian: str, crcs, validate: bool = True):
    """[(offset, size)] or a status. The checksums decode in reverse codec order."""
    data = bytes(raw)
    for loc in reversed(crcs):
        if len(data) < 4:
            return CRC_INPUT_TOO_SHORT
        stored, data = (data[:4], data[4:]) if loc == "start" else (data[-4:], data[:-4])
        if validate and struct.pack("<I", crc32c(data)) != stored:
            return INVALID_CHECKSUM
    assert len(data) == 16 * n_inner
    w = struct.unpack((">" if endian == "big" else "<") + "%dQ" % (2 * n_inner), data)
    return [(w[2 * k], w[2 * k + 1]) for k in range(n_inner)]


# ---------------------------------------------------------------------------------------------------
# inner chains
# ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Chain:
    """transpose? + bytes{endian} + bytes->bytes codecs ("gzip", "zstd", "crc32c" = at the end,
    "crc32c_start")"""
    name: str
    endian: str = "little"
    order: tuple | None = None
    b2b: tuple = ()

    def codecs(self) -> list:
        m = [{"name": "transpose", "configuration": {"order": list(self.order)}}] if self.order else []
        m.append({"name": "bytes", "configuration": {"endian": self.endian}})
        for k in self.b2b:
            if k == "gzip":
                m.append({"name": "gzip", "configuration": {"level": 1}})
            elif k == "zstd":
                m.append({"name": "zstd", "configuration": {"level": 1, "checksum": False}})
            else:
                m.append({"name": "crc32c", "configuration": {"location": "start" if k.endswith("start") else "end"}})
        return m

    # The status of a present entry of size 0, the inner chain's own for zero bytes (the
    # status table): the last bytes->bytes codec sees them first. crc32c: "crc32c decoder expects a 32 bit
    # input" (crc32c_codec.rs:137); gzip: flate2 reads no header, an io::Error (gzip_codec.rs:116-118);
    # zstd: zstd::bulk::decompress of nothing is nothing (zstd_codec.rs:119-123), so `bytes` gets 0 bytes
    # for a chunk that needs more: UnexpectedChunkDecodedSize (array_bytes.rs:376-386), as for bare `bytes`.
    def zero_status(self) -> int:
        last = self.b2b[-1] if self.b2b else None
        if last is None or last == "zstd":
            return DECODED_SIZE_MISMATCH
        return CORRUPT_STREAM if last == "gzip" else CRC_INPUT_TOO_SHORT


LE = Chain("bytes_le")
BE = Chain("bytes_be", endian="big")
LE_CRC = Chain("bytes_crc", b2b=("crc32c",))
TR_BE = Chain("transpose_bytes", endian="big", order=(1, 0))
GZ_CRC = Chain("bytes_gzip_crc", b2b=("gzip", "crc32c"))  # the C3 inner chain
ZSTD = Chain("bytes_zstd", b2b=("zstd",))
CHAINS = [LE, BE, LE_CRC, TR_BE, GZ_CRC, ZSTD]


def np_dtype(dt: str):
    return np.dtype(TYPES[dt][0])


def encode_inner(chain: Chain, a: np.ndarray) -> bytes:
    t = np.ascontiguousarray(np.transpose(a, chain.order) if chain.order else a)
    data = (t.byteswap() if chain.endian == "big" else t).tobytes()  # bytes moved, values never touched
    for k in chain.b2b:
        if k == "gzip":
            z = zlib.compressobj(1, zlib.DEFLATED, 31)
            data = z.compress(data) + z.flush()
        elif k == "zstd":
            data = ZF.stream_frame(data, 0, level=1)
        else:
            c = struct.pack("<I", crc32c(data))
            data = c + data if k.endswith("start") else data + c
    return data


def decode_inner(chain: Chain, data: bytes, shape, dt: str, validate: bool, partial: bool):
    """(status, array). A partial read strips a crc32c unverified (the partial decoder of crc32c,
    strip_suffix_partial_decoder.rs)."""
    nbytes = int(np.prod(shape)) * TYPES[dt][1]
    for k in reversed(chain.b2b):
        if k == "gzip":
            try:
                z = zlib.decompressobj(31)
                data = z.decompress(data)
                if not z.eof:  # truncated, or no stream at all
                    return CORRUPT_STREAM, None
            except zlib.error:
                return CORRUPT_STREAM, None
        elif k == "zstd":
            try:
                data = ZF.zstd_decompress(data, nbytes + 64) if data else b""
            except RuntimeError:
                return CORRUPT_STREAM, None
        else:
            if len(data) < 4:
                return CRC_INPUT_TOO_SHORT, None
            stored, data = (data[:4], data[4:]) if k.endswith("start") else (data[-4:], data[:-4])
            if validate and not partial and struct.pack("<I", crc32c(data)) != stored:
                return INVALID_CHECKSUM, None
    if len(data) != nbytes:
        return DECODED_SIZE_MISMATCH, None
    enc_shape = [shape[i] for i in chain.order] if chain.order else list(shape)
    t = np.frombuffer(data, np_dtype(dt)).reshape(enc_shape)
    t = t.byteswap() if chain.endian == "big" else t
    return OK, (np.transpose(t, np.argsort(chain.order)) if chain.order else t)


# ---------------------------------------------------------------------------------------------------
# shards
# ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Layout:
    """Where the encoded inner chunks lie in the shard. order: the storage order of the stored inner
    chunks (C-order inner indices; None: C order). pre / gap / post: junk bytes before the first, between
    two, and after the last stored inner chunk (so, with the index at the end, before the index). alias
    {k: j}: entry k names entry j's range (their contents are made equal). overlap (a, b): b's range
    starts half-way into a's (the second half of a is made equal to the first half of b). selfref {k: off}:
    entry k names the absolute range [off, off + its size), wherever that lies (inside the index)."""
    order: tuple | None = None
    pre: int = 0
    gap: int = 0
    post: int = 0
    alias: tuple = ()
    overlap: tuple | None = None
    selfref: tuple = ()


CANON = Layout()


@dataclass(frozen=True)
class Shard:
    """One sharding_indexed codec and how the shards of a case are laid out. empty: inner chunks with an
    empty entry. patch {k: f(len, offset, size) -> (offset, size)}: entries rewritten after the layout is
    fixed (len: the shard's length). flip: bytes flipped after everything else: ("crc", i) the i-th
    stored index checksum, ("inner", k) a byte in the middle of inner chunk k's range. cut: the shard is
    replaced by `cut` junk bytes. only: for a nested shard, the parent's inner chunks that patch / flip /
    empty apply to (None: all)."""
    inner_shape: tuple
    chain: object  # Chain | Shard
    location: str = "end"
    endian: str = "little"
    crcs: tuple = ("end",)
    layout: Layout = CANON
    empty: frozenset = frozenset()
    patch: tuple = ()
    flip: tuple = ()
    cut: int | None = None
    only: frozenset | None = None

    def codecs(self) -> list:
        inner = self.chain.codecs()
        idx = [{"name": "bytes", "configuration": {"endian": self.endian}}] + \
            [{"name": "crc32c", "configuration": {"location": loc}} for loc in self.crcs]
        return [{"name": "sharding_indexed", "configuration": {
            "chunk_shape": list(self.inner_shape), "codecs": inner, "index_codecs": idx,
            "index_location": self.location}}]

    def grid(self, shape):
        return [s // i for s, i in zip(shape, self.inner_shape)]

    def depth(self) -> int:
        return 1 + (self.chain.depth() if isinstance(self.chain, Shard) else 0)


def boxes(shape, inner_shape):
    """the box of every inner chunk, C order"""
    grid = [s // i for s, i in zip(shape, inner_shape)]
    return [tuple(slice(g * i, (g + 1) * i) for g, i in zip(idx, inner_shape))
            for idx in itertools.product(*[range(g) for g in grid])]


def build_shard(inner, layout: Layout, index_location: str, index_codecs, patch=()):
    """inner: the encoded bytes of every inner chunk in C order, None for an empty one. index_codecs:
    (endian, crcs). Returns (shard bytes, entries)."""
    endian, crcs = index_codecs
    n = len(inner)
    alias, selfref = dict(layout.alias), dict(layout.selfref)
    base = index_bytes(n, crcs) if index_location == "start" else 0
    second = layout.overlap[1] if layout.overlap else None
    stored = [k for k in (layout.order if layout.order is not None else range(n))
              if inner[k] is not None and k not in alias and k not in selfref and k != second]
    assert sorted(stored) == [k for k in range(n) if inner[k] is not None and k not in alias and k not in selfref
                              and k != second], "layout.order names every stored inner chunk once"
    body = bytearray(junk(layout.pre))
    entries = [(MAX, MAX)] * n
    for i, k in enumerate(stored):
        if i:
            body += junk(layout.gap, i)
        entries[k] = (base + len(body), len(inner[k]))
        body += inner[k]
        if layout.overlap and k == layout.overlap[0]:
            h = len(inner[k]) // 2
            assert inner[k][h:] == inner[second][:h]
            entries[second] = (entries[k][0] + h, len(inner[second]))
            body += inner[second][h:]
    body += junk(layout.post, 99)
    for k, j in alias.items():
        assert inner[k] == inner[j]
        entries[k] = entries[j]
    for k, off in selfref.items():
        entries[k] = (off, len(inner[k]))
    total = len(body) + index_bytes(n, crcs)
    for k, f in patch:
        entries[k] = tuple(v % 2 ** 64 for v in f(total, *entries[k]))
    idx = pack_index(entries, endian, crcs)
    return (idx + bytes(body) if index_location == "start" else bytes(body) + idx), entries


def encode(sh: Shard, a: np.ndarray, dt: str, path=()) -> bytes:
    """The shard of array `a` (its shape is the shard's), laid out as sh says. `a` is changed in place
    where the layout fixes contents: empty inner chunks take the fill value, aliased and overlapping ones
    are made equal, a self-referencing one takes the bytes its entry names."""
    here = sh.only is None or (path and path[-1] in sh.only)
    bx = boxes(a.shape, sh.inner_shape)
    fill = np.frombuffer(fill_bytes(dt), np_dtype(dt))[0]
    if here:
        for k in sh.empty:
            a[bx[k]] = fill
    for k, j in sh.layout.alias:
        a[bx[k]] = a[bx[j]]
    if sh.layout.overlap:
        assert sh.chain in (LE, BE) and not sh.chain.order
        x, y = sh.layout.overlap
        fa, fb = np.ascontiguousarray(a[bx[x]]).reshape(-1), np.ascontiguousarray(a[bx[y]]).reshape(-1)
        fb[:fb.size // 2] = fa[fa.size // 2:]
        a[bx[y]] = fb.reshape(a[bx[y]].shape)
    inner = []
    for k, b in enumerate(bx):
        if here and k in sh.empty:
            inner.append(None)
        elif isinstance(sh.chain, Shard):
            inner.append(encode(sh.chain, a[b], dt, path + (k,)))  # a view: the nested call writes through
        else:
            inner.append(encode_inner(sh.chain, a[b]))
    shard, entries = build_shard(inner, sh.layout, sh.location, (sh.endian, sh.crcs), sh.patch if here else ())
    for k, off in sh.layout.selfref:
        assert sh.chain == LE
        a[bx[k]] = np.frombuffer(shard[off:off + entries[k][1]], np_dtype(dt)).reshape(sh.inner_shape)
    if not here:
        return shard
    out = bytearray(shard)
    n, x = len(bx), index_bytes(len(bx), sh.crcs)
    ibase = 0 if sh.location == "start" else len(out) - x
    for what, k in sh.flip:
        if what == "crc":
            out[ibase + crc_positions(n, sh.crcs)[k] + 1] ^= 0x10
        else:
            out[entries[k][0] + entries[k][1] // 2] ^= 0x04
    return junk(sh.cut, 5) if sh.cut is not None else bytes(out)


def entries_of(sh: Shard, shape, data: bytes, validate: bool = True):
    """Per inner chunk (C order) its encoded bytes, "empty", or SHARD_INDEX_OOB; or the status of the
    shard as a whole when its index does not decode."""
    n = int(np.prod(sh.grid(shape)))
    x = index_bytes(n, sh.crcs)
    if len(data) < x:
        return SHARD_TOO_SMALL
    idx = parse_index(data[:x] if sh.location == "start" else data[len(data) - x:], n, sh.endian, sh.crcs, validate)
    if isinstance(idx, int):
        return idx
    out = []
    for off, size in idx:
        if off == MAX and size == MAX:
            out.append("empty")
        elif off + size > MAX or off + size > len(data):  # a wrapped sum counts as out of bounds
            out.append(SHARD_INDEX_OOB)
        else:
            out.append(data[off:off + size])
    return out


def read_shard(sh: Shard, shape, dt: str, data, sel=None, validate: bool = True, partial=None):
    """(status, array of the selection's shape, stats). data None: a missing shard, all fill. sel:
    (start, shape) in the shard, None: all of it. Only the inner chunks the selection meets are looked at,
    in C order; the first that fails gives the status. stats: "enc_bytes" the sizes of the present leaf
    entries looked at (an aliased range once per entry), "items" the leaf inner chunks met."""
    shape = list(shape)
    start, sub = (list(sel[0]), list(sel[1])) if sel is not None else ([0] * len(shape), shape)
    if partial is None:
        partial = sub != shape
    out = np.empty(sub, np_dtype(dt))
    out.reshape(-1).view(np.uint8)[:] = np.tile(np.frombuffer(fill_bytes(dt), np.uint8), out.size)
    stats = {"enc_bytes": 0, "items": 0}
    leaf = not isinstance(sh.chain, Shard)
    ent = None if data is None else entries_of(sh, shape, data, validate)
    if isinstance(ent, int):
        return ent, None, stats
    for k, b in enumerate(boxes(shape, sh.inner_shape)):
        lo = [max(s.start, a) for s, a in zip(b, start)]
        hi = [min(s.stop, a + n) for s, a, n in zip(b, start, sub)]
        if any(l >= h for l, h in zip(lo, hi)):
            continue
        dst = tuple(slice(l - a, h - a) for l, h, a in zip(lo, hi, start))
        isel = ([l - s.start for l, s in zip(lo, b)], [h - l for l, h in zip(lo, hi)])
        e = "empty" if ent is None else ent[k]
        if leaf:
            stats["items"] += 1
        if isinstance(e, int):
            return e, None, stats
        if isinstance(e, str):
            if not leaf:  # the leaves of an empty middle shard are still met
                stats["items"] += read_shard(sh.chain, sh.inner_shape, dt, None, isel)[2]["items"]
            continue
        if leaf:
            stats["enc_bytes"] += len(e)
            st, v = decode_inner(sh.chain, e, sh.inner_shape, dt, validate, partial)
            if st:
                return st, None, stats
            out[dst] = v[tuple(slice(s, s + n) for s, n in zip(*isel))]
        else:
            st, v, s2 = read_shard(sh.chain, sh.inner_shape, dt, e, isel, validate, partial)
            stats = {q: stats[q] + s2[q] for q in stats}
            if st:
                return st, None, stats
            out[dst] = v
    return OK, out, stats


# ---------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    group: str
    dtype: str
    shape: tuple         # of the shard
    shard: Shard
    sels: tuple = ()     # partial selections (start, shape); the full read is always made
    validate: bool = True
    seed: int = 0

    def codecs(self) -> list:
        return self.shard.codecs()

    @functools.lru_cache(maxsize=None)
    def built(self):
        """(the array the shard holds, the shard's bytes): built once, never changed"""
        rng = np.random.default_rng(1000 + self.seed + len(self.name))
        es = TYPES[self.dtype][1]
        a = rng.integers(1, 256, int(np.prod(self.shape)) * es, dtype=np.uint8).view(np_dtype(self.dtype)) \
            .reshape(self.shape).copy()
        if any(c in ("gzip", "zstd") for c in leaf_chain(self.shard).b2b):  # something to compress
            a = (a.view(np.uint8) % 4 + 1).astype(np.uint8).view(a.dtype).reshape(self.shape)
        enc = encode(self.shard, a, self.dtype)
        a.setflags(write=False)
        return a, enc

    def expect(self, sel=None, validate=None):
        """(status, array or None, stats) of a read by the model"""
        _, enc = self.built()
        return read_shard(self.shard, self.shape, self.dtype, enc, sel, self.validate if validate is None else validate)


def leaf_chain(sh: Shard) -> Chain:
    return leaf_chain(sh.chain) if isinstance(sh.chain, Shard) else sh.chain


def _cases():
    c = []
    S2, I2 = (4, 6), (2, 3)  # 2 x 2 inner chunks of 6 elements
    SELS2 = (((1, 2), (1, 1)), ((2, 3), (2, 3)), ((0, 0), (2, 6)), ((1, 2), (2, 2)))
    # one element of inner chunk 0; inner chunk 3; the line 0, 1; a box over all four

    def sh(chain=LE, inner=I2, **kw):
        return Shard(inner, chain, **kw)

    # ---- layout -------------------------------------------------------------------------------
    for ch in CHAINS:
        c.append(Case(f"reversed_{ch.name}", "layout", "uint16", S2, sh(ch, layout=Layout(order=(3, 2, 1, 0))), SELS2))
    c.append(Case("permuted_start", "layout", "uint32", S2,
                  sh(BE, location="start", layout=Layout(order=(2, 0, 3, 1))), SELS2))
    for loc in ("start", "end"):
        c.append(Case(f"gaps_1_3_17_{loc}", "layout", "uint16", S2,
                      sh(LE_CRC, location=loc, layout=Layout(pre=1, gap=3, post=17)), SELS2))
        # inner rows of 16 bytes: whole inner chunks of a gzip chain can take the direct-rows path
        c.append(Case(f"gaps_17_1_3_permuted_{loc}", "layout", "float32", (4, 8),
                      sh(GZ_CRC, inner=(2, 4), location=loc, layout=Layout(order=(1, 3, 0, 2), pre=17, gap=1, post=3)),
                      (((1, 2), (1, 1)), ((2, 4), (2, 4)), ((0, 0), (2, 8)), ((1, 3), (2, 2)))))
    c.append(Case("gaps_3_17_1_zstd", "layout", "uint16", S2, sh(ZSTD, layout=Layout(pre=3, gap=17, post=1)), SELS2))
    c.append(Case("alias_two", "layout", "uint16", S2, sh(LE_CRC, layout=Layout(alias=((2, 1),))), SELS2))
    c.append(Case("alias_all", "layout", "uint16", S2,
                  sh(TR_BE, location="start", layout=Layout(alias=((1, 0), (2, 0), (3, 0)), pre=1)), SELS2))
    c.append(Case("overlap_half", "layout", "uint8", S2, sh(LE, layout=Layout(overlap=(1, 2), pre=3)), SELS2))
    # index at the start, 4 entries + one crc32c = 68 bytes; entry 3 names bytes 16..32 of the shard,
    # entry 1 of the index itself: offsets are absolute, not relative to the end of the index
    c.append(Case("entry_into_index", "layout", "uint8", (8, 8),
                  sh(LE, inner=(4, 4), location="start", layout=Layout(selfref=((3, 16),))),
                  (((5, 5), (2, 2)), ((3, 3), (2, 2)))))
    # ---- entries ------------------------------------------------------------------------------
    for loc in ("start", "end"):
        c.append(Case(f"all_empty_{loc}", "entries", "uint16", S2, sh(LE, location=loc, empty=frozenset(range(4))), SELS2[:2]))
    c.append(Case("some_empty", "entries", "uint16", S2, sh(GZ_CRC, empty=frozenset((0, 3)), layout=Layout(order=(2, 1))), SELS2))
    half = {"half_sentinel_offset": lambda n, o, s: (MAX, s), "half_sentinel_size": lambda n, o, s: (o, MAX),
            "past_end_by_one": lambda n, o, s: (n - s + 1, s), "offset_len_plus_100": lambda n, o, s: (n + 100, s),
            "wrapped_sum": lambda n, o, s: (MAX - 1, 4)}
    for name, f in half.items():  # entry 1 is bad: reads of inner chunks 0, 2, 3 alone do not look at it
        c.append(Case(name, "entries", "uint16", S2, sh(LE_CRC, patch=((1, f),)),
                      (SELS2[0], SELS2[1], ((2, 0), (2, 6)), ((0, 3), (2, 3)))))
    # with the index at the start the last inner chunk ends at the shard's end: offset + size == len
    c.append(Case("ends_at_len", "entries", "uint16", S2, sh(LE, location="start"), SELS2[:2]))
    # index at the end: three stored inner chunks of 12 bytes and 68 bytes of index; entry 1 names the last
    # 12 bytes of the shard (the end of the index): offset + size == len
    c.append(Case("ends_at_len_in_index", "entries", "uint16", S2, sh(LE, layout=Layout(selfref=((1, 92),))), SELS2[:2]))
    for ch in CHAINS:  # a present entry of size 0: the inner chain's own status for zero bytes
        c.append(Case(f"size0_at_len_{ch.name}", "entries", "uint16", S2,
                      sh(ch, patch=((2, lambda n, o, s: (n, 0)),)), (SELS2[0], SELS2[1])))
    c.append(Case("size0_at_0", "entries", "uint16", S2, sh(LE_CRC, location="start", patch=((0, lambda n, o, s: (0, 0)),)),
                  (SELS2[1],)))
    # ---- the index chain ----------------------------------------------------------------------
    for endian, loc in itertools.product(("little", "big"), ("start", "end")):
        for crcs in ((), ("end",), ("start", "end"), ("end", "start", "end", "end")):
            c.append(Case(f"index_{endian}_{loc}_{len(crcs)}crc", "index", "uint16", S2,
                          sh(LE, endian=endian, location=loc, crcs=crcs, layout=Layout(order=(1, 0, 3, 2), gap=1)), SELS2[:2]))
    for crcs in (("end",), ("start", "end"), ("end", "start", "end", "end")):
        for i in range(len(crcs)):
            s = sh(LE_CRC, crcs=crcs, flip=(("crc", i),))
            c.append(Case(f"index_{len(crcs)}crc_corrupt_{i}", "index", "uint16", S2, s, SELS2[:1]))
            c.append(Case(f"index_{len(crcs)}crc_corrupt_{i}_novalidate", "index", "uint16", S2, s, SELS2[:1], validate=False))
    s = sh(LE_CRC, crcs=("start", "end"), flip=(("crc", 1),), patch=((1, half["offset_len_plus_100"]),))
    c.append(Case("index_corrupt_and_oob", "index", "uint16", S2, s, SELS2[:1]))
    c.append(Case("index_corrupt_and_oob_novalidate", "index", "uint16", S2, s, SELS2[:1], validate=False))
    # ---- length -------------------------------------------------------------------------------
    for loc in ("start", "end"):
        for n in (0, 1, index_bytes(4, ("end",)) - 1):
            c.append(Case(f"length_{n}_{loc}", "length", "uint16", S2, sh(LE, location=loc, cut=n), SELS2[:1]))
    # ---- size ---------------------------------------------------------------------------------
    c.append(Case("one_inner", "size", "uint16", I2, sh(LE_CRC, location="start", layout=Layout(pre=1, post=3)),
                  (((1, 1), (1, 2)),)))
    c.append(Case("eight_3d", "size", "uint16", (4, 4, 6), sh(TR3, inner=(2, 2, 3), layout=Layout(order=(7, 0, 6, 1, 5, 2, 4, 3), gap=3)),
                  (((1, 1, 2), (2, 2, 2)), ((2, 2, 3), (2, 2, 3)))))
    c.append(Case("sixteen_4d", "size", "uint8", (2, 4, 4, 6), sh(LE_CRC, inner=(1, 2, 2, 3), empty=frozenset((5,)),
                                                                 layout=Layout(order=tuple(k for k in range(15, -1, -1) if k != 5), pre=1)),
                  (((0, 1, 1, 2), (2, 2, 2, 2)),)))
    # 300 entries, 600 index words: more than k_shard_index has threads (CRC_THREADS = 256)
    order = tuple(int(k) for k in np.random.default_rng(3).permutation(300))
    c.append(Case("three_hundred", "size", "uint8", (40, 30), sh(LE, inner=(2, 2), endian="big", crcs=("start",),
                                                                layout=Layout(order=order, gap=1)),
                  (((39, 29), (1, 1)), ((1, 1), (38, 28)))))
    # ---- partial reads past poisoned entries ---------------------------------------------------
    # 3 x 3 inner chunks, number 2 (the top right corner) poisoned: an element, an inner chunk, a line of
    # them and a box crossing inner boundaries in both axes, none of which meets it
    psel = (((0, 0), (1, 1)), ((2, 3), (2, 3)), ((4, 0), (2, 9)), ((3, 1), (2, 4)))
    for ch in (LE_CRC, GZ_CRC):
        lay = Layout(order=(8, 1, 6, 3, 4, 5, 2, 7, 0), gap=3)
        c.append(Case(f"poison_oob_{ch.name}", "partial", "uint16", (6, 9),
                      sh(ch, layout=lay, patch=((2, half["offset_len_plus_100"]),)), psel))
        c.append(Case(f"poison_bytes_{ch.name}", "partial", "uint16", (6, 9), sh(ch, layout=lay, flip=(("inner", 2),)), psel))
    # ---- nesting: [8, 12] shards of [4, 6] middle shards of [2, 3] leaves ------------------------
    mid = Shard(I2, LE_CRC, location="start", endian="big", crcs=(), layout=Layout(order=(2, 0, 3, 1), pre=1, gap=3, post=1))
    nsel = (((1, 2), (1, 1)), ((3, 5), (2, 2)), ((0, 0), (4, 12)), ((4, 0), (4, 6)), ((4, 9), (2, 3)))
    c.append(Case("nested2", "nesting", "uint16", (8, 12),
                  Shard(S2, mid, layout=Layout(order=(3, 0, 1), gap=17, post=3), empty=frozenset((2,))), nsel))
    bad_mid = dataclasses.replace(mid, patch=((1, half["half_sentinel_size"]),), only=frozenset((3,)))
    c.append(Case("nested2_mid_oob", "nesting", "uint16", (8, 12),
                  Shard(S2, bad_mid, layout=Layout(order=(3, 0, 1), gap=17, post=3), empty=frozenset((2,))), nsel))
    top = (16, 24)
    nsel3 = (((1, 2), (1, 1)), ((7, 11), (2, 2)), ((0, 0), (8, 12)), ((12, 21), (2, 3)))
    for name, m in (("nested3", mid), ("nested3_mid_oob", bad_mid)):
        c.append(Case(name, "nesting", "uint16", top,
                      Shard((8, 12), Shard(S2, m, location="start", layout=Layout(order=(3, 0, 1), gap=1), empty=frozenset((2,))),
                            layout=Layout(order=(1, 3, 0), pre=3), empty=frozenset((2,))), nsel3))
    # a bad entry in the outermost index of three levels, which the general path reads on the host
    for name in ("half_sentinel_offset", "half_sentinel_size", "wrapped_sum", "past_end_by_one"):
        c.append(Case(f"nested3_top_{name}", "nesting", "uint16", top,
                      Shard((8, 12), Shard(S2, mid, location="start", layout=Layout(order=(3, 0, 1), gap=1), empty=frozenset((2,))),
                            layout=Layout(order=(1, 3, 0), pre=3), empty=frozenset((2,)), patch=((1, half[name]),)), nsel3))
    return c


TR3 = Chain("transpose3_bytes", endian="big", order=(2, 0, 1))
CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

FIVE_CRCS = Shard((2, 3), LE, crcs=("end",) * 5)  # the GPU refuses it: UNSUPPORTED at chain or plan creation


# ---------------------------------------------------------------------------------------------------
# the readers of the library every case runs against (test_gpu_shards.py), and the refusals by design
# ---------------------------------------------------------------------------------------------------
READERS = ("batch", "array", "cache", "wrapped", "transposed", "deeper", "plugin", "store")
# batch: CodecChain.decode_batch (the fused plan one and two levels deep, the general path below that);
# array / cache: Array and ArrayCached over a grid of shards with the case's shard in it; wrapped /
# transposed / deeper: the case's shard under crc32c + gzip after sharding_indexed, under a transpose before
# it, and as an inner chunk of one more sharding level (the general path; for a one-level case `deeper` is
# the fused plan's second level); plugin: decode_pinned_into; store: store_array_subset, which takes its old
# shards from the layouts of the table (test_gpu_shards.OLD_LAYOUTS) and so needs a one-level chain.
REFUSALS = {
    # (reader, predicate on the case): reason. The reader answers UNSUPPORTED, and the test asserts that.
    "store": (lambda c: c.shard.depth() > 1, "the store path writes one sharding level: nested sharding is refused"),
}


def refusal(case: Case, reader: str):
    """None, or why `reader` refuses the case's chain by design (it answers UNSUPPORTED)"""
    assert reader in READERS
    pred, why = REFUSALS.get(reader, (None, None))
    return why if pred and pred(case) else None


def readers(case: Case) -> dict:
    """{reader: None or the reason of its refusal}: every case runs against every reader"""
    return {r: refusal(case, r) for r in READERS}


def clean(sh: Shard) -> Shard:
    """sh without its bad entries, flipped bytes and cut: a neighbour of the case's shard in a grid"""
    return dataclasses.replace(sh, patch=(), flip=(), cut=None, chain=clean(sh.chain) if isinstance(sh.chain, Shard) else sh.chain)
