"""Replay scripts for prepared plans: what one plan over FIXED device buffers is given execute after
execute, and what each execute must answer. numpy and pure Python; no GPU.

A plan fixes (pointer, encoded length) per descriptor, so everything that changes between two executes
is the CONTENT of its buffers. A Variant is one such content: the encoded bytes of every descriptor
(all variants of a family brought to one length per descriptor by padding the format allows), the
status every descriptor must get, and the decoded selection of every descriptor whose status is 0. A
Family is one plan (chain, data type, chunk shape, output shape, descriptors) and a script, the list
of variants executed in order; test_gpu_plan_replay.py holds every execute of a script to the variant,
and test_plan_replay_model.py holds the variants to their CPU references and the scripts to the
transitions they claim.

No codec writer lives here. The bytes come from the suite's writers (shard_model.build_shard,
zstd_frames, deflate_streams, blosc_inner_streams / blosc_frames, bz2_streams, Python's zlib, the
oracle's encoder for chains with no compressor); the expectations from the references the suite already
trusts (shard_model.read_shard, the oracle's decoder over libzstd and c-blosc, Python's zlib and bz2,
test_checksum_models' checkers, the hand-built cases' own `expect`). Never from the library.

Padding to the common length: a shard grows by junk bytes after its last inner chunk (Layout.post;
the index at the end or at the start), an unsharded zstd chunk by a trailing skippable frame, a blosc
frame by slack after its cbytes. zlib, bz2 and the checksums have no legal padding and appear inside
shards only.
"""
from __future__ import annotations

import functools
import struct
import zlib
from dataclasses import dataclass, field

import numpy as np

import shard_model as SM
import zstd_frames as Z
from scatter_cases import TYPES, fill_bytes

OK, INVALID_CHECKSUM, DECODED_SIZE_MISMATCH, SHARD_INDEX_OOB, CORRUPT_STREAM = 0, 1, 2, 3, 4
ROWS, TILED, GENERIC, TILED_PERSISTENT = range(4)  # zgpu_plan_scatter_path

BYTES_LE = {"name": "bytes", "configuration": {"endian": "little"}}


@dataclass(frozen=True)
class Desc:
    """One descriptor of the plan: the selection of its chunk and where it goes in the output. null: the
    descriptor has no encoded bytes (a NULL pointer: a missing chunk, all fill) in every variant."""
    sel_start: tuple
    sel_shape: tuple
    out_start: tuple
    null: bool = False


@dataclass
class Variant:
    """enc[d]: descriptor d's encoded bytes, padded (None for a null descriptor); status[d]; expect[d]: the
    selection's array when status[d] == 0. mismatch: what zgpu_last_size_mismatch answers after the
    execute, (descriptor, len, expected_len), when the FIRST failing descriptor failed with
    DECODED_SIZE_MISMATCH; else None. facts: what the variant was built to be, for the model test."""
    name: str
    enc: list
    status: list
    expect: list
    mismatch: tuple | None = None
    facts: dict = field(default_factory=dict)
    counters: dict | None = None  # {"enc_bytes", "items"} by shard_model.read_shard, where every descriptor is clean


@dataclass
class Family:
    name: str
    codecs: list
    dtype: str
    chunk_shape: tuple
    out_shape: tuple
    descs: list
    variants: dict          # name -> Variant
    script: list            # variant names, in execute order
    modes: dict = field(default_factory=lambda: {"default": {}})  # mode name -> environment of plan and executes
    path: tuple = (ROWS, ROWS)  # zgpu_plan_scatter_path with the output 16-byte aligned / offset by one element
    facts: dict = field(default_factory=dict)

    def lengths(self):
        """The plan's encoded length per descriptor: one for all variants (asserted by the model test)."""
        v = self.variants[self.script[0]]
        return [0 if e is None else len(e) for e in v.enc]

    def np_dtype(self):
        return np.dtype(TYPES[self.dtype][0])

    def fill(self):
        return np.frombuffer(fill_bytes(self.dtype), self.np_dtype())[0]


def rc_of(statuses) -> int:
    return next((s for s in statuses if s), OK)


def fill_array(shape, dt: str) -> np.ndarray:
    a = np.empty(shape, np.dtype(TYPES[dt][0]))
    a.reshape(-1).view(np.uint8)[:] = np.tile(np.frombuffer(fill_bytes(dt), np.uint8), a.size)
    return a


def _rng(seed):
    return np.random.default_rng(seed)


def _pad_to(encs_by_variant: dict, pad):
    """{variant: [bytes]} with every descriptor's bytes brought to the longest of its variants by
    pad(bytes, n) -> bytes of length n (n >= len(bytes); pad may ask for room: see _zstd_pad)."""
    names = list(encs_by_variant)
    nd = len(encs_by_variant[names[0]])
    out = {v: [None] * nd for v in names}
    for d in range(nd):
        if encs_by_variant[names[0]][d] is None:
            continue
        n = max(len(encs_by_variant[v][d]) for v in names)
        for v in names:
            out[v][d] = pad(encs_by_variant[v][d], n)
    return out


# ---------------------------------------------------------------------------------------------------
# shards: built by shard_model.build_shard, read back by shard_model.read_shard or read_shard_with
# ---------------------------------------------------------------------------------------------------
def gz(data: bytes, level: int) -> bytes:
    z = zlib.compressobj(level, zlib.DEFLATED, 31)
    return z.compress(data) + z.flush()


def with_crc32c(enc: bytes) -> bytes:
    return enc + struct.pack("<I", SM.crc32c(enc))


@dataclass
class ShardSpec:
    """One shard of a variant. a: the array it holds; enc(k, block) -> the inner chunk's bytes; empty: inner
    chunks with an empty entry; replace {k: bytes}: inner chunks whose bytes are given; patch: as
    shard_model.build_shard's; flip_tail {k}: a byte of inner chunk k's last four flipped; flip_index_crc:
    the index's stored crc32c flipped."""
    a: np.ndarray
    enc: object
    layout: SM.Layout = SM.CANON
    empty: frozenset = frozenset()
    replace: dict = field(default_factory=dict)
    patch: tuple = ()
    flip_tail: frozenset = frozenset()
    flip_index_crc: bool = False


def shard_bytes(sp: ShardSpec, inner_shape, location: str, total: int | None = None) -> bytes:
    """The shard (index: little-endian, one crc32c at the end), padded to `total` bytes by junk after its
    last inner chunk."""
    bx = SM.boxes(sp.a.shape, inner_shape)
    inner = [None if k in sp.empty else sp.replace[k] if k in sp.replace else sp.enc(k, np.ascontiguousarray(sp.a[b]))
             for k, b in enumerate(bx)]
    crcs = ("end",)

    def build(post):
        lay = SM.Layout(order=sp.layout.order, pre=sp.layout.pre, gap=sp.layout.gap, post=post)
        return SM.build_shard(inner, lay, location, ("little", crcs), sp.patch)

    data, entries = build(sp.layout.post)
    if total is not None:
        assert total >= len(data)
        data, entries = build(sp.layout.post + total - len(data))
        assert len(data) == total
    out = bytearray(data)
    for k in sp.flip_tail:
        out[entries[k][0] + entries[k][1] - 2] ^= 0x10
    if sp.flip_index_crc:
        x = SM.index_bytes(len(bx), crcs)
        out[(0 if location == "start" else len(out) - x) + SM.crc_positions(len(bx), crcs)[0] + 1] ^= 0x10
    return bytes(out)


def read_shard_with(sh: SM.Shard, shape, dt: str, data: bytes, decode):
    """shard_model.read_shard of the whole shard for an inner chain the model has no decoder of:
    decode(bytes) -> (status, the inner chunk's bytes). The index, the entries and the order of failure
    are the model's (entries_of)."""
    out = fill_array(shape, dt)
    ent = SM.entries_of(sh, shape, data)
    if isinstance(ent, int):
        return ent, None
    nbytes = int(np.prod(sh.inner_shape)) * TYPES[dt][1]
    for k, b in enumerate(SM.boxes(shape, sh.inner_shape)):
        e = ent[k]
        if isinstance(e, int):
            return e, None
        if isinstance(e, str):
            continue
        st, raw = decode(e)
        if st:
            return st, None
        if len(raw) != nbytes:
            return DECODED_SIZE_MISMATCH, None
        out[b] = np.frombuffer(raw, out.dtype).reshape(sh.inner_shape)
    return OK, out


def _shard_family(name, dt, shape, inner_shape, location, inner_codecs, specs: dict, script, read, sel=None, **kw):
    """A family of n shards per variant stacked along axis 0. specs: {variant: [ShardSpec per shard]}; read(
    bytes) -> (status, array of the selection) is the CPU reference. sel: (start, shape) in the shard."""
    names = list(specs)
    n = len(specs[names[0]])
    total = [max(len(shard_bytes(specs[v][s], inner_shape, location)) for v in names) for s in range(n)]
    start, sub = sel if sel is not None else ((0,) * len(shape), tuple(shape))
    # a partial selection lands in an output of whole shards: the bytes around it stay untouched
    descs = [Desc(tuple(start), tuple(sub), (s * shape[0] + start[0],) + tuple(start[1:])) for s in range(n)]
    variants = {}
    for v in names:
        enc = [shard_bytes(specs[v][s], inner_shape, location, total[s]) for s in range(n)]
        got = [read(e) for e in enc]
        variants[v] = Variant(v, enc, [g[0] for g in got], [g[1] for g in got], facts={"specs": specs[v]})
        if all(len(g) == 3 and g[0] == OK for g in got):  # the model's count of what a clean read resolves
            variants[v].counters = {k: sum(g[2][k] for g in got) for k in ("enc_bytes", "items")}
    codecs = [{"name": "sharding_indexed", "configuration": {
        "chunk_shape": list(inner_shape), "codecs": inner_codecs,
        "index_codecs": [BYTES_LE, {"name": "crc32c", "configuration": {"location": "end"}}],
        "index_location": location}}]
    return Family(name, codecs, dt, tuple(shape), (n * shape[0],) + tuple(shape[1:]), descs, variants, list(script), **kw)


# ---- shard_gzip_crc: the C3 inner chain [bytes, gzip, crc32c] --------------------------------------
GZ_SHAPE, GZ_INNER = (8, 16, 16), (2, 4, 16)  # 16 inner chunks of 512 bytes, rows of 64 bytes (direct rows)
GZ_PARTIAL = ((1, 2, 3), (6, 11, 9))           # meets all 16 inner chunks, none of them whole
GZ_REVERSED = SM.Layout(order=tuple(range(15, -1, -1)), pre=5, gap=3)
GZ_MODES = {f"{k}-direct{d}": dict({"ZGPU_GZIP_DIRECT": d}, **({"ZGPU_GZIP_PIPE_MAX": "0"} if k == "one_wave" else {}))
            for k in ("pipelined", "one_wave") for d in ("1", "0")}


def _small_floats(seed, shape=GZ_SHAPE):
    return _rng(seed).integers(0, 7, shape).astype(np.float32)  # compresses well: stored streams are far longer


def corrupt_deflate():
    """deflate_streams' blocks_type3: two literals, then a block of the reserved type"""
    import deflate_streams as D
    c = [c for c in D.family("blocks") if c.name == "blocks_type3"]
    assert len(c) == 1 and c[0].status == D.CORRUPT
    return c[0]


def _gz_specs(enc_of, corrupt_inner, tail_flip):
    """The variants of shard_gzip_crc / shard_zlib. enc_of(level) -> enc(k, block)."""
    a1 = [_small_floats(11), _small_floats(12)]
    a2 = [_small_floats(21), _small_floats(22)]
    mixed = lambda k, b: enc_of(0 if k % 3 == 0 else 9)(k, b)  # noqa: E731  (every third stream stored)
    A = [ShardSpec(a, enc_of(1)) for a in a1]
    B = [ShardSpec(a, mixed, GZ_REVERSED, frozenset((3, 7))) for a in a2]
    C = [ShardSpec(a2[0], mixed, GZ_REVERSED, frozenset((3, 7)), replace={9: corrupt_inner}, flip_tail=frozenset(tail_flip)),
         ShardSpec(a2[1], mixed, GZ_REVERSED, frozenset((3, 7)), flip_index_crc=True)]
    D = [ShardSpec(a1[0], enc_of(1), empty=frozenset((0,))),
         ShardSpec(a1[1], enc_of(1), empty=frozenset((0,)), patch=((6, lambda n, o, s: (n + 100, s)),))]
    return {"A": A, "B": B, "C": C, "D": D}


def _shard_gzip_crc(partial: bool):
    sh = SM.Shard(GZ_INNER, SM.GZ_CRC, location="start" if partial else "end")
    sel = GZ_PARTIAL if partial else None
    enc_of = lambda level: (lambda k, b: with_crc32c(gz(b.tobytes(), level)))  # noqa: E731
    specs = _gz_specs(enc_of, corrupt_deflate().enc("gz_crc"), (5,))

    def read(data):
        return SM.read_shard(sh, GZ_SHAPE, "float32", data, sel, partial=partial)
    return _shard_family("shard_gzip_crc_partial" if partial else "shard_gzip_crc", "float32", GZ_SHAPE, GZ_INNER, sh.location,
                         SM.GZ_CRC.codecs(), specs, ["A", "A", "B", "C", "B", "D", "A"], read, sel, modes=GZ_MODES)


@functools.lru_cache(maxsize=None)
def shard_gzip_crc():
    return _shard_gzip_crc(False)


@functools.lru_cache(maxsize=None)
def shard_gzip_crc_partial():
    return _shard_gzip_crc(True)


# ---- shard_zlib: the same shape on numcodecs.zlib ---------------------------------------------------
def zlib_decode(e: bytes):
    try:
        z = zlib.decompressobj()
        raw = z.decompress(e)
        return (OK, raw) if z.eof else (CORRUPT_STREAM, None)
    except zlib.error:
        return CORRUPT_STREAM, None


@functools.lru_cache(maxsize=None)
def shard_zlib():
    sh = SM.Shard(GZ_INNER, None)
    enc_of = lambda level: (lambda k, b: zlib.compress(b.tobytes(), level))  # noqa: E731
    specs = _gz_specs(enc_of, None, ())
    del specs["D"]
    # C: B with inner chunk 9 of shard 0 under a wrong Adler-32 (the trailer's last bytes flipped)
    b0 = specs["B"][0]
    specs["C"] = [ShardSpec(b0.a, b0.enc, b0.layout, b0.empty, flip_tail=frozenset((9,))), specs["B"][1]]
    return _shard_family("shard_zlib", "float32", GZ_SHAPE, GZ_INNER, "end",
                         [BYTES_LE, {"name": "numcodecs.zlib", "configuration": {"level": 1}}], specs, ["A", "B", "C", "A"],
                         lambda data: read_shard_with(sh, GZ_SHAPE, "float32", data, zlib_decode))


# ---- checksum_ranges: [bytes, gzip, X] with one inner chunk per shard, three ranges and under one -----
CK_RANGE = 256 << 10  # kernels/linsum.hpp, as tests/test_checksum_models.py has it
CK_N = 2 * CK_RANGE + 4096  # the inner chunk's bytes: stored, its gzip member is three checksum ranges long


def _ck(kind: str, e: bytes) -> bytes:
    import oracle
    from test_checksum_models import encode_checksum
    return e + struct.pack("<I", oracle.crc32c(e)) if kind == "crc32c" else encode_checksum(kind, e, False)


def ck_decode(kind: str, e: bytes):
    """(status, bytes): the checksum by the suite's checkers, the member by Python's zlib"""
    import oracle
    from test_checksum_models import checksum
    if len(e) < 4:
        return SM.CRC_INPUT_TOO_SHORT, None
    stored, body = int.from_bytes(e[-4:], "little"), e[:-4]
    if stored != (oracle.crc32c(body) if kind == "crc32c" else checksum(kind, body)):
        return INVALID_CHECKSUM, None
    try:
        z = zlib.decompressobj(31)
        raw = z.decompress(body)
        return (OK, raw) if z.eof else (CORRUPT_STREAM, None)
    except zlib.error:
        return CORRUPT_STREAM, None


CK_CODECS = {"adler32": {"name": "numcodecs.adler32", "configuration": {"location": "end"}},
             "fletcher32": {"name": "numcodecs.fletcher32"},
             "crc32c": {"name": "crc32c"}}


@functools.lru_cache(maxsize=None)
def checksum_ranges(kind: str):
    shape = (CK_N,)
    sh = SM.Shard(shape, None)
    noise = [_rng(31 + s).integers(0, 256, CK_N, dtype=np.uint8) for s in range(2)]
    flat = [np.full(CK_N, 3 + s, np.uint8) for s in range(2)]
    long_ = lambda k, b: _ck(kind, gz(b.tobytes(), 0))   # noqa: E731  (stored blocks: longer than its data)
    short = lambda k, b: _ck(kind, gz(b.tobytes(), 9))   # noqa: E731
    # shard 0 follows the script; shard 1 runs in the opposite phase and is always valid
    specs = {"long": [ShardSpec(noise[0], long_), ShardSpec(flat[1], short)],
             "short": [ShardSpec(flat[0], short), ShardSpec(noise[1], long_)],
             "long_bad": [ShardSpec(noise[0], long_, flip_tail=frozenset((0,))), ShardSpec(flat[1], short)]}
    inner = [BYTES_LE, {"name": "gzip", "configuration": {"level": 1}}, CK_CODECS[kind]]
    return _shard_family(f"checksum_ranges_{kind}", "uint8", shape, shape, "end", inner, specs,
                         ["long", "short", "long_bad", "short"],
                         lambda data: read_shard_with(sh, shape, "uint8", data, lambda e: ck_decode(kind, e)),
                         facts={"kind": kind})


# ---- shard_bz2: one block, three blocks, one block per inner chunk ---------------------------------
BZ_SHAPE, BZ_INNER = (8, 32768), (1, 32768)  # 32 KiB slots: 1 MiB of bz2 scratch holds five of the eight items


def _runs(seed, n):
    """n bytes in runs of 100 to 259 equal bytes: RLE1 leaves a few hundred, which the Python BWT sorts at once"""
    r, out = _rng(seed), bytearray()
    while len(out) < n:
        out += bytes([int(r.integers(0, 256))]) * int(r.integers(100, 260))
    return bytes(out[:n])


def bz2_decode(e: bytes):
    import bz2
    try:
        return OK, bz2.decompress(e)
    except (OSError, ValueError):
        return CORRUPT_STREAM, None


@functools.lru_cache(maxsize=None)
def shard_bz2():
    import bz2_streams as BZ
    sh = SM.Shard(BZ_INNER, None)

    def enc(parts):
        def f(k, b):
            d, n = b.tobytes(), len(b.tobytes())
            cuts = [n * i // parts for i in range(parts + 1)]
            return BZ.stream([BZ.block_of(d[lo:hi]) for lo, hi in zip(cuts, cuts[1:])])
        return f
    a = [np.frombuffer(_runs(41 + v, BZ_SHAPE[0] * BZ_SHAPE[1]), np.uint8).reshape(BZ_SHAPE) for v in range(2)]
    specs = {"one": [ShardSpec(a[0], enc(1))], "three": [ShardSpec(a[1], enc(3))]}
    return _shard_family("shard_bz2", "uint8", BZ_SHAPE, BZ_INNER, "end", [BYTES_LE, {"name": "numcodecs.bz2", "configuration": {"level": 9}}],
                         specs, ["one", "three", "one"],
                         lambda data: read_shard_with(sh, BZ_SHAPE, "uint8", data, bz2_decode),
                         modes={"default": {}, "rounds": {"ZGPU_BZ2_SCRATCH_MB": "1"}})


# ---- nested: [8, 12] shards of [4, 6] middle shards of [2, 3] leaves, fused two levels deep ------------
N_SHAPE, N_MID, N_LEAF = (8, 12), (4, 6), (2, 3)


@functools.lru_cache(maxsize=None)
def nested():
    import dataclasses
    mid = SM.Shard(N_LEAF, SM.LE_CRC, location="start", endian="little", crcs=("end",), layout=SM.Layout(order=(2, 0, 3, 1), gap=1))
    bad_mid = dataclasses.replace(mid, flip=(("crc", 0),), only=frozenset((1,)))
    top = lambda m, **kw: SM.Shard(N_MID, m, crcs=("end",), **kw)  # noqa: E731
    # shard 0's middle shard 1: present, empty, present with a bad index checksum, present; shard 1 stays whole
    shards = {"present": top(mid), "empty": top(mid, empty=frozenset((1,))), "bad_crc": top(bad_mid)}
    script = ["present", "empty", "bad_crc", "present"]
    enc0 = {}
    for v, sh in shards.items():
        a = _rng(50 + len(v)).integers(1, 60000, N_SHAPE).astype(np.uint16)
        enc0[v] = SM.encode(sh, a, "uint16")
    total = max(len(e) for e in enc0.values())
    variants = {}
    for i, (v, sh) in enumerate(shards.items()):
        # the outer shard grows by junk in front of its index (Layout.post), the model's own padding
        a = _rng(50 + len(v)).integers(1, 60000, N_SHAPE).astype(np.uint16)
        padded = dataclasses.replace(sh, layout=SM.Layout(post=total - len(enc0[v])))
        e0 = SM.encode(padded, a, "uint16")
        a1 = _rng(60 + i).integers(1, 60000, N_SHAPE).astype(np.uint16)
        e1 = SM.encode(top(mid), a1, "uint16")
        enc = [e0, e1]
        got = [SM.read_shard(shards["present"], N_SHAPE, "uint16", e)[:2] for e in enc]
        variants[v] = Variant(v, enc, [g[0] for g in got], [g[1] for g in got])
    descs = [Desc((0, 0), N_SHAPE, (s * N_SHAPE[0], 0)) for s in range(2)]
    return Family("nested", shards["present"].codecs(), "uint16", N_SHAPE, (2 * N_SHAPE[0], N_SHAPE[1]), descs, variants, script)


# ---------------------------------------------------------------------------------------------------
# unsharded zstd: six chunks of 4096 bytes, padded by a trailing skippable frame
# ---------------------------------------------------------------------------------------------------
ZN, ZK = 4096, 6
ZSTD_CODEC = {"name": "zstd", "configuration": {"level": 3, "checksum": False}}
ZSTD_CHAINS = {"u8": ([BYTES_LE, ZSTD_CODEC], "uint8"),
               "shuffle_u16": ([BYTES_LE, {"name": "numcodecs.shuffle", "configuration": {"elementsize": 2}}, ZSTD_CODEC], "uint16")}


def reserved_block_frame() -> bytes:
    """A frame announcing ZN bytes: a raw block of 100 bytes, then a block of the reserved type 3"""
    return struct.pack("<IB", Z.MAGIC, 0xA0) + struct.pack("<I", ZN) + struct.pack("<I", 0 | Z.RAW << 1 | 100 << 3)[:3] + \
        bytes(range(100)) + struct.pack("<I", 1 | 3 << 1 | 10 << 3)[:3] + bytes(10)


def _zstd_pad(e: bytes, n: int) -> bytes:
    return e if len(e) == n else e + Z.skippable(bytes(n - len(e) - 8))


def zstd_items():
    """{variant: [(frame bytes, the Case it came from or None)]}"""
    exact = {c.name: c for c in Z.family_chains_exact()}
    cap = {c.name: c for c in Z.family_capacity()}
    text = [Z.text(ZN, 70 + i) for i in range(ZK)]
    A = [(Z.stream_frame(t, 0), None) for t in text]
    B = [(exact[f"depth_{ZN}_k{k}"].enc, exact[f"depth_{ZN}_k{k}"]) for k in (15, 16, 17, 31, 32, 33)]
    C = []
    for i in range(ZK):
        if i == 4:  # 65 blocks: one more than the block-parallel pipeline's records hold
            C.append((cap[f"blk_cap_above_{ZN}"].enc, cap[f"blk_cap_above_{ZN}"]))
        elif i % 2:
            C.append((Z.build(Z.Frame([Z.rle(17 * i, ZN // 2), Z.rle(17 * i + 1, ZN // 2)])), None))
        else:
            C.append((Z.build(Z.Frame([Z.raw(_rng(80 + i).integers(0, 256, ZN, dtype=np.uint8).tobytes())])), None))
    short = lambda n: Z.stream_frame(Z.text(n, n), 0)  # noqa: E731  (a whole frame of fewer bytes than the chunk)
    D = list(A)
    D[1] = (short(4000), None)
    D[3] = (reserved_block_frame(), None)
    D2 = list(B)  # test_two_plans_interleaved: the other plan's failing variant
    D2[2] = (short(3000), None)
    return {"A": A, "B": B, "C": C, "D": D, "D2": D2}


@functools.lru_cache(maxsize=None)
def zstd_chunks(chain: str = "u8", nd: int = 1):
    """nd: the chunks as [1, .., 1, n] (a plan group has one ndim for all its parts)."""
    import oracle as O
    from test_gpu_zstd_frames import PATHS
    codecs, dt = ZSTD_CHAINS[chain]
    es = TYPES[dt][1]
    oc = O.OracleChain.from_metadata(codecs, dt, fill_bytes(dt), 1)
    items = zstd_items()
    room = max(len(e) for v in items.values() for e, _ in v) + 8  # every chunk can take a skippable frame
    encs = {v: [_zstd_pad(e, room) for e, _ in it] for v, it in items.items()}
    variants = {}
    for v, enc in encs.items():
        st, exp = [], []
        for e in enc:
            try:
                exp.append(oc.decode(e, (ZN // es,)).reshape((1,) * (nd - 1) + (ZN // es,)))
                st.append(OK)
            except O.OracleError as err:
                exp.append(None)
                st.append(err.status)
        short = {"D": (1, 4000, ZN), "D2": (2, 3000, ZN)}.get(v)
        variants[v] = Variant(v, enc, st, exp, short, {"cases": [c for _, c in items[v]]})
    shape = (1,) * (nd - 1) + (ZN // es,)
    descs = [Desc((0,) * nd, shape, (i,) + (0,) * (nd - 1) if nd > 1 else (i * shape[0],)) for i in range(ZK)]
    out_shape = (ZK,) + shape[1:] if nd > 1 else (ZK * shape[0],)
    return Family(f"zstd_chunks_{chain}", codecs, dt, shape, out_shape, descs, variants, ["A", "B", "A", "C", "B", "D", "A"],
                  modes=dict(PATHS))


# ---------------------------------------------------------------------------------------------------
# blosc: chunks of 16384 bytes (8192 uint16), padded by slack after cbytes
# ---------------------------------------------------------------------------------------------------
BL_N, BL_K = 16384, 4


def _blosc_codec(cname):
    return {"name": "blosc", "configuration": {"cname": cname, "clevel": 5, "shuffle": "shuffle", "typesize": 2, "blocksize": 0}}


def _blosc_family(name, cname, cases: dict, script, **kw):
    """cases: {variant: [(frame, the chunk's bytes or None)]}"""
    encs = _pad_to({v: [f for f, _ in c] for v, c in cases.items()}, lambda e, n: e + bytes(n - len(e)))
    variants = {}
    for v, c in cases.items():
        exp = [None if d is None else np.frombuffer(d, "<u2") for _, d in c]
        variants[v] = Variant(v, encs[v], [OK if d is not None else CORRUPT_STREAM for _, d in c], exp)
    descs = [Desc((0,), (BL_N // 2,), (i * (BL_N // 2),)) for i in range(BL_K)]
    return Family(name, [BYTES_LE, _blosc_codec(cname)], "uint16", (BL_N // 2,), (BL_K * BL_N // 2,), descs, variants, list(script), **kw)


def blosc_zstd_cases():
    """{variant: [blosc_inner_streams.Case]}: A with aliased raw / RLE / literal blocks, B with none, C: B with
    one stream that decodes to a byte less than its split (blosc_inner_streams' sizes family, at this size)"""
    import blosc_inner_streams as I
    planes = {c.id: c for c in I.family("alias_planes")}
    A = [planes[f"planes_ts2_{n}"] for n in ("on_plane_raw", "two_planes_rle", "mid_to_mid_lit_raw", "inside_plane_lit_huf")]
    plain = lambda i: I._shuffled_case(f"replay_plain_{i}", "replay", I.zstream(BL_N, [], 900 + i), 2, BL_N, {})  # noqa: E731
    B = [plain(i) for i in range(BL_K)]
    bad = I.make("replay_short_stream", "replay", [[I._sized("zstd", BL_N - 1, 77)]], comp=I.ZSTD, ts=2, bs=BL_N, nbytes=BL_N, mode=1)
    C = [B[0], B[1], bad, B[3]]
    return {"A": A, "B": B, "C": C}


@functools.lru_cache(maxsize=None)
def blosc_zstd():
    cases = blosc_zstd_cases()
    return _blosc_family("blosc_zstd", "zstd", {v: [(c.frame, c.expect) for c in cs] for v, cs in cases.items()}, ["A", "B", "C", "A"])


@functools.lru_cache(maxsize=None)
def blosc_lz4():
    """Direct rows (one row of 16384 bytes per chunk): one block, then four blocks (the stream table grows),
    then one block of other contents."""
    import blosc_frames as B
    def frames(bs, seed):
        out = []
        for i in range(BL_K):
            fr, chunk, _ = B.grid_frame("lz4", BL_N, bs, 2, True, mode=1, seed=seed + i)
            out.append((fr.data, chunk))
        return out
    return _blosc_family("blosc_lz4", "lz4", {"A": frames(BL_N, 10), "B": frames(4096, 20), "C": frames(BL_N, 30)}, ["A", "B", "C", "A"])


# ---------------------------------------------------------------------------------------------------
# no stage: only the scatter runs; one descriptor is a missing chunk in every variant
# ---------------------------------------------------------------------------------------------------
def _no_stage(name, codecs, chunk, descs, out_shape, path):
    import oracle as O
    oc = O.OracleChain.from_metadata(codecs, "float32", fill_bytes("float32"), len(chunk))
    variants = {}
    for v, seed in (("A", 1), ("B", 2)):
        enc, exp = [], []
        for i, d in enumerate(descs):
            if d.null:
                enc.append(None)
                exp.append(fill_array(d.sel_shape, "float32"))
                continue
            a = _rng(100 * seed + i).standard_normal(chunk).astype(np.float32)
            e = oc.encode(a)
            assert len(e) == a.nbytes
            enc.append(e)
            exp.append(a[tuple(slice(s, s + n) for s, n in zip(d.sel_start, d.sel_shape))])
        variants[v] = Variant(v, enc, [OK] * len(descs), exp)
    return Family(name, codecs, "float32", tuple(chunk), tuple(out_shape), descs, variants, ["A", "B", "A", "B"], path=path)


@functools.lru_cache(maxsize=None)
def no_stage_tiled():
    c = (64, 64, 64)
    codecs = [{"name": "transpose", "configuration": {"order": [2, 1, 0]}}, {"name": "bytes", "configuration": {"endian": "big"}}]
    descs = [Desc((0, 0, 0), c, (64 * i, 0, 0), null=i == 1) for i in range(3)]
    return _no_stage("no_stage_tiled", codecs, c, descs, (192, 64, 64), (TILED_PERSISTENT, TILED))


@functools.lru_cache(maxsize=None)
def no_stage_rows():
    c = (8, 16, 32)
    descs = [Desc((1, 2, 3), (6, 11, 9), (8 * i + 1, 2, 3), null=i == 2) for i in range(4)]
    return _no_stage("no_stage_rows", [BYTES_LE], c, descs, (32, 16, 32), (ROWS, ROWS))


# ---------------------------------------------------------------------------------------------------
FAMILIES = {
    "shard_gzip_crc": shard_gzip_crc,
    "shard_gzip_crc_partial": shard_gzip_crc_partial,
    "shard_zlib": shard_zlib,
    "zstd_chunks_u8": lambda: zstd_chunks("u8"),
    "zstd_chunks_shuffle_u16": lambda: zstd_chunks("shuffle_u16"),
    "blosc_zstd": blosc_zstd,
    "blosc_lz4": blosc_lz4,
    "checksum_ranges_adler32": lambda: checksum_ranges("adler32"),
    "checksum_ranges_fletcher32": lambda: checksum_ranges("fletcher32"),
    "checksum_ranges_crc32c": lambda: checksum_ranges("crc32c"),
    "shard_bz2": shard_bz2,
    "nested": nested,
    "no_stage_tiled": no_stage_tiled,
    "no_stage_rows": no_stage_rows,
}
# the modes of every family by name, without building it (the model test holds this to Family.modes)
ZSTD_PATH_NAMES = ("latency", "window", "wave", "wave_dense", "serial")
MODE_NAMES = {f: ["default"] for f in FAMILIES}
MODE_NAMES.update({"shard_gzip_crc": list(GZ_MODES), "shard_gzip_crc_partial": list(GZ_MODES),
                   "zstd_chunks_u8": list(ZSTD_PATH_NAMES), "zstd_chunks_shuffle_u16": list(ZSTD_PATH_NAMES),
                   "shard_bz2": ["default", "rounds"]})
RUNS = [(f, m) for f in FAMILIES for m in MODE_NAMES[f]]  # (family, mode) of test_script


@functools.lru_cache(maxsize=None)
def family(name: str) -> Family:
    return FAMILIES[name]()
