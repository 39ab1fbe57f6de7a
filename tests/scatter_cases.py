"""The final decode stage (scatter.hip: bytes endianness + transpose + fused numcodecs.shuffle undo + fill
+ scatter of a selection) and its write-side mirror (encode.hip), as a numpy reference and a table of
cases, one per branch of the kernels. numpy only; no GPU.

The reference of the stage is a few lines: `encode_ref` writes a chunk through the chain, and the
expected decode of any selection is the matching slice of the array, the fill value where a chunk is
missing. test_scatter_cases_model.py holds `encode_ref` to the C oracle; test_gpu_scatter_cases.py and
test_gpu_encode_cases.py hold the kernels to it.

Array contents are random bytes viewed as the data type, so NaN payloads, denormals and bool bytes
other than 0 and 1 occur: a byte mover carries them unchanged, and every comparison is on bytes. The
fill value of every case is es distinct bytes, 0x11, 0x12, ...: a wrong replication or a fill swapped
by a big-endian chain (fill bytes are native order on the decode side) shows.
"""
from __future__ import annotations

import dataclasses
import functools
import struct
import zlib

import numpy as np

ROWS, TILED, GENERIC, TILED_PERSISTENT = range(4)  # zgpu_plan_scatter_path
PATH_NAMES = ["ROWS", "TILED", "GENERIC", "TILED_PERSISTENT"]
SENTINEL = 0xA5

# data type -> (numpy dtype the bytes are viewed as, element size, component size): chain.cpp's table.
# bfloat16 has no numpy dtype; its bytes are moved as uint16
TYPES = {
    "bool": ("|b1", 1, 1), "int8": ("<i1", 1, 1), "uint8": ("<u1", 1, 1),
    "int16": ("<i2", 2, 2), "uint16": ("<u2", 2, 2), "float16": ("<f2", 2, 2), "bfloat16": ("<u2", 2, 2),
    "int32": ("<i4", 4, 4), "uint32": ("<u4", 4, 4), "float32": ("<f4", 4, 4),
    "int64": ("<i8", 8, 8), "uint64": ("<u8", 8, 8), "float64": ("<f8", 8, 8),
    "complex64": ("<c8", 8, 4), "complex128": ("<c16", 16, 8),
}


def es_of(dt: str) -> int:
    return TYPES[dt][1]


def fill_bytes(dt: str) -> bytes:
    return bytes(range(0x11, 0x11 + es_of(dt)))


def encode_ref(a: np.ndarray, orders, endian: str, shuffle: bool, crc: str | None = None) -> bytes:
    """The chain written plainly: each transpose order in turn, every component in the requested byte
    order (complex types have two), numcodecs.shuffle over the element size, a crc32c at the start or
    the end."""
    es = a.dtype.itemsize
    comp = es // 2 if a.dtype.kind == "c" else es
    t = a.view(f"V{es}")  # elements as opaque bytes: nothing below may normalise a value
    for o in orders:
        t = np.transpose(t, o)
    b = np.ascontiguousarray(t).view(np.uint8).reshape(-1, es)
    if endian == "big" and comp > 1:
        b = b.reshape(-1, es // comp, comp)[:, :, ::-1].reshape(-1, es)
    if shuffle:
        b = b.T
    data = np.ascontiguousarray(b).tobytes()
    if crc:
        import oracle
        c = struct.pack("<I", oracle.crc32c(data))
        data = c + data if crc == "start" else data + c
    return data


def codecs_of(case) -> list:
    """The case's chain as zarr V3 codec metadata."""
    m = [{"name": "transpose", "configuration": {"order": list(o)}} for o in case.orders]
    m.append({"name": "bytes", "configuration": {"endian": case.endian}})
    if case.shuffle:
        m.append({"name": "numcodecs.shuffle", "configuration": {"elementsize": es_of(case.dtype)}})
    if case.crc:
        m.append({"name": "crc32c", "configuration": {"location": case.crc}})
    return m


def composed_axes(orders, nd: int) -> list:
    """m[a]: the decoded axis that encoded axis a runs along."""
    m = list(range(nd))
    for o in orders:
        m = [m[j] for j in o]
    return m


def model_path(case) -> int:
    """The kernel the plan builder picks for the chain (plan_layout.cpp, scatter_mode), restated."""
    nd = len(case.chunk)
    if composed_axes(case.orders, nd)[-1] == nd - 1:
        return ROWS
    if not case.shuffle and es_of(case.dtype) in (1, 2, 4, 8):
        return TILED
    return GENERIC


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    group: str
    dtype: str
    orders: tuple       # transpose orders, applied in turn
    endian: str         # "little" | "big"
    shuffle: bool       # numcodecs.shuffle with elementsize = the element size (fused into the scatter)
    crc: str | None     # crc32c location: None | "start" | "end"
    chunk: tuple
    array: tuple
    sels: tuple         # ((start, shape), ...) in array coordinates
    drop: frozenset     # missing chunks (grid indices): decoded as the fill value
    src_off: int        # device source: bytes past a 16-byte-aligned buffer start
    path: int           # expected zgpu_plan_scatter_path
    wide: str | None    # ZGPU_UNSHUFFLE_WIDE while the chain and the plan are created (None: unset)
    note: str           # the branch the case is there for

    @property
    def grid(self):
        return tuple(-(-s // c) for s, c in zip(self.array, self.chunk))


def _seed(name: str) -> int:
    return zlib.crc32(name.encode())


def random_array(name: str, dt: str, shape) -> np.ndarray:
    """Random bytes viewed as the data type (read-only)."""
    es = es_of(dt)
    raw = np.random.default_rng(_seed(name)).integers(0, 256, int(np.prod(shape)) * es, np.uint8)
    a = raw.view(np.dtype(TYPES[dt][0])).reshape(shape)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def case_data(name: str):
    """(array, reference array with the missing chunks filled, {grid index: encoded chunk}) of a case,
    computed once and never changed."""
    c = BY_NAME[name]
    a = random_array(name, c.dtype, c.array)
    ref = a.copy()
    fv = np.frombuffer(fill_bytes(c.dtype), dtype=f"V{es_of(c.dtype)}")[0]
    chunks = {}
    for k in np.ndindex(*c.grid):
        box = tuple(slice(i * n, (i + 1) * n) for i, n in zip(k, c.chunk))
        if k in c.drop:
            ref.view(fv.dtype)[box] = fv
        else:
            chunks[k] = encode_ref(a[box], c.orders, c.endian, c.shuffle, c.crc)
    ref.flags.writeable = False
    return a, ref, chunks


def expected(name: str, start, shape) -> bytes:
    """The bytes of the selection [start, start + shape): a slice of the reference array."""
    ref = case_data(name)[1]
    return np.ascontiguousarray(ref[tuple(slice(s, s + n) for s, n in zip(start, shape))]).tobytes()


# ---- the table --------------------------------------------------------------------------------------
CASES: list = []


def _add(group, note, dt, chunk, array=None, sels=None, *, orders=(), endian="little", shuffle=False, crc=None,
         drop=(), src_off=0, path=ROWS, wide=None):
    array = tuple(array if array is not None else chunk)
    sels = tuple((tuple(s), tuple(n)) for s, n in (sels or [([0] * len(array), array)]))
    tag = [group, dt, endian[0] + "e", "x".join(map(str, chunk))]
    tag += ["t" + "".join(map(str, o)) for o in orders]
    tag += (["shuf"] if shuffle else []) + ([f"crc{crc}"] if crc else []) + ([f"off{src_off}"] if src_off else [])
    tag += [f"wide{wide or 'unset'}"] if group == "unshuffle-wide" else []
    name = "-".join(tag)
    assert all(c.name != name for c in CASES), name
    CASES.append(Case(name, group, dt, tuple(tuple(o) for o in orders), endian, shuffle, crc, tuple(chunk), array,
                      sels, frozenset(tuple(k) for k in drop), src_off, path, wide, f"{note} [{dt}, {endian}]"))


def _inner(sh):
    """The selection one element inside every face of the array."""
    return [1] * len(sh), [s - 2 for s in sh]


def _swap(dt, endian):
    es, comp = TYPES[dt][1:]
    if endian == "little" or comp == 1:
        return "bytes unchanged"
    return f"{comp}-byte components reversed" + (" (two per element)" if comp != es else "")


def _lv(dt):
    """Shortest row of whole 16-byte vectors with at least two elements."""
    return max(16 // es_of(dt), 2)


def _build():
    for dt in TYPES:
        es = es_of(dt)
        L = _lv(dt)
        # rows-vec: whole chunks of 16-B aligned rows, one chunk missing (the replicated fill vector)
        for endian, k in (("little", 1), ("big", 2)):
            Lk = L * k
            _add("rows-vec", f"k_scatter_rows, 16-B vector rows of {Lk * es // 16} vectors, {_swap(dt, endian)} "
                 f"(swap_vec); fill vector P.fill[i % {es}] for the missing chunk", dt, [3, 5, Lk], [6, 10, 2 * Lk],
                 endian=endian, drop=[(1, 1, 1)])
        # rows-elem
        sh = [6, 10, 2 * L]
        what = ("rows stay 16-B aligned at es 16: vector path on rows that start inside the chunk" if es == 16 else
                "element path, rows start and end inside the chunk's rows")
        _add("rows-elem", f"k_scatter_rows, selection one element inside the array: {what}, {_swap(dt, 'big')}",
             dt, [3, 5, L], sh, [_inner(sh)], endian="big")
        for Lo, endian in ((5, "little"), (7, "big")):
            what = "rows of whole 16-B elements: vector path" if es == 16 else "row bytes no multiple of 16: element path"
            _add("rows-elem", f"k_scatter_rows, rows of {Lo} elements, {what}, {_swap(dt, endian)}; element fill "
                 "for the missing chunk", dt, [3, 5, Lo], [6, 10, 2 * Lo], endian=endian, drop=[(0, 1, 1)])
        for off in (1, 2, 4, 8):
            al = "aligned" if off % min(es, 8) == 0 and es in (2, 4, 8) else "byte-wise"
            _add("rows-elem", f"k_scatter_rows element path, source {off} bytes past a 16-B boundary: load_elem "
                 f"{al} at es {es}, {_swap(dt, 'big')}", dt, [3, 5, L], endian="big", src_off=off)
        _add("rows-elem", "k_scatter_rows element path, source 4 bytes into its buffer behind crc32c at the start",
             dt, [3, 5, L], [6, 10, 2 * L], crc="start")
    _add("rows-vec", "k_scatter_rows, transpose [1,0,2] keeps the innermost axis: rows at permuted encoded strides, "
         "vector path", "float32", [3, 5, 4], [6, 10, 8], orders=[[1, 0, 2]], endian="big")
    _add("rows-elem", "k_scatter_rows, transposes [1,0,2] then [1,0,2] compose to the identity", "int16", [3, 5, 7],
         [6, 10, 14], [_inner([6, 10, 14])], orders=[[1, 0, 2], [1, 0, 2]], endian="big")

    # rows-groups: 65 rows = one full group of 64 and a group of one
    for dt in ("uint8", "float32", "complex128"):
        for endian in ("little", "big"):
            L = _lv(dt)
            _add("rows-groups", f"k_scatter_rows, 65 rows per item: a 64-row group and a ragged group of one, "
                 f"{_swap(dt, endian)}", dt, [5, 13, L], [10, 13, L], endian=endian)

    # rank 1 and rank ZG_MAXD
    for dt, endian in (("uint16", "big"), ("float64", "little")):
        other = "little" if endian == "big" else "big"
        _add("rank", "k_scatter_rows rank 1, one row of 257 elements per item, whole and from element 1", dt, [257],
             [514], [([0], [514]), ([1], [512])], endian=endian)
        _add("rank", "k_scatter_rows rank 1, one row of 256 elements per item (whole vectors), whole and from element 1",
             dt, [256], [512], [([0], [512]), ([1], [510])], endian=other)
        c8, a8 = [2, 1, 2, 1, 2, 1, 3, 4], [4, 1, 2, 1, 2, 1, 3, 8]
        s8 = [([0] * 8, a8), ([1, 0, 0, 0, 1, 0, 1, 1], [2, 1, 2, 1, 1, 1, 2, 6])]
        _add("rank", "k_scatter_rows rank 8 (ZG_MAXD), whole and a partial selection across chunks", dt, c8, a8, s8,
             endian=endian)
        _add("rank", "k_scatter_rows rank 8 under transpose [6,5,4,3,2,1,0,7]: outer encoded strides reversed", dt,
             c8, a8, s8, orders=[[6, 5, 4, 3, 2, 1, 0, 7]], endian=other)

    # unshuffle-vec: fused unshuffle, 8-byte (es 2) / 4-byte (es 4) plane loads
    for dt in ("int16", "float16", "uint32", "float32"):
        es = es_of(dt)
        L = 32 // es
        for endian in ("little", "big"):
            how = ("planes 0 and 1 " + ("exchanged" if endian == "big" else "in order") if es == 2 else
                   "4x4 byte transpose" + (" then swap_word" if endian == "big" else ""))
            _add("unshuffle-vec", f"k_scatter_rows fused unshuffle, vec_ok: {16 // es} elements per 16-B store from "
                 f"{16 // es}-byte plane loads, {how}; whole rows, whole and from row 1", dt, [3, 5, L],
                 [6, 10, 2 * L], [([0, 0, 0], [6, 10, 2 * L]), ([1, 1, 0], [4, 8, 2 * L])], endian=endian,
                 shuffle=True, drop=[(1, 0, 1)])

    # unshuffle-wide: the u16 16-B plane loads of ZGPU_UNSHUFFLE_WIDE
    for dt in ("uint16", "int16"):
        for endian in ("little", "big"):
            for wide in (None, "1", "2"):
                mode = {None: "unset: 8-B plane loads", "1": "1: non-temporal 16-B plane loads and stores",
                        "2": "2: plain 16-B plane loads and stores"}[wide]
                sel = "lo/hi planes " + ("exchanged" if endian == "big" else "in order")
                _add("unshuffle-wide", f"k_scatter_rows fused u16 unshuffle, ZGPU_UNSHUFFLE_WIDE {mode}, rows of "
                     f"two 16-element units, {sel}", dt, [3, 5, 32], [6, 10, 64], endian=endian, shuffle=True,
                     wide=wide, drop=[(0, 0, 1)])
                _add("unshuffle-wide", f"k_scatter_rows fused u16 unshuffle, ZGPU_UNSHUFFLE_WIDE {mode}, rows of 8 "
                     f"elements: wide refused, 8-B plane loads, {sel}", dt, [3, 5, 8], [6, 10, 16], endian=endian,
                     shuffle=True, wide=wide)
                if wide:
                    _add("unshuffle-wide", f"k_scatter_rows fused u16 unshuffle, ZGPU_UNSHUFFLE_WIDE {mode}, 320 "
                         f"units in a 64-row group: a thread's second unit in flight, and a ragged group, {sel}",
                         dt, [5, 13, 80], endian=endian, shuffle=True, wide=wide)

    # unshuffle-elem: every way vec_ok fails, and the element sizes that have no vector form
    U = "unshuffle-elem"
    for dt, endian in (("uint16", "little"), ("uint16", "big"), ("float32", "big")):
        _add(U, f"k_scatter_rows fused unshuffle, rows of 7 elements and an odd nelem (105): vec_ok fails on the row "
             f"length, element path, {_swap(dt, endian)}", dt, [3, 5, 7], [6, 10, 14], endian=endian, shuffle=True,
             drop=[(1, 1, 0)])
    _add(U, "k_scatter_rows fused unshuffle, rows of 8 of a chunk of 180 elements: vec_ok fails on nelem % 8", "uint16",
         [3, 5, 12], sels=[([0, 0, 0], [3, 5, 8])], endian="big", shuffle=True)
    _add(U, "k_scatter_rows fused unshuffle, rows of 16 from element 1: vec_ok fails on the per-row plane offset",
         "uint16", [3, 5, 24], sels=[([0, 0, 1], [3, 5, 16])], shuffle=True)
    _add(U, "k_scatter_rows fused unshuffle, rows of 8 from element 1: vec_ok fails on the per-row plane offset, "
         "swap_word skipped for the byte loop", "float32", [3, 5, 12], sels=[([0, 0, 1], [3, 5, 8])], endian="big",
         shuffle=True)
    _add(U, "k_scatter_rows fused unshuffle behind crc32c at the start: vec_ok fails on src & 15 (source + 4)",
         "uint16", [3, 5, 16], [6, 10, 32], endian="big", shuffle=True, crc="start")
    _add(U, "k_scatter_rows fused unshuffle behind crc32c at the start: vec_ok fails on src & 15 (source + 4)",
         "float32", [3, 5, 8], [6, 10, 16], shuffle=True, crc="start")
    _add(U, "k_scatter_rows fused unshuffle, source 8 bytes past a 16-B boundary: plane loads would be aligned, "
         "vec_ok still fails on src & 15", "int16", [3, 5, 16], endian="big", shuffle=True, src_off=8)
    _add(U, "k_scatter_rows fused unshuffle at es 1 (one plane, the identity): element path", "uint8", [3, 5, 7],
         [6, 10, 14], shuffle=True, drop=[(0, 0, 1)])
    for endian in ("little", "big"):
        sh = [6, 10, 14]
        _add(U, f"k_scatter_rows fused unshuffle at es 8: element path, byte loop, {_swap('float64', endian)}; whole "
             "and from an odd element", "float64", [3, 5, 7], sh, [([0] * 3, sh), _inner(sh)], endian=endian,
             shuffle=True)
        _add(U, f"k_scatter_rows fused unshuffle at es 16: element path over 16 planes, {_swap('complex128', endian)}"
             " (c0 += comp)", "complex128", [3, 5, 7], sh, [([0] * 3, sh), _inner(sh)], endian=endian, shuffle=True,
             drop=[(1, 1, 1)])
    _add(U, "k_scatter_rows fused unshuffle at es 8, comp 4: the c0 += comp loop reverses two components", "complex64",
         [3, 5, 7], [6, 10, 14], [([0] * 3, [6, 10, 14]), _inner([6, 10, 14])], endian="big", shuffle=True)
    _add(U, "k_scatter_rows fused unshuffle at es 8, comp 4, behind crc32c at the start", "complex64", [3, 5, 8],
         endian="big", shuffle=True, crc="start")

    # tiled-small: k_scatter_tiled, never the persistent form (ragged tiles or partial selections)
    for dt in ("int8", "float16", "bfloat16", "uint32", "int64", "complex64"):
        es = es_of(dt)
        sh = [10, 6, 14]
        _add("tiled-small", f"k_scatter_tiled<{es}> order [2,1,0], one ragged 5x7 tile per slab group: element loads "
             f"and stores, {_swap(dt, 'big')}; whole, one element inside, a missing chunk", dt, [5, 3, 7], sh,
             [([0] * 3, sh), _inner(sh)], orders=[[2, 1, 0]], endian="big", drop=[(1, 0, 1)], path=TILED)
        sh = [64, 6, 128]
        _add("tiled-small", f"k_scatter_tiled<{es}> order [2,1,0], full 64x64 tiles of partly selected chunks: 16-B "
             f"loads and (on aligned output rows) stores, {_swap(dt, 'big')} (swap_vec); one element inside: ragged "
             "tiles; a missing chunk: vector fill", dt, [64, 3, 64], sh, [([0, 1, 0], [64, 4, 128]), _inner(sh)],
             orders=[[2, 1, 0]], endian="big", drop=[(0, 1, 1)], path=TILED)
        sh = [18, 140]
        _add("tiled-small", f"k_scatter_tiled<{es}> rank 2 order [1,0] (no slab axis), two tiles along the output "
             "row, the second ragged", dt, [9, 70], sh, [([0] * 2, sh), _inner(sh)], orders=[[1, 0]], path=TILED)

    for dt, off in (("float16", 1), ("complex64", 4)):
        _add("tiled-small", f"k_scatter_tiled<{es_of(dt)}> order [2,1,0], source {off} bytes past a 16-B boundary: "
             "load_elem byte-wise from an address that is no multiple of the element size", dt, [5, 3, 7],
             orders=[[2, 1, 0]], endian="big", src_off=off, path=TILED)
    for dt in ("uint32", "int64"):
        _add("tiled-small", f"k_scatter_tiled<{es_of(dt)}> order [2,1,0] behind crc32c at the start: source + 4, "
             "element loads", dt, [5, 3, 7], [10, 6, 14], orders=[[2, 1, 0]], endian="big", crc="start", path=TILED)
    # orders that are not their own inverse: an order applied the wrong way round shows
    sh = [10, 6, 14]
    _add("tiled-small", "k_scatter_tiled<2> order [1,2,0] (not its own inverse): tile axis 0, slab axis 1", "float16",
         [5, 3, 7], sh, [([0] * 3, sh), _inner(sh)], orders=[[1, 2, 0]], endian="big", drop=[(0, 1, 0)], path=TILED)
    _add("tiled-small", "k_scatter_tiled<8> orders [1,2,0] twice, composed to [2,0,1]: tile axis 1", "int64", [5, 3, 7],
         sh, [([0] * 3, sh), _inner(sh)], orders=[[1, 2, 0], [1, 2, 0]], endian="big", path=TILED)
    _add("generic", "k_scatter_generic, es 16 under order [2,0,1] (not its own inverse)", "complex128", [5, 3, 7], sh,
         [([0] * 3, sh), _inner(sh)], orders=[[2, 0, 1]], endian="big", drop=[(1, 0, 1)], path=GENERIC)
    _add("rows-elem", "k_scatter_rows, orders [1,2,0] then [2,0,1] compose to the identity", "uint32", [3, 5, 7],
         [6, 10, 14], [_inner([6, 10, 14])], orders=[[1, 2, 0], [2, 0, 1]], endian="big")
    _add("rows-vec", "k_scatter_rows rank 4 under order [2,0,1,3] (not its own inverse, innermost axis kept): vector "
         "rows at permuted encoded strides", "float32", [2, 3, 5, 4], [4, 3, 10, 8], orders=[[2, 0, 1, 3]],
         endian="big", drop=[(1, 0, 1, 0)])
    _add("unshuffle-wide", "k_scatter_rows fused unshuffle at es 4 with ZGPU_UNSHUFFLE_WIDE 1: the switch is for "
         "u16 only, 4-byte plane loads as without it", "float32", [3, 5, 16], [6, 10, 32], endian="big",
         shuffle=True, wide="1")

    # generic: 16-byte elements under a transpose, and the fused unshuffle under a transpose
    sh = [10, 12, 18]
    for endian in ("little", "big"):
        _add("generic", f"k_scatter_generic, es 16 under order [2,1,0] (two blocks per item): load_elem / store_elem "
             f"byte paths, {_swap('complex128', endian)}; whole, one element inside, 16-byte fill", "complex128",
             [5, 6, 9], sh, [([0] * 3, sh), _inner(sh)], orders=[[2, 1, 0]], endian=endian, drop=[(1, 1, 0)],
             path=GENERIC)
    for dt, endian in (("uint16", "big"), ("float32", "little"), ("float32", "big"), ("float64", "big"),
                       ("complex64", "big")):
        _add("generic", f"k_scatter_generic, fused unshuffle under order [2,1,0] at es {es_of(dt)}: plane gather at "
             f"the transposed offset, {_swap(dt, endian)}; whole, one element inside, fill", dt, [5, 6, 9], sh,
             [([0] * 3, sh), _inner(sh)], orders=[[2, 1, 0]], endian=endian, shuffle=True, drop=[(0, 1, 1)],
             path=GENERIC)


_build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the (group, type) cells that must each hold at least one case
ALL = list(TYPES)
CELLS = {
    "rows-vec": ALL, "rows-elem": ALL, "rows-groups": ["uint8", "float32", "complex128"],
    "rank": ["uint16", "float64"], "unshuffle-vec": ["int16", "float16", "uint32", "float32"],
    "unshuffle-wide": ["uint16", "int16"], "unshuffle-elem": ["uint8", "float64", "complex64", "complex128"],
    "tiled-small": ["int8", "float16", "bfloat16", "uint32", "int64", "complex64"],
    "generic": ["complex128", "uint16", "float32", "float64"],
}


# ---- the write side: the same chains over arrays whose edge chunks cross the array's end -------------
def encode_cases() -> list:
    """One case per distinct (type, chain, chunk shape) of the table."""
    seen, out = set(), []
    for c in CASES:
        k = (c.dtype, c.orders, c.endian, c.shuffle, c.crc, c.chunk)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


def encode_array_shapes(chunk) -> list:
    """[c0 + 1, c1 + 2, ..., 2 * c_last - 1]: a grid with an edge of every kind (one row past a chunk, two
    past, one short of two chunks), and odd rows, so nothing in the array is 16-byte aligned; then the
    same with rows of 2 * c_last, on which the tiled encoder's 16-byte loads run."""
    sh = list(chunk)
    if len(sh) > 1:
        sh[0] = chunk[0] + 1
    if len(sh) > 2:
        sh[1] = chunk[1] + 2
    return [sh[:-1] + [max(1, 2 * chunk[-1] - 1)], sh[:-1] + [2 * chunk[-1]]]


def padded_chunk(a: np.ndarray, dt: str, chunk, start) -> np.ndarray:
    """The chunk at `start` of the array as the writer encodes it: the fill value past the array's end."""
    es = es_of(dt)
    blk = np.empty(chunk, dtype=f"V{es}")
    blk[...] = np.frombuffer(fill_bytes(dt), dtype=f"V{es}")[0]
    src = a.view(f"V{es}")[tuple(slice(s, min(s + c, n)) for s, c, n in zip(start, chunk, a.shape))]
    blk[tuple(slice(0, n) for n in src.shape)] = src
    return blk.view(a.dtype)
