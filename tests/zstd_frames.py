"""Zstandard frames the library's own encoder never makes, for the GPU decoder's tests: a builder and
a reference executor in plain Python (no GPU, no oracle), and the test cases made with them.

Two sources of frames:

(a) streaming frames from libzstd through ctypes (ZSTD_compressStream2 with ZSTD_e_flush every F
    bytes: every flush closes a block, so a chunk becomes many tiny blocks that reference each other);
(b) hand-assembled frames (RFC 8878): any frame header form, raw / RLE / compressed blocks, raw or
    RLE literals, and a sequence section whose three tables are in RLE mode (modes byte 0x54 and one
    code each), so the FSE states take no bits and the bitstream holds only each sequence's extra bits.

execute() is the reference: it runs (literals, ll, ml, offset_value) lists with the repeat-offset rules
of RFC 8878 3.1.1.5. tests/test_zstd_frames_model.py checks every case against libzstd's own
ZSTD_decompress; tests/test_gpu_zstd_frames.py decodes the same cases on the GPU.
"""
from __future__ import annotations

import ctypes as C
import functools
import struct
from dataclasses import dataclass, field

import numpy as np

MAGIC = 0xFD2FB528
RAW, RLE, CMP = 0, 1, 2
BLOCK_MAX = 131072

# ---------------------------------------------------------------------------------------------------
# libzstd through ctypes
# ---------------------------------------------------------------------------------------------------
ZSTD_c_compressionLevel, ZSTD_c_windowLog, ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 100, 101, 200, 201
ZSTD_e_continue, ZSTD_e_flush, ZSTD_e_end = 0, 1, 2


class _InBuf(C.Structure):
    _fields_ = [("src", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


class _OutBuf(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


@functools.lru_cache(maxsize=None)
def libzstd() -> C.CDLL:
    z = C.CDLL("libzstd.so.1")
    z.ZSTD_createCCtx.restype = C.c_void_p
    z.ZSTD_freeCCtx.argtypes = [C.c_void_p]
    z.ZSTD_CCtx_setParameter.restype = C.c_size_t
    z.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
    z.ZSTD_CCtx_setPledgedSrcSize.restype = C.c_size_t
    z.ZSTD_CCtx_setPledgedSrcSize.argtypes = [C.c_void_p, C.c_ulonglong]
    z.ZSTD_compressStream2.restype = C.c_size_t
    z.ZSTD_compressStream2.argtypes = [C.c_void_p, C.POINTER(_OutBuf), C.POINTER(_InBuf), C.c_int]
    z.ZSTD_compressBound.restype = C.c_size_t
    z.ZSTD_compressBound.argtypes = [C.c_size_t]
    z.ZSTD_isError.restype = C.c_uint
    z.ZSTD_isError.argtypes = [C.c_size_t]
    z.ZSTD_getErrorName.restype = C.c_char_p
    z.ZSTD_getErrorName.argtypes = [C.c_size_t]
    z.ZSTD_decompress.restype = C.c_size_t
    z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    return z


def _ok(rc: int) -> int:
    z = libzstd()
    if z.ZSTD_isError(rc):
        raise RuntimeError(z.ZSTD_getErrorName(rc).decode())
    return rc


def zstd_decompress(frames: bytes, n: int) -> bytes:
    """ZSTD_decompress of `frames` (one or more frames) into a buffer of n bytes."""
    buf = C.create_string_buffer(max(n, 1))
    got = _ok(libzstd().ZSTD_decompress(buf, n, frames, len(frames)))
    return buf.raw[:got]


def stream_frame(data: bytes, flush: int, *, level: int = 3, pledged: bool = True, checksum: bool = False,
                 window_log: int = 0, end_empty: bool = False) -> bytes:
    """One frame from ZSTD_compressStream2: `flush` bytes of input per call, ZSTD_e_flush after each
    (flush = 0: one ZSTD_e_end call). pledged: the content size is announced (a single-segment frame
    with a content-size field); else the frame has a window descriptor and no content size.
    end_empty: every byte is flushed first and the frame is ended with no input left, which appends an
    empty raw last block."""
    z = libzstd()
    cctx = z.ZSTD_createCCtx()
    try:
        _ok(z.ZSTD_CCtx_setParameter(cctx, ZSTD_c_compressionLevel, level))
        _ok(z.ZSTD_CCtx_setParameter(cctx, ZSTD_c_checksumFlag, int(checksum)))
        if window_log:
            _ok(z.ZSTD_CCtx_setParameter(cctx, ZSTD_c_windowLog, window_log))
        if pledged:
            _ok(z.ZSTD_CCtx_setPledgedSrcSize(cctx, len(data)))
        else:
            _ok(z.ZSTD_CCtx_setParameter(cctx, ZSTD_c_contentSizeFlag, 0))
        src = C.create_string_buffer(data, max(len(data), 1))
        cap = z.ZSTD_compressBound(len(data)) + 16 * (len(data) // max(flush, 1) + 2) + 64
        dst = C.create_string_buffer(cap)
        ob = _OutBuf(C.cast(dst, C.c_void_p), cap, 0)
        pos, step = 0, flush or len(data)
        while pos < len(data):
            n = min(step, len(data) - pos)
            ib = _InBuf(C.cast(src, C.c_void_p).value + pos, n, 0)
            final = pos + n == len(data) and not end_empty
            op = ZSTD_e_end if final else ZSTD_e_flush
            while True:
                left = _ok(z.ZSTD_compressStream2(cctx, C.byref(ob), C.byref(ib), op))
                if left == 0 and ib.pos == n:
                    break
            pos += n
        if end_empty or not data:
            ib = _InBuf(C.cast(src, C.c_void_p), 0, 0)
            while _ok(z.ZSTD_compressStream2(cctx, C.byref(ob), C.byref(ib), ZSTD_e_end)):
                pass
        return dst.raw[:ob.pos]
    finally:
        z.ZSTD_freeCCtx(cctx)


# ---------------------------------------------------------------------------------------------------
# walking a frame
# ---------------------------------------------------------------------------------------------------
def _frame_header_len(buf: bytes, p: int):
    """(header bytes after the magic, has_checksum) of the frame whose magic is at p."""
    fhd = buf[p + 4]
    single, fcs_flag, did = (fhd >> 5) & 1, fhd >> 6, fhd & 3
    n = 1 + (0 if single else 1) + (4 if did == 3 else did)
    n += (1 if single else 0) if fcs_flag == 0 else (2, 4, 8)[fcs_flag - 1]
    return n, bool(fhd & 4)


def walk(buf: bytes):
    """The blocks of every zstd frame of buf, one list per frame (skippable frames are passed over):
    (type, size field, payload offset, payload length)."""
    out, p = [], 0
    while p < len(buf):
        magic = struct.unpack_from("<I", buf, p)[0]
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            p += 8 + struct.unpack_from("<I", buf, p + 4)[0]
            continue
        assert magic == MAGIC, hex(magic)
        n, ck = _frame_header_len(buf, p)
        p += 4 + n
        blks = []
        while True:
            bh = buf[p] | buf[p + 1] << 8 | buf[p + 2] << 16
            p += 3
            btype, size = (bh >> 1) & 3, bh >> 3
            plen = size if btype != RLE else 1
            blks.append((btype, size, p, plen))
            p += plen
            if bh & 1:
                break
        p += 4 if ck else 0
        out.append(blks)
    assert p == len(buf)
    return out


def blocks(frame: bytes):
    """(type, size) of every block of the frame(s), in order (size: the block header's field: the
    decoded size of a raw / RLE block, the encoded size of a compressed one)."""
    return [(t, s) for f in walk(frame) for t, s, _, _ in f]


def literal_types(frame: bytes):
    """Literals_Block_Type (0 raw, 1 RLE, 2 Huffman, 3 treeless) of every compressed block."""
    return [frame[o] & 3 for f in walk(frame) for t, _, o, _ in f if t == CMP]


def sections(frame: bytes):
    """(literals type, regenerated literals size, number of sequences) of every compressed block."""
    out = []
    for f in walk(frame):
        for t, _, o, _ in f:
            if t != CMP:
                continue
            ltype, sf = frame[o] & 3, (frame[o] >> 2) & 3
            v = int.from_bytes(frame[o:o + 5], "little")
            if ltype <= 1:
                h = (1, 2, 1, 3)[sf]
                regen = (v & (1 << 8 * h) - 1) >> (3 if h == 1 else 4)
                q = o + h + (regen if ltype == 0 else 1)
            else:
                h, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
                regen, csize = (v >> 4) & (1 << bits) - 1, (v >> (4 + bits)) & (1 << bits) - 1
                q = o + h + csize
            c0 = frame[q]
            nseq = c0 if c0 < 128 else ((c0 - 128) << 8) + frame[q + 1] if c0 < 255 \
                else (frame[q + 1] | frame[q + 2] << 8) + 0x7F00
            out.append((ltype, regen, nseq))
    return out


def sequence_counts(frame: bytes):
    """Number_of_Sequences of every compressed block."""
    return [n for _, _, n in sections(frame)]


# ---------------------------------------------------------------------------------------------------
# hand-assembled frames
# ---------------------------------------------------------------------------------------------------
# (baseline, extra bits) per code, RFC 8878 3.1.1.3.2.1.1
LL_CODES = [(i, 0) for i in range(16)] + [(16, 1), (18, 1), (20, 1), (22, 1), (24, 2), (28, 2), (32, 3), (40, 3),
                                            (48, 4), (64, 6), (128, 7), (256, 8), (512, 9), (1024, 10), (2048, 11),
                                            (4096, 12), (8192, 13), (16384, 14), (32768, 15), (65536, 16)]
ML_CODES = [(i + 3, 0) for i in range(32)] + [(35, 1), (37, 1), (39, 1), (41, 1), (43, 2), (47, 2), (51, 3), (59, 3),
                                                (67, 4), (83, 4), (99, 5), (131, 7), (259, 8), (515, 9), (1027, 10),
                                                (2051, 11), (4099, 12), (8195, 13), (16387, 14), (32771, 15),
                                                (65539, 16)]
assert len(LL_CODES) == 36 and len(ML_CODES) == 53


def _code_of(table, v):
    for c in range(len(table) - 1, -1, -1):
        if table[c][0] <= v:
            assert v - table[c][0] < (1 << table[c][1]) or (table[c][1] == 0 and v == table[c][0]), v
            return c
    raise ValueError(v)


@dataclass
class Block:
    """One block of a hand-built frame. kind RAW: data; RLE: data[0] repeated n times; CMP: literals
    (`lits`, or an RLE literals section of lit_rle = (byte, count)) and seqs = [(ll, ml, offset_value)],
    all of whose lengths share one LL code and one ML code and whose offset values share one offset code
    (the RLE table modes). lit_hdr / nseq_hdr force the size of the literals header (1, 2, 3 bytes) and
    of the sequence count (1, 2, 3 bytes); 0: the shortest. huf ('tree' or 'treeless'): `lits`, bytes of
    value 0 or 1 only and at most 1023 of them, are Huffman-coded in one stream with the two-symbol tree
    of one bit per symbol (its description in the block, or the previous block's tree reused)."""
    kind: int
    data: bytes = b""
    n: int = 0
    lits: bytes = b""
    lit_rle: tuple | None = None
    seqs: list = field(default_factory=list)
    lit_hdr: int = 0
    nseq_hdr: int = 0
    huf: str = ""

    def literals(self) -> bytes:
        return bytes([self.lit_rle[0]]) * self.lit_rle[1] if self.lit_rle else self.lits


def raw(data: bytes) -> Block:
    return Block(RAW, data=bytes(data))


def rle(byte: int, n: int) -> Block:
    return Block(RLE, data=bytes([byte]), n=n)


def cmp_block(lits=b"", seqs=(), *, lit_rle=None, lit_hdr=0, nseq_hdr=0, huf="") -> Block:
    return Block(CMP, lits=bytes(lits), lit_rle=lit_rle, seqs=list(seqs), lit_hdr=lit_hdr, nseq_hdr=nseq_hdr, huf=huf)


@dataclass
class Frame:
    """header: 'fcs1' | 'fcs2' | 'fcs4' | 'fcs8' (single segment, content size of that many bytes) or
    'window' (no content size, a window descriptor of 2^window_log bytes)."""
    blocks: list
    header: str = "fcs4"
    window_log: int = 17


def _huffman_literals(b: Block) -> bytes:
    """Huffman literals, one stream (size format 0). The tree: direct weights, header byte 127 + 1, the
    weight of symbol 0 (1) in the high nibble; symbol 1's weight follows from the sum: both codes one
    bit, symbol 0 -> 0. The stream is read backwards like the sequences': 0..0 1 <symbol 0> <symbol 1> .."""
    n = len(b.lits)
    assert 0 < n < 1024 and set(b.lits) <= {0, 1} and b.huf in ("tree", "treeless")
    v = 1
    for x in b.lits:
        v = v << 1 | x
    stream = v.to_bytes((n + 1 + 7) // 8, "little")
    tree = bytes([128, 0x10]) if b.huf == "tree" else b""
    csize = len(tree) + len(stream)
    ltype = 2 if b.huf == "tree" else 3
    return struct.pack("<I", ltype | n << 4 | csize << 14)[:3] + tree + stream


def _literals_section(b: Block) -> bytes:
    if b.huf:
        return _huffman_literals(b)
    n = b.lit_rle[1] if b.lit_rle else len(b.lits)
    ltype = 1 if b.lit_rle else 0
    h = b.lit_hdr or (1 if n < 32 else 2 if n < 4096 else 3)
    assert n < (32, 4096, 1 << 20)[h - 1]
    if h == 1:
        hdr = bytes([ltype | n << 3])
    elif h == 2:
        hdr = struct.pack("<H", ltype | 1 << 2 | n << 4)
    else:
        hdr = struct.pack("<I", ltype | 3 << 2 | n << 4)[:3]
    return hdr + (bytes([b.lit_rle[0]]) if b.lit_rle else b.lits)


def _sequences_section(b: Block) -> bytes:
    n = len(b.seqs)
    h = b.nseq_hdr or (1 if n < 128 else 2 if n < 0x7F00 else 3)
    if h == 1:
        assert n < 128
        out = bytes([n])
    elif h == 2:
        assert n < 0x7F00
        out = bytes([(n >> 8) + 128, n & 255])
    else:
        assert 0x7F00 <= n <= 0x7F00 + 0xFFFF
        out = bytes([255]) + struct.pack("<H", n - 0x7F00)
    if not n:
        assert h == 1
        return out
    ll0, ml0, ov0 = b.seqs[0]
    llc, mlc, ofc = _code_of(LL_CODES, ll0), _code_of(ML_CODES, ml0), ov0.bit_length() - 1
    (llb, lln), (mlb, mln) = LL_CODES[llc], ML_CODES[mlc]
    # the bitstream, read backwards by the decoder: as a big-endian bit string 0..0 1 <seq 0> <seq 1> ..,
    # each sequence its offset, match-length and literal-length extra bits (the RLE tables' states take none)
    per = ofc + mln + lln
    v, nbits = 1, 1
    for ll_, ml_, ov in b.seqs:
        assert ov >= 1 and ov.bit_length() - 1 == ofc, (ov, ofc)
        assert 0 <= ll_ - llb < (1 << lln) and 0 <= ml_ - mlb < (1 << mln), (ll_, ml_)
        v = (v << per) | (ov - (1 << ofc)) << (mln + lln) | (ml_ - mlb) << lln | (ll_ - llb)
        nbits += per
    return out + bytes([0x54, llc, ofc, mlc]) + v.to_bytes((nbits + 7) // 8, "little")


def _block_bytes(b: Block, last: bool) -> bytes:
    if b.kind == RAW:
        assert len(b.data) <= BLOCK_MAX
        return struct.pack("<I", int(last) | RAW << 1 | len(b.data) << 3)[:3] + b.data
    if b.kind == RLE:
        assert b.n <= BLOCK_MAX
        return struct.pack("<I", int(last) | RLE << 1 | b.n << 3)[:3] + b.data
    body = _literals_section(b) + _sequences_section(b)
    assert len(body) < BLOCK_MAX
    return struct.pack("<I", int(last) | CMP << 1 | len(body) << 3)[:3] + body


def build(fr: Frame) -> bytes:
    n = len(execute([fr]))
    if fr.header == "window":
        assert 10 <= fr.window_log <= 30
        hdr = bytes([0x00, (fr.window_log - 10) << 3])
    elif fr.header == "fcs1":
        assert n < 256
        hdr = bytes([0x20, n])
    elif fr.header == "fcs2":
        assert 256 <= n < 65536 + 256
        hdr = bytes([0x60]) + struct.pack("<H", n - 256)
    elif fr.header == "fcs4":
        hdr = bytes([0xA0]) + struct.pack("<I", n)
    elif fr.header == "fcs8":
        hdr = bytes([0xE0]) + struct.pack("<Q", n)
    else:
        raise ValueError(fr.header)
    assert fr.blocks
    body = b"".join(_block_bytes(b, i == len(fr.blocks) - 1) for i, b in enumerate(fr.blocks))
    return struct.pack("<I", MAGIC) + hdr + body


def skippable(payload: bytes = b"skipped", nibble: int = 3) -> bytes:
    return struct.pack("<II", 0x184D2A50 | nibble, len(payload)) + payload


def _copy_match(out: bytearray, off: int, ml: int) -> None:
    assert 0 < off <= len(out), (off, len(out))
    if off >= ml:
        start = len(out) - off
        out += out[start:start + ml]
    else:
        pat = bytes(out[-off:])
        out += (pat * (ml // off + 1))[:ml]


def execute(frames) -> bytes:
    """The reference executor: the bytes a list of Frame specs decodes to (RFC 8878 3.1.1.4-5)."""
    total = bytearray()
    for fr in frames:
        out = bytearray()  # offsets never reach before their own frame
        rep = [1, 4, 8]
        for b in fr.blocks:
            if b.kind == RAW:
                out += b.data
                continue
            if b.kind == RLE:
                out += b.data * b.n
                continue
            lits, lp = b.literals(), 0
            for ll, ml, ov in b.seqs:
                out += lits[lp:lp + ll]
                lp += ll
                if ov > 3:
                    off = ov - 3
                    rep = [off, rep[0], rep[1]]
                else:
                    k = ov - 1 + (1 if ll == 0 else 0)
                    if k == 0:
                        off = rep[0]
                    elif k == 1:
                        off = rep[1]
                        rep = [rep[1], rep[0], rep[2]]
                    elif k == 2:
                        off = rep[2]
                        rep = [rep[2], rep[0], rep[1]]
                    else:
                        off = rep[0] - 1
                        rep = [off, rep[0], rep[1]]
                _copy_match(out, off, ml)
            assert lp <= len(lits)
            out += lits[lp:]
        total += out
    return bytes(total)


# ---------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """One encoded chunk: `enc` decodes to `expect` (len(expect) is the chunk size). `check` asserts
    the shape the case is meant to have (block counts, types, sequence counts); `parallel`: the case
    is meant for the block-parallel pipeline (None: either decoder may take it); `specs`: the Frame
    specs of a hand-built case (expect == execute(specs))."""
    name: str
    enc: bytes
    expect: bytes
    check: object = None
    parallel: bool | None = True
    specs: list | None = None
    checksummed: bool = False

    def check_path(self) -> None:
        """A case meant for the block-parallel pipeline fits its scratch by the mirrored layout, and a
        case that leaves the path open does so because it does not: no case changes sides unnoticed."""
        assert self.parallel in (True, None), self.name
        assert fits_parallel(self.enc, len(self.expect)) == (self.parallel is True), (self.name, self.parallel)


HUF_TAB = (1 << 12) * 2 + 16  # zstd.hip: a Huffman decoding table in the literal scratch


def layout(chunk: int):
    """(blk_cap, lit_stride, seq_cap) of a chunk of `chunk` decoded bytes: zstd_scratch_sizes
    (zarrs_amd/csrc/zstd_launch.cpp; tests/test_zstd_launch.py holds the two together) over the plan's
    slot (the chunk rounded up to 256 bytes)."""
    slot = (chunk + 255) & ~255
    lit_stride = (max(slot + slot // 8, BLOCK_MAX + 64 + 2 * HUF_TAB) + 255) & ~255
    return min(slot // 32768 + 64, 1 << 20), lit_stride, slot // 4 + 1024


def fits_parallel(enc: bytes, chunk: int) -> bool:
    """Whether the chunk fits the block-parallel pipeline's scratch as k_zstd_scan counts it (zstd.hip):
    at most blk_cap blocks, seq_cap sequences, and lit_stride bytes of literal scratch, which holds the
    RLE and Huffman literals and, 16-byte aligned before each block of Huffman literals, its decoding
    table of HUF_TAB bytes. A chunk over one of these takes the serial decoder: the library's business,
    so such a case asserts exact bytes and leaves the path open."""
    blk_cap, lit_stride, seq_cap = layout(chunk)
    lit = 0
    for ltype, regen, _ in sections(enc):
        if ltype >= 2:
            lit = ((lit + 15) & ~15) + HUF_TAB
        lit += regen if ltype else 0
    return len(blocks(enc)) <= blk_cap and sum(sequence_counts(enc)) <= seq_cap and lit <= lit_stride


WSPAN = 32768 - 16 - 16  # zstd_xwin.inc: the latency mode's bytes of a block per workgroup


def _rng(seed):
    return np.random.default_rng(seed)


def _hand(name, frames, *, check=None, parallel=True, pre=b"", mid=None) -> Case:
    """A case of hand-built frames (mid: bytes put between the frames, e.g. a skippable frame)."""
    encs = [build(f) for f in frames]
    enc = pre + (mid if mid is not None else b"").join(encs)
    return Case(name, enc, execute(frames), check, parallel, list(frames))


def periodic(n: int, period: int, seed: int) -> bytes:
    pat = _rng(seed).integers(0, 256, period, dtype=np.uint8)
    return np.tile(pat, n // period + 1)[:n].tobytes()


WORDS = [b"zarr", b"chunk", b"shard", b"decode", b"gpu", b"codec", b"window", b"sequence", b"literal", b" ", b" the ",
         b"\n", b", ", b"offset", b"block"]


def text(n: int, seed: int) -> bytes:
    r = _rng(seed)
    return b"".join(WORDS[i] for i in r.integers(0, len(WORDS), n // 3 + 8))[:n]


def runs(n: int, flush: int, n_changing: int, seed: int) -> bytes:
    """Runs of one byte value (0 .. 3) whose value changes inside exactly n_changing of the n / flush
    pieces the streaming encoder is flushed at (once or twice, never at a piece's edge; the first piece
    is one of them): libzstd makes those pieces compressed blocks and the pieces that lie inside one
    run RLE blocks."""
    r = _rng(seed)
    out = np.zeros(n, np.uint8)
    changing = {0} | set(1 + int(b) for b in r.choice(n // flush - 1, n_changing - 1, replace=False))
    v = int(r.integers(0, 4))
    for b in range(n // flush):
        cuts = sorted(set(int(c) for c in r.integers(1, flush, int(r.integers(1, 3))))) if b in changing else []
        p = 0
        for c in cuts + [flush]:
            out[b * flush + p:b * flush + c] = v
            if c < flush:
                v = (v + 1 + int(r.integers(0, 3))) % 4
            p = c
    return out.tobytes()


def skewed_text(n: int, seed: int) -> bytes:
    """Word text over a drifting vocabulary with a skewed letter mix between the words: level 19 gives it
    Huffman literals, and treeless ones where the statistics stay put."""
    r = _rng(seed)
    out, size = [], 0
    while size < n:
        w = WORDS[int(r.integers(0, len(WORDS)))]
        g = bytes((97 + np.minimum(r.geometric(0.25, int(r.integers(1, 9))), 25)).astype(np.uint8))
        out += [w, g]
        size += len(w) + len(g)
    return b"".join(out)[:n]


# --- family 1: block chains, streaming --------------------------------------------------------------
CHAIN_PAIRS = [(4096, 64), (4096, 72), (8192, 128), (16384, 256), (65536, 1024), (1 << 20, 16384)]


def _chain_check(chunk):
    def check(c: Case):
        b = blocks(c.enc)
        assert b[0][0] == RAW and all(t == CMP for t, _ in b[1:]), b[:4]
        assert len(b) <= chunk // 32768 + 64, len(b)
        if chunk <= 8192:
            assert len(b) > 33, len(b)
    return check


@functools.lru_cache(maxsize=None)
def family_chains_streaming():
    out = []
    for chunk, f in CHAIN_PAIRS:
        data = periodic(chunk, f, chunk + f)
        for pledged in (True, False):
            for ck in (False, True):
                enc = stream_frame(data, f, pledged=pledged, checksum=ck)
                out.append(Case(f"chain_{chunk}_f{f}_{'pledged' if pledged else 'nosize'}{'_ck' if ck else ''}", enc,
                                data, _chain_check(chunk), True, None, ck))
    return out


# --- family 2: block chains, hand-built, exact depth -------------------------------------------------
CHAIN_DEPTHS = [15, 16, 17, 31, 32, 33, 63]


def chain_frame(b: int, k: int, chunk: int, seed: int) -> Frame:
    """One raw block of b bytes, k compressed blocks of one sequence (ll 0, ml b, offset b) each: byte p
    of compressed block j comes from block j - 1, j hops from the raw block; then raw blocks padding
    the chunk to `chunk` bytes (when they would be one block more than the block-parallel path admits,
    the padding goes in front of the b bytes, in the same raw block)."""
    r = _rng(seed)
    pad = chunk - b * (k + 1)
    assert pad >= 0
    n_pad = (pad + BLOCK_MAX - 1) // BLOCK_MAX
    front = pad if 1 + k + n_pad > layout(chunk)[0] else 0
    blks = [raw(r.integers(0, 256, front + b, dtype=np.uint8).tobytes())]
    blks += [cmp_block(b"", [(0, b, b + 3)]) for _ in range(k)]
    for o in range(0, pad - front, BLOCK_MAX):
        blks.append(raw(r.integers(0, 256, min(BLOCK_MAX, pad - o), dtype=np.uint8).tobytes()))
    return Frame(blks, "fcs4")


def _depth_check(k):
    def check(c: Case):
        b = blocks(c.enc)
        assert b[0][0] == RAW and b[0][1] in (64, len(c.expect) - 64 * k), b[0]
        assert all(t == CMP for t, _ in b[1:k + 1]) and all(t == RAW for t, _ in b[k + 1:])
        assert len(b) <= layout(len(c.expect))[0]
        assert sequence_counts(c.enc) == [1] * k
        assert all(len(bl.lits) == 0 and bl.seqs == [(0, 64, 67)] for bl in c.specs[0].blocks[1:k + 1])
    return check


@functools.lru_cache(maxsize=None)
def family_chains_exact():
    out = []
    for chunk in (4096, 8192, 16384, 65536):
        for k in CHAIN_DEPTHS:
            out.append(_hand(f"depth_{chunk}_k{k}", [chain_frame(64, k, chunk, 1000 * k + chunk)], check=_depth_check(k)))
    return out


# --- family 3: streaming text and runs ---------------------------------------------------------------
def _count_check(lo_cmp=None, hi_cmp=None, n_rle=None, n_blocks=None, lit_types=None, last_empty_raw=False):
    def check(c: Case):
        b = blocks(c.enc)
        ncmp, nrle = sum(t == CMP for t, _ in b), sum(t == RLE for t, _ in b)
        if lo_cmp is not None:
            assert lo_cmp <= ncmp <= hi_cmp, (ncmp, nrle, len(b))
        if n_rle is not None:
            assert nrle == n_rle, (ncmp, nrle, len(b))
        if n_blocks is not None:
            assert len(b) == n_blocks, len(b)
        if lit_types is not None:
            have = set(literal_types(c.enc))
            assert set(lit_types) <= have, have
        if last_empty_raw:
            assert walk(c.enc)[0][-1][:2] == (RAW, 0)
    return check


@functools.lru_cache(maxsize=None)
def family_streaming_mixed():
    out = []

    def add(name, data, check, parallel=True, **kw):
        for ck in (False, True):
            enc = stream_frame(data, checksum=ck, **kw)
            out.append(Case(name + ("_ck" if ck else ""), enc, data, check, parallel, None, ck))

    for chunk, f in ((4096, 64), (16384, 256), (65536, 1000)):
        add(f"text_{chunk}_f{f}", text(chunk, chunk), _count_check(64, 66, lit_types=[0]), flush=f)
    add("runs_4096_f64", runs(4096, 64, 12, 1), _count_check(12, 12, n_rle=52), flush=64)
    add("runs_16384_f256", runs(16384, 256, 44, 2), _count_check(44, 44, n_rle=20), flush=256)
    # 64 blocks of Huffman literals take 64 tables in the literal scratch, more than it holds: these (and
    # the 64-block windowLog 10 frames below) leave the path open; their smaller twins do not
    add("text19_262144_f4096", skewed_text(262144, 3), _count_check(n_blocks=64, lit_types=[2, 3]), None, flush=4096,
        level=19)
    # level 19 on 32 KiB: few enough Huffman blocks for the block-parallel pipeline's literal scratch
    add("text19_32768_f4096", skewed_text(32768, 3), _count_check(n_blocks=8, lit_types=[2, 3]), flush=4096, level=19)
    noise = _rng(4).integers(0, 4, 65536, dtype=np.uint8).tobytes()
    add("wlog10_noise_8192", noise[:8192], _count_check(n_blocks=8, lit_types=[2]), flush=0, window_log=10)
    add("wlog10_noise_16384", noise[:16384], _count_check(n_blocks=16, lit_types=[2]), flush=0, window_log=10)
    add("wlog10_noise_65536", noise, _count_check(n_blocks=64), None, flush=0, window_log=10)
    add("wlog10_noise_65536_nosize", noise, _count_check(n_blocks=64), None, flush=0, window_log=10, pledged=False)
    t = text(16384, 5)
    add("empty_last_16384", t, _count_check(last_empty_raw=True), flush=2048, end_empty=True, pledged=False)
    # that frame followed by a second frame in the same chunk
    for ck in (False, True):
        a = stream_frame(t[:8192], 1024, end_empty=True, pledged=False, checksum=ck)
        b = stream_frame(t[8192:], 512, checksum=ck)

        def check(c, a=a):
            assert walk(c.enc)[0][-1][:2] == (RAW, 0) and len(walk(c.enc)) == 2 and c.enc.startswith(a)
        out.append(Case("empty_last_then_frame_16384" + ("_ck" if ck else ""), a + b, t, check, True, None, ck))
    return out


# --- family 4: capacity edges ------------------------------------------------------------------------
def _far_seqs(ns: int, seed: int, head: int):
    """ns sequences (ll 0, ml 3, offset in [1021, 2044], no further back than the frame's start: `head`
    bytes precede the first): offset values 1024 .. 2047, offset code 10."""
    u = _rng(seed).random(ns)
    hi = np.minimum(2044, head + 3 * np.arange(ns))
    return [(0, 3, int(1021 + x * (h - 1021 + 1)) + 3) for x, h in zip(u, hi)]


def _seq_cap_case(chunk, ns, tag, parallel):
    head = _rng(ns).integers(0, 256, chunk - 3 * ns, dtype=np.uint8).tobytes()
    assert len(head) >= 1021
    fr = Frame([raw(head), cmp_block(b"", _far_seqs(ns, ns + 1, len(head)))])

    def check(c: Case):
        assert blocks(c.enc)[0] == (RAW, chunk - 3 * ns) and sequence_counts(c.enc) == [ns]
        assert ns - layout(chunk)[2] == {"below": -1, "at": 0, "above": 1}[tag]
    return _hand(f"seq_cap_{tag}_{chunk}", [fr], check=check, parallel=parallel)


def _blk_cap_case(chunk, nb, tag, parallel):
    """nb tiny blocks: a raw head, then blocks of one literal and one 3-byte match 8 back, then raw."""
    k = nb - 2
    head = chunk - 4 * k - 16
    r = _rng(nb)
    blks = [raw(r.integers(0, 256, head, dtype=np.uint8).tobytes())]
    blks += [cmp_block(bytes([int(r.integers(0, 256))]), [(1, 3, 8 + 3)]) for _ in range(k)]
    blks.append(raw(r.integers(0, 256, 16, dtype=np.uint8).tobytes()))

    def check(c: Case):
        b = blocks(c.enc)
        assert len(b) == nb and nb - layout(chunk)[0] == {"below": -1, "at": 0, "above": 1}[tag]
        assert sequence_counts(c.enc) == [1] * k
    return _hand(f"blk_cap_{tag}_{chunk}", [Frame(blks)], check=check, parallel=parallel)


def _lit_fill_case(chunk):
    """RLE-literals blocks whose literals are the whole chunk: literals are all output, and the literal
    scratch (lit_stride) is larger than the slot, so a legal frame of RLE literals fills at most
    chunk bytes of it; this is that most (a head block with matches into it, then literal-only
    blocks)."""
    blks, left, r = [], chunk, _rng(chunk)
    first = True
    while left:
        n = min(left, 4000 if first else 4096)
        if first:  # 4000 RLE literals in runs of 40 with a 3-byte match 2 back after each
            seqs = [(40, 3, 2 + 3)] * 31
            blks.append(cmp_block(lit_rle=(int(r.integers(0, 256)), n - 93), seqs=seqs))
            first = False
        else:
            blks.append(cmp_block(lit_rle=(int(r.integers(0, 256)), n)))
        left -= n

    def check(c: Case):
        assert all(t == CMP for t, _ in blocks(c.enc)) and set(literal_types(c.enc)) == {1}
        assert sum(bl.lit_rle[1] for bl in c.specs[0].blocks) == chunk - 93 < layout(chunk)[1]
    return _hand(f"lit_rle_fill_{chunk}", [Frame(blks)], check=check)


def _lit_stride_case(delta, tag, parallel):
    """The literal scratch filled to lit_stride + delta by 17 literal-only blocks of Huffman literals
    (each takes a table of HUF_TAB bytes, 16-byte aligned, and its literals; every other block
    treeless): 16 blocks of 496 literals and one of 240 + delta, then raw bytes up to the chunk size.
    RLE literals cannot reach the edge: literals are all output and lit_stride is larger than the slot."""
    chunk = 8448
    r = _rng(17 + delta)
    sizes = [496] * 16 + [240 + delta]
    assert 17 * HUF_TAB + sum(sizes) == layout(chunk)[1] + delta
    blks = [cmp_block(r.integers(0, 2, n, dtype=np.uint8).tobytes(), huf="treeless" if i % 2 else "tree")
            for i, n in enumerate(sizes)]
    blks.append(raw(r.integers(0, 256, chunk - sum(sizes), dtype=np.uint8).tobytes()))

    def check(c: Case):
        assert [t for t, _ in blocks(c.enc)] == [CMP] * 17 + [RAW]
        assert [(t, n) for t, n, _ in sections(c.enc)] == [(3 if i % 2 else 2, n) for i, n in enumerate(sizes)]
        assert fits_parallel(c.enc, chunk) == (delta <= 0)
    return _hand(f"lit_stride_{tag}_{chunk}", [Frame(blks)], check=check, parallel=parallel)


def _huf_match_case():
    """Huffman literals (one-bit codes, then treeless) under sequences: matches copy Huffman-decoded bytes."""
    r = _rng(23)
    blks = [cmp_block(r.integers(0, 2, 700, dtype=np.uint8).tobytes(), [(40, 9, 17 + 3)] * 12, huf="tree"),
            cmp_block(r.integers(0, 2, 1023, dtype=np.uint8).tobytes(), [(16, 35, 600 + 3), (17, 36, 850 + 3)], huf="treeless")]
    fr = Frame(blks)
    n = len(execute([fr]))
    fr.blocks.append(raw(r.integers(0, 256, 8448 - n, dtype=np.uint8).tobytes()))

    def check(c: Case):
        assert [(t, n) for t, _, n in sections(c.enc)] == [(2, 12), (3, 2)] and len(c.expect) == 8448
    return _hand("huffman_one_bit_codes_8448", [fr], check=check)


@functools.lru_cache(maxsize=None)
def family_capacity():
    out = []
    cap = layout(16384)[2]
    assert cap == 16384 // 4 + 1024
    for ns, tag, par in ((cap - 1, "below", True), (cap, "at", True), (cap + 1, "above", None)):
        out.append(_seq_cap_case(16384, ns, tag, par))
    bc = layout(4096)[0]
    assert bc == 64
    for nb, tag, par in ((bc - 1, "below", True), (bc, "at", True), (bc + 1, "above", None)):
        out.append(_blk_cap_case(4096, nb, tag, par))
    out.append(_lit_fill_case(16384))
    out.append(_lit_fill_case(4096))
    for delta, tag, par in ((-1, "below", True), (0, "at", True), (1, "above", None)):
        out.append(_lit_stride_case(delta, tag, par))
    out.append(_huf_match_case())
    return out


# --- family 5: sequence-table and window edges -------------------------------------------------------
def _nseq_case(ns, chunk):
    """One compressed block of ns sequences (ll 1, ml 35 or 36: ML code 32, offset 1021 .. 2044; for the
    two largest counts ll 0 and ml 3) after a raw head; trailing literals after the last sequence."""
    r = _rng(ns)
    ml = r.integers(35, 37, ns) if ns < 20000 else np.full(ns, 3)
    ll = 1 if ns < 20000 else 0
    seqs = [(ll, int(m), int(v)) for m, v in zip(ml, r.integers(1024, 2048, ns))]
    body = sum(s[0] + s[1] for s in seqs)
    tail = 5
    lits = r.integers(0, 256, ns * ll + tail, dtype=np.uint8).tobytes()
    head = chunk - body - tail
    assert head >= 2044, (ns, head)
    heads = [raw(r.integers(0, 256, min(BLOCK_MAX, head - o), dtype=np.uint8).tobytes()) for o in range(0, head, BLOCK_MAX)]
    fr = Frame(heads + [cmp_block(lits, seqs)])

    def check(c: Case):
        assert sequence_counts(c.enc) == [ns] and c.parallel is True
        o = walk(c.enc)[0][-1][2]
        q = o + (1 if len(lits) < 32 else 2 if len(lits) < 4096 else 3) + len(lits)
        assert (1 if c.enc[q] < 128 else 2 if c.enc[q] < 255 else 3) == (1 if ns < 128 else 2 if ns < 0x7F00 else 3)
    return _hand(f"nseq_{ns}", [fr], check=check)


def _split(gap: int, k: int):
    """k (ll, ml) pairs with ll in 256 .. 511 and ml in 131 .. 258 whose lengths sum to gap."""
    extra = gap - 387 * k
    assert 0 <= extra <= 382 * k, gap
    out = []
    for _ in range(k):
        dl = min(extra, 255)
        dm = min(extra - dl, 127)
        extra -= dl + dm
        out.append((256 + dl, 131 + dm))
    return out


def _wspan_block(kind, delta, seed):
    """A 100 KiB compressed block after a 4 KiB raw head. The RLE table modes give a block one code per
    field, so every sequence has ll in 256 .. 511 (LL code 27), ml in 131 .. 258 (ML code 43) and an
    offset value of the special sequence's code. The special sequence is placed so that its match
    (kind 'lit': its literal run) starts WSPAN + delta bytes into the block: a match of 203 bytes at
    offset 1, 7 or 3000, or a run of 456 literals."""
    r = _rng(seed)
    bsize = 102400
    at = WSPAN + delta
    special = {"off1": (256, 203, 1 + 3), "off7": (256, 203, 7 + 3), "offbig": (256, 203, 3000 + 3),
               "lit": (456, 131, 1500 + 3)}[kind]
    ofc = special[2].bit_length() - 1
    lo, hi = max(1 << ofc, 4), 1 << (ofc + 1)

    def filler():
        return int(r.integers(256, 512)), int(r.integers(131, 259)), int(r.integers(lo, hi))

    seqs, pos = [], 0
    target = at - (special[0] if kind != "lit" else 0)  # where the special sequence starts
    while target - pos > 1800:
        seqs.append(filler())
        pos += seqs[-1][0] + seqs[-1][1]
    gap = target - pos  # 1031 .. 1800: two or three sequences take it exactly
    for ll, ml in _split(gap, 2 if gap <= 1538 else 3):
        seqs.append((ll, ml, int(r.integers(lo, hi))))
    pos = target
    seqs.append(special)
    pos += special[0] + special[1]
    while pos + 770 < bsize - 300:
        seqs.append(filler())
        pos += seqs[-1][0] + seqs[-1][1]
    tail = bsize - pos
    lits = r.integers(0, 256, sum(s[0] for s in seqs) + tail, dtype=np.uint8).tobytes()
    head = raw(r.integers(0, 256, 4096, dtype=np.uint8).tobytes())
    return Frame([head, cmp_block(lits, seqs)]), len(seqs)


def _wspan_case(kind, delta, seed):
    fr, ns = _wspan_block(kind, delta, seed)

    def check(c: Case):
        b = blocks(c.enc)
        assert [t for t, _ in b] == [RAW, CMP] and sequence_counts(c.enc) == [ns]
        # the special sequence's start within the block
        pos, hit = 0, False
        for ll, ml, ov in c.specs[0].blocks[1].seqs:
            start = pos if kind == "lit" else pos + ll
            hit |= start == WSPAN + delta
            pos += ll + ml
        assert hit and len(c.expect) == 4096 + 102400
    name = f"wspan_{kind}_{'m' if delta < 0 else 'p'}{abs(delta)}"
    return _hand(name, [fr], check=check)


def _long_match_case(off):
    """A 128 KiB block: one literal... `off` literals, then one match of 131071 bytes (ML code 52) at
    offset `off` reaching back over them; the block is the whole frame after a raw head of 2 KiB."""
    r = _rng(off)
    head = r.integers(0, 256, 2048, dtype=np.uint8).tobytes()
    fr = Frame([raw(head), cmp_block(bytes([int(r.integers(0, 256))]), [(1, 131071, off + 3)])])

    def check(c: Case):
        assert sequence_counts(c.enc) == [1] and len(c.expect) == 2048 + 131072
        assert _code_of(ML_CODES, 131071) == 52
    return _hand(f"long_match_off{off}", [fr], check=check)


def _long_literal_case():
    r = _rng(70000)
    lits = r.integers(0, 256, 70000 + 9, dtype=np.uint8).tobytes()
    fr = Frame([cmp_block(lits, [(70000, 40, 66000 + 3)])])

    def check(c: Case):
        assert sequence_counts(c.enc) == [1] and _code_of(LL_CODES, 70000) == 35
    return _hand("long_literal_70000", [fr], check=check)


@functools.lru_cache(maxsize=None)
def family_tables_windows():
    out = [_nseq_case(ns, 102400) for ns in (1, 127, 128, 1023, 1024, 1025, 2048, 2049)]
    # about 100 KiB of 3-byte matches in a 130 KiB chunk, whose seq_cap (34304) holds them
    out += [_nseq_case(ns, 133120) for ns in (0x7EFF, 0x7F00)]
    seed = 0
    for kind in ("off1", "off7", "offbig", "lit"):
        for delta in (-1, 0, 1):
            seed += 1
            out.append(_wspan_case(kind, delta, seed))
    # a match (and a literal run) straddling WSPAN: starts 100 bytes before it
    for kind in ("off1", "off7", "offbig", "lit"):
        seed += 1
        out.append(_wspan_case(kind, -100, seed))
    out += [_long_match_case(off) for off in (1, 2, 3, 5, 255, 1021)]
    out.append(_long_literal_case())
    return out


# --- family 6: repeat offsets ------------------------------------------------------------------------
def _repeat_frame(variant, seed):
    r = _rng(seed)
    head = raw(r.integers(0, 256, 1024, dtype=np.uint8).tobytes())
    # block A: three real offsets (one offset code per block: values 259 .. 511 -> offsets 256 .. 508);
    # the 'falling' variant starts its history at 300
    a_offs = (300, 410, 505) if variant == "cycle" else (505, 410, 300)
    blk_a = cmp_block(r.integers(0, 256, 3 * 5 + 2, dtype=np.uint8).tobytes(), [(5, 6, o + 3) for o in a_offs])
    blks = [head, blk_a]
    nseq = 0
    if variant == "falling":
        # offset_value 3 with ll == 0 fifty times in a row: rep1 - 1 each time (300 -> 250)
        blks.append(cmp_block(b"", [(0, 4, 3)] * 50))
        nseq += 50
    k = 0
    while nseq < 200:
        n = min(25, 200 - nseq)
        ll = 0 if k % 2 == 0 else 3
        if k % 3 == 2:
            seqs = [(ll, 5, 1)] * n  # offset code 0: value 1
        else:
            seqs = [(ll, 5, 2 + (i + k) % 2) for i in range(n)]  # offset code 1: values 2 and 3
        blks.append(cmp_block(r.integers(0, 256, ll * n + (k % 2), dtype=np.uint8).tobytes(), seqs))
        nseq += n
        k += 1
    # block C starts with a repeat code: the history crosses the block boundary
    blks.append(cmp_block(r.integers(0, 256, 2 * 4, dtype=np.uint8).tobytes(), [(2, 7, 2), (2, 7, 3), (2, 7, 2), (2, 7, 3)]))
    return Frame(blks), nseq


def _repeat_case(variant, seed):
    f1, n1 = _repeat_frame(variant, seed)
    # a second frame in the same chunk starts again from 1, 4, 8: its first block uses repeat codes at
    # once (8 literals first, so offsets 1, 4 and 8 are all in reach)
    r = _rng(seed + 50)
    f2 = Frame([cmp_block(r.integers(0, 256, 8 * 6, dtype=np.uint8).tobytes(),
                          [(8, 5, 3), (8, 5, 2), (8, 5, 3), (8, 5, 2), (8, 5, 3), (8, 5, 2)]),
                cmp_block(b"", [(0, 4, 1), (0, 4, 1), (0, 4, 1)])], "fcs1" if variant == "cycle" else "window")

    def check(c: Case):
        assert n1 == 200 and len(walk(c.enc)) == 2
        rep_blocks = c.specs[0].blocks[2:]
        assert all(s[2] <= 3 for b in rep_blocks for s in b.seqs)
        lls = [b.seqs[0][0] == 0 for b in rep_blocks]
        assert True in lls and False in lls
        if variant == "falling":
            assert c.specs[0].blocks[2].seqs == [(0, 4, 3)] * 50
    return _hand(f"repeat_{variant}", [f1, f2], check=check)


@functools.lru_cache(maxsize=None)
def family_repeat_offsets():
    return [_repeat_case("falling", 61), _repeat_case("cycle", 62)]


# --- family 7: frame headers --------------------------------------------------------------------------
def _small_cmp_frame(n, header, seed, window_log=17):
    """A frame of n bytes: a compressed block of raw literals and a few matches (n >= 40)."""
    r = _rng(seed)
    nlit = n - 3 * 6
    return Frame([cmp_block(r.integers(0, 256, nlit, dtype=np.uint8).tobytes(),
                            [(7, 6, 5 + 3), (7, 6, 6 + 3), (7, 6, 8 + 3)])], header, window_log)


@functools.lru_cache(maxsize=None)
def family_headers():
    out = []
    for header, n in (("fcs1", 200), ("fcs2", 4000), ("fcs4", 4000), ("fcs8", 4000), ("window", 4000)):
        def check(c, header=header):
            fhd = c.enc[4]
            assert (fhd >> 5) & 1 == (header != "window") and fhd >> 6 == {"fcs1": 0, "fcs2": 1, "fcs4": 2, "fcs8": 3,
                                                                           "window": 0}[header]
            assert blocks(c.enc) and blocks(c.enc)[0][0] == CMP
        # pad every case to the same chunk size (4096) with a second, raw-block frame
        pad = Frame([raw(_rng(n).integers(0, 256, 4096 - n, dtype=np.uint8).tobytes())], "fcs2" if 4096 - n >= 256 else "fcs1")
        out.append(_hand(f"header_{header}", [_small_cmp_frame(n, header, n + len(header)), pad], check=check))
    # the long forms of the literals size (3 bytes) and of the sequence count (2 bytes) for small values,
    # after an RLE block the matches reach into
    r = _rng(7)
    long_forms = Frame([rle(0xA5, 500), cmp_block(r.integers(0, 256, 3500, dtype=np.uint8).tobytes(),
                                                  [(7, 6, 8 + 3), (7, 6, 12 + 3), (7, 6, 9 + 3)], lit_hdr=3, nseq_hdr=2),
                        rle(0x11, 78)])

    def check_long(c):
        t, _, o, _ = walk(c.enc)[0][1]
        assert [b[0] for b in blocks(c.enc)] == [RLE, CMP, RLE] and (c.enc[o] >> 2) & 3 == 3 and c.enc[o + 3 + 3500] == 128
        assert len(c.expect) == 4096
    out.append(_hand("long_forms_after_rle", [long_forms], check=check_long))
    # a zero-length frame (one empty raw last block) followed by a real one
    empty = Frame([raw(b"")], "fcs1")

    def check_empty(c):
        assert walk(c.enc)[0] == [(RAW, 0, 9, 0)] and len(walk(c.enc)) == 2
    out.append(_hand("empty_frame_then_frame", [empty, _small_cmp_frame(4096, "fcs4", 77)], check=check_empty))

    # a skippable frame between two hand-built frames
    def check_skip(c):
        assert len(walk(c.enc)) == 2 and skippable() in c.enc
    out.append(_hand("skippable_between", [_small_cmp_frame(2000, "fcs2", 78), _small_cmp_frame(2096, "window", 79, 12)],
                     check=check_skip, mid=skippable()))
    return out


FAMILIES = {
    "chains_streaming": family_chains_streaming,
    "chains_exact": family_chains_exact,
    "streaming_mixed": family_streaming_mixed,
    "capacity": family_capacity,
    "tables_windows": family_tables_windows,
    "repeat_offsets": family_repeat_offsets,
    "headers": family_headers,
}
