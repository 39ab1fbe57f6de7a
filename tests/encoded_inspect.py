"""Test infrastructure (no GPU): read back what an encoder chose. The write side's tests
(tests/test_gpu_encoder_edges.py) state, per input, the edge of the format the input exists for; these
readers turn an encoded chunk into the tokens and header fields that statement is a predicate over.

  * deflate_tokens(raw): a small RFC 1951 inflater returning every block's header fields, the
    code-length symbols as written (16 / 17 / 18 with their repeat counts) and the LZ77 tokens.
  * zstd_blocks(frame): every block of a zstd frame (RFC 8878); of a compressed block the literals
    section's header fields and the sequences decoded from the predefined-table bitstream.
  * lz_tokens(fmt, stream): the elements of an lz4 / blosclz / snappy stream (the reference executors of
    tests/blosc_frames.py, tracing) and blosc_streams(frame): the streams of a c-blosc 1.x frame.

tests/test_encoded_inspect_model.py holds them to the hand builders (deflate_streams, zstd_frames,
blosc_frames), zlib and libzstd."""
from __future__ import annotations

import struct
from collections import namedtuple

import blosc_frames as BF
import zstd_frames as ZF

# ---------------------------------------------------------------------------------------------------
# DEFLATE
# ---------------------------------------------------------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

# btype 0 stored / 1 fixed / 2 dynamic; bitpos: the bit offset of the block's BFINAL bit; data_bit: of a
# stored block's first data byte (a multiple of 8); clsyms: the dynamic header's symbols as written,
# (0..15,) or (16 | 17 | 18, repeat count); ll / dd: the code lengths they describe; tokens: ('L', byte)
# or ('M', length, distance, length code) (a stored block: none, its bytes in `data`); size: the bytes
# the block decodes to.
DeflateBlock = namedtuple("DeflateBlock", "btype final hlit hdist hclen clsyms tokens bitpos data_bit data ll dd size")


class _Bits:
    def __init__(self, raw):
        self.raw, self.pos, self.acc, self.n = raw, 0, 0, 0

    def need(self, k):
        while self.n < k:
            if self.pos >= len(self.raw) + 8:
                raise ValueError("the DEFLATE stream ends inside a block")
            # zero bits past the end (a table lookup reads ahead): deflate_tokens checks what was used
            self.acc |= (self.raw[self.pos] if self.pos < len(self.raw) else 0) << self.n
            self.pos += 1
            self.n += 8

    def take(self, k):
        if not k:
            return 0
        self.need(k)
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def bitpos(self):
        return 8 * self.pos - self.n


def _table(lens):
    """Decoding table over max(lens) bits, LSB-first input: index -> (symbol, length). An incomplete
    code leaves holes (None)."""
    mx = max(lens) if lens else 0
    if mx == 0:
        return [], 0
    cnt = [0] * (mx + 2)
    for ln in lens:
        if ln:
            cnt[ln] += 1
    code, nxt = 0, [0] * (mx + 2)
    for b in range(1, mx + 1):
        code = (code + cnt[b - 1]) << 1 if b > 1 else 0
        nxt[b] = code
    tab = [None] * (1 << mx)
    for s, ln in enumerate(lens):
        if not ln:
            continue
        c = nxt[ln]
        nxt[ln] += 1
        if c >> ln:
            raise ValueError("over-subscribed code lengths")
        r = int(format(c, "0%db" % ln)[::-1], 2)
        for hi in range(1 << (mx - ln)):
            tab[r | hi << ln] = (s, ln)
    return tab, mx


def _sym(b, tab, mx):
    b.need(mx)
    e = tab[b.acc & ((1 << mx) - 1)]
    if e is None:
        raise ValueError("a bit string outside the code at bit %d" % b.bitpos())
    b.acc >>= e[1]
    b.n -= e[1]
    return e[0]


_FIXED = None


def deflate_tokens(raw):
    """(blocks, decoded bytes, bytes of `raw` the stream occupies) of the raw DEFLATE stream at the
    start of `raw`: a list of DeflateBlock up to and including the final one."""
    global _FIXED
    b, out, blocks = _Bits(bytes(raw)), bytearray(), []
    while True:
        bitpos = b.bitpos()
        final, btype = b.take(1), b.take(2)
        n0 = len(out)
        if btype == 3:
            raise ValueError("block type 3")
        if btype == 0:
            b.take(b.n % 8)
            ln, nln = b.take(16), b.take(16)
            if ln ^ nln != 0xFFFF:
                raise ValueError("a stored block's LEN / NLEN disagree")
            data_bit = b.bitpos()
            assert data_bit % 8 == 0 and b.n % 8 == 0
            # the whole bytes still in the accumulator first, then the stream's
            data = bytearray()
            while b.n and len(data) < ln:
                data.append(b.take(8))
            rest = ln - len(data)
            if b.pos + rest > len(b.raw):
                raise ValueError("a stored block runs past the stream")
            data += b.raw[b.pos:b.pos + rest]
            b.pos += rest
            out += data
            blocks.append(DeflateBlock(0, final, None, None, None, [], [], bitpos, data_bit, bytes(data), None, None,
                                       ln))
        else:
            hlit = hdist = hclen = None
            clsyms = []
            if btype == 1:
                if _FIXED is None:
                    _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 32))
                (lt, lm), (dt, dm) = _FIXED
                ll, dd = None, None
            else:
                hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CLEN_ORDER[i]] = b.take(3)
                ct, cm = _table(cl)
                seq = []
                while len(seq) < hlit + hdist:
                    s = _sym(b, ct, cm)
                    if s < 16:
                        clsyms.append((s,))
                        seq.append(s)
                    elif s == 16:
                        r = 3 + b.take(2)
                        if not seq:
                            raise ValueError("a repeat with nothing before it")
                        clsyms.append((16, r))
                        seq += [seq[-1]] * r
                    else:
                        r = 3 + b.take(3) if s == 17 else 11 + b.take(7)
                        clsyms.append((s, r))
                        seq += [0] * r
                if len(seq) != hlit + hdist:
                    raise ValueError("the code lengths overrun HLIT + HDIST")
                ll, dd = seq[:hlit], seq[hlit:]
                if not ll[256]:
                    raise ValueError("no end-of-block code")
                (lt, lm), (dt, dm) = _table(ll), _table(dd)
            tokens = []
            while True:
                s = _sym(b, lt, lm)
                if s < 256:
                    tokens.append(("L", s))
                    out.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise ValueError("length code %d" % s)
                    ln = LEN_BASE[s - 257] + b.take(LEN_EXTRA[s - 257])
                    if not dm:
                        raise ValueError("a match in a block without distance codes")
                    d = _sym(b, dt, dm)
                    if d > 29:
                        raise ValueError("distance code %d" % d)
                    dist = DIST_BASE[d] + b.take(DIST_EXTRA[d])
                    if dist > len(out):
                        raise ValueError("distance %d before the start" % dist)
                    tokens.append(("M", ln, dist, s))
                    if dist >= ln:
                        out += out[len(out) - dist:len(out) - dist + ln]
                    else:
                        pat = bytes(out[-dist:])
                        out += (pat * (ln // dist + 1))[:ln]
            blocks.append(DeflateBlock(btype, final, hlit, hdist, hclen, clsyms, tokens, bitpos, None, None, ll, dd,
                                       len(out) - n0))
        if final:
            break
    used = (b.bitpos() + 7) // 8
    if used > len(b.raw):
        raise ValueError("the DEFLATE stream ends inside a block")
    return blocks, bytes(out), used


def gzip_member(enc):
    """(blocks, decoded) of a gzip member with the 10-byte header the GPU encoder writes (no optional
    fields); the CRC-32 / ISIZE trailer is left to zlib (the tests decode with it first)."""
    assert enc[:3] == b"\x1f\x8b\x08" and enc[3] == 0, enc[:4]
    blocks, out, used = deflate_tokens(enc[10:])
    assert 10 + used + 8 == len(enc), (used, len(enc))
    return blocks, out


def zlib_stream(enc):
    """(blocks, decoded) of an RFC 1950 stream (no preset dictionary)."""
    assert enc[0] & 15 == 8 and (enc[0] << 8 | enc[1]) % 31 == 0 and not enc[1] & 32, enc[:2]
    blocks, out, used = deflate_tokens(enc[2:])
    assert 2 + used + 4 == len(enc), (used, len(enc))
    return blocks, out


def replay_deflate(blocks):
    """The bytes the blocks' tokens stand for, copied a byte at a time (the check of `decoded`)."""
    out = bytearray()
    for b in blocks:
        if b.btype == 0:
            out += b.data
            continue
        for t in b.tokens:
            if t[0] == "L":
                out.append(t[1])
            else:
                for _ in range(t[1]):
                    out.append(out[-t[2]])
    return bytes(out)


def matches(blocks):
    """Every ('M', length, distance, code) token of the blocks, in order."""
    return [t for b in blocks for t in b.tokens if t[0] == "M"]


# ---------------------------------------------------------------------------------------------------
# zstd
# ---------------------------------------------------------------------------------------------------
# the predefined distributions (RFC 8878 3.1.1.3.2.2.1-3), -1: "less than 1"
LL_NORM = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_NORM = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_NORM = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
assert len(LL_NORM) == 36 and len(ML_NORM) == 53 and len(OF_NORM) == 29


def fse_dtable(norm, log):
    """FSE decoding table (RFC 8878 4.1.1): per state (symbol, bits to read, baseline)."""
    size = 1 << log
    sym, high = [None] * size, size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
    step, mask, pos = (size >> 1) + (size >> 3) + 3, size - 1, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & mask
            while pos > high:
                pos = (pos + step) & mask
    assert pos == 0 and None not in sym
    nxt = [1 if c == -1 else c for c in norm]
    tab = []
    for u in range(size):
        s = sym[u]
        x = nxt[s]
        nxt[s] += 1
        nb = log - (x.bit_length() - 1)
        tab.append((s, nb, (x << nb) - size))
    return tab


def read_ncount(buf):
    """An FSE table description (RFC 8878 4.1.1): (normalised counts, accuracy log, bytes it takes)."""
    v, pos = int.from_bytes(buf, "little"), 0

    def take(k):
        nonlocal pos
        r = (v >> pos) & ((1 << k) - 1)
        pos += k
        return r

    log = 5 + take(4)
    remaining, threshold, nbits, norm = (1 << log) + 1, 1 << log, log + 1, []
    while remaining > 1:
        mx = 2 * threshold - 1 - remaining
        low = (v >> pos) & (threshold - 1)
        if low < mx:
            count = low
            pos += nbits - 1
        else:
            count = take(nbits)
            if count >= threshold:
                count -= mx
        count -= 1
        remaining -= abs(count)
        norm.append(count)
        if count == 0:
            while True:
                r = take(2)
                norm += [0] * r
                if r != 3:
                    break
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
        if pos > 8 * len(buf) or len(norm) > 256:
            raise ValueError("an FSE table description runs past its bytes")
    if remaining != 1:
        raise ValueError("FSE probabilities do not add up")
    return norm, log, (pos + 7) // 8


def huf_lengths_of(desc):
    """The code length of every symbol of a Huffman tree description (RFC 8878 4.2.1), which starts at
    desc[0]: direct 4-bit weights or FSE-compressed ones (two interleaved states)."""
    hb = desc[0]
    if hb >= 128:
        nw = hb - 127
        ws = [(desc[1 + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(nw)]
    else:
        norm, log, used = read_ncount(desc[1:1 + hb])
        tab = fse_dtable(norm, log)
        stream = desc[1 + used:1 + hb]
        if not stream or not stream[-1]:
            raise ValueError("the weights' bitstream has no end mark")
        v = int.from_bytes(stream, "little")
        pos = v.bit_length() - 1

        def take(k):
            nonlocal pos
            pos -= k
            return (v >> pos) & ((1 << k) - 1)

        st = [take(log), take(log)]
        ws, k = [], 0
        while True:  # the state whose update overflows the stream ends it; the other gives the last weight
            sym, nb, base = tab[st[k]]
            ws.append(sym)
            if nb > pos:
                ws.append(tab[st[k ^ 1]][0])
                break
            st[k] = base + take(nb)
            k ^= 1
            if len(ws) > 255:
                raise ValueError("more than 255 weights")
    total = sum(1 << (w - 1) for w in ws if w)
    max_bits = total.bit_length()
    rest = (1 << max_bits) - total
    if not total or rest & (rest - 1):
        raise ValueError("the Huffman weights do not complete a power of two")
    ws.append(rest.bit_length())
    return [max_bits + 1 - w if w else 0 for w in ws]


_PRE = None


def _sequences(payload, nseq):
    """[(ll, ml, offset_value)] of a predefined-mode sequences bitstream (RFC 8878 3.1.1.3.2.1.2)."""
    global _PRE
    if _PRE is None:
        _PRE = (fse_dtable(LL_NORM, 6), fse_dtable(OF_NORM, 5), fse_dtable(ML_NORM, 6))
    llt, oft, mlt = _PRE
    if not payload or payload[-1] == 0:
        raise ValueError("a sequences bitstream without its end mark")
    v = int.from_bytes(payload, "little")
    pos = v.bit_length() - 1  # bits below the end mark, read from the top down

    def take(k):
        nonlocal pos
        if k > pos:
            raise ValueError("the sequences bitstream is too short")
        pos -= k
        return (v >> pos) & ((1 << k) - 1)

    sl, so, sm = take(6), take(5), take(6)
    seqs = []
    for i in range(nseq):
        llc, ofc, mlc = llt[sl][0], oft[so][0], mlt[sm][0]
        ov = (1 << ofc) + take(ofc)
        ml = ZF.ML_CODES[mlc][0] + take(ZF.ML_CODES[mlc][1])
        ll = ZF.LL_CODES[llc][0] + take(ZF.LL_CODES[llc][1])
        seqs.append((ll, ml, ov))
        if i + 1 < nseq:
            sl = llt[sl][2] + take(llt[sl][1])
            sm = mlt[sm][2] + take(mlt[sm][1])
            so = oft[so][2] + take(oft[so][1])
    if pos:
        raise ValueError("%d bits of the sequences bitstream are left over" % pos)
    return seqs


# type: 0 raw / 1 RLE / 2 compressed; size: the bytes the block decodes to; last: the header's Last_Block bit. Of a
# compressed block: ltype (0 raw, 1 RLE, 2 Huffman, 3 treeless), sf (Size_Format), lhdr (header bytes),
# regen / csize (regenerated and compressed size; csize of raw / RLE literals: regen / 1), streams (of a
# Huffman section: 1 or 4), tree ("direct" | "fse" | None), nseq, modes (Symbol_Compression_Modes), seqs
# [(ll, ml, offset_value)], lits (raw / RLE literals' bytes, None for Huffman ones).
# max_bits: the longest code of the block's own Huffman tree (None without one).
ZstdBlock = namedtuple("ZstdBlock", "type size last ltype sf lhdr regen csize streams tree nseq modes seqs lits max_bits")
ZstdFrame = namedtuple("ZstdFrame", "fcs_bytes content_size checksum blocks")


def zstd_frames(buf, strict=True):
    """The frames of buf (skippable ones passed over) as ZstdFrame. A compressed block whose
    Symbol_Compression_Modes is not 0 (the predefined tables, all the GPU encoder writes) raises
    NotImplementedError (strict=False: its seqs and size are None instead, and its frame's total is not
    checked); an inconsistent block (sum(ll) beyond the literals, a frame whose blocks do not add up to
    its content size) raises ValueError."""
    buf = bytes(buf)
    frames, p = [], 0
    for blks in ZF.walk(buf):
        while struct.unpack_from("<I", buf, p)[0] & 0xFFFFFFF0 == 0x184D2A50:
            p += 8 + struct.unpack_from("<I", buf, p + 4)[0]
        fhd = buf[p + 4]
        single, flag = (fhd >> 5) & 1, fhd >> 6
        hlen, ck = ZF._frame_header_len(buf, p)
        fcs_bytes = (1 if single else 0) if flag == 0 else (2, 4, 8)[flag - 1]
        fcs = None
        if fcs_bytes:
            fcs = int.from_bytes(buf[p + 4 + hlen - fcs_bytes:p + 4 + hlen], "little") + (256 if flag == 1 else 0)
        out = []
        for i, (t, size, o, plen) in enumerate(blks):
            last = bool(buf[o - 3] & 1)  # Last_Block, the lowest bit of the 3-byte block header
            if t != ZF.CMP:
                out.append(ZstdBlock(t, size, last, *[None] * 12))
                continue
            out.append(_cmp_block(buf, o, plen, last, strict))
        total = None if any(b.size is None for b in out) else sum(b.size for b in out)
        if fcs is not None and total is not None and total != fcs:
            raise ValueError("the blocks decode to %d bytes, the frame header says %d" % (total, fcs))
        frames.append(ZstdFrame(fcs_bytes, fcs, ck, out))
        p = blks[-1][2] + blks[-1][3] + (4 if ck else 0)
    return frames


def zstd_blocks(frame, strict=True):
    """The ZstdBlock list of a single frame."""
    fr = zstd_frames(frame, strict)
    assert len(fr) == 1, len(fr)
    return fr[0].blocks


def _cmp_block(buf, o, plen, last, strict=True):
    ltype, sf = buf[o] & 3, (buf[o] >> 2) & 3
    v = int.from_bytes(buf[o:o + 5], "little")
    streams = tree = lits = max_bits = None
    if ltype <= 1:
        h = (1, 2, 1, 3)[sf]
        regen = (v & (1 << 8 * h) - 1) >> (3 if h == 1 else 4)
        csize = regen if ltype == 0 else 1
        lits = buf[o + h:o + h + regen] if ltype == 0 else buf[o + h:o + h + 1] * regen
    else:
        h, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
        regen, csize = (v >> 4) & (1 << bits) - 1, (v >> (4 + bits)) & (1 << bits) - 1
        streams = 1 if sf == 0 else 4
        if ltype == 2:
            tree = "fse" if buf[o + h] < 128 else "direct"
            max_bits = max(huf_lengths_of(buf[o + h:o + h + csize]))
    q = o + h + csize
    if q >= o + plen:
        raise ValueError("the literals section overruns its block")
    c0 = buf[q]
    if c0 < 128:
        nseq, q = c0, q + 1
    elif c0 < 255:
        nseq, q = ((c0 - 128) << 8) + buf[q + 1], q + 2
    else:
        nseq, q = (buf[q + 1] | buf[q + 2] << 8) + 0x7F00, q + 3
    modes, seqs = None, []
    if nseq:
        modes = buf[q]
        q += 1
        if modes != 0:
            if strict:
                raise NotImplementedError("Symbol_Compression_Modes 0x%02x: only the predefined tables (0) are "
                                          "decoded here" % modes)
            return ZstdBlock(ZF.CMP, None, last, ltype, sf, h, regen, csize, streams, tree, nseq, modes, None, lits,
                             max_bits)
        seqs = _sequences(buf[q:o + plen], nseq)
    elif q != o + plen:
        raise ValueError("bytes after an empty sequences section")
    sll = sum(s[0] for s in seqs)
    if sll > regen:
        raise ValueError("the sequences take %d literals, the section holds %d" % (sll, regen))
    size = regen + sum(s[1] for s in seqs)  # = sum(ll) + sum(ml) + the trailing literals
    return ZstdBlock(ZF.CMP, size, last, ltype, sf, h, regen, csize, streams, tree, nseq, modes, seqs, lits, max_bits)


def replay_zstd(blocks, history=b""):
    """The bytes a frame's ZstdBlock list decodes to when every compressed block has raw or RLE
    literals (lits is not None) and no repeat offsets beyond the plain rules; raw / RLE blocks need
    their payload, so this takes (block, payload) pairs: payload None for compressed blocks."""
    out = bytearray(history)
    rep = [1, 4, 8]
    for b, payload in blocks:
        if b.type == ZF.RAW:
            out += payload
            continue
        if b.type == ZF.RLE:
            out += payload * b.size
            continue
        lp = 0
        for ll, ml, ov in b.seqs:
            out += b.lits[lp:lp + ll]
            lp += ll
            if ov > 3:
                off = ov - 3
                rep = [off, rep[0], rep[1]]
            else:
                k = ov - 1 + (1 if ll == 0 else 0)
                if k == 0:
                    off = rep[0]
                elif k == 3:
                    off = rep[0] - 1
                    rep = [off, rep[0], rep[1]]
                else:
                    off = rep[k]
                    rep = [off] + [r for j, r in enumerate(rep) if j != k]
            ZF._copy_match(out, off, ml)
        out += b.lits[lp:]
    return bytes(out[len(history):])


# ---------------------------------------------------------------------------------------------------
# blosc: LZ streams and frames
# ---------------------------------------------------------------------------------------------------
# lits: the literal run lengths; matches: (match length, offset); elements: every element in stream
# order, ("lit", length, form) / ("match", length, offset, form). The form: lz4: the count of length
# extension bytes; blosclz: "run" (a literal run of <= 32) or ("near" | "far", extension bytes); snappy:
# a literal's length bytes after its tag (0..4), a copy's tag type (1, 2, 3). preamble (snappy):
# (decoded length, its varint's bytes).
LzTokens = namedtuple("LzTokens", "lits matches elements decoded preamble")


def lz_tokens(fmt, stream):
    trace = []
    fn = {"lz4": BF._lz4, "blosclz": BF._blosclz, "snappy": BF._snappy}[fmt]
    try:
        out = fn(bytes(stream), 1 << 31, trace)
    except BF._Bad as e:
        raise ValueError("a corrupt %s stream at byte %d" % (fmt, e.args[0]))
    pre = None
    if trace and trace[0][0] == "pre":
        pre = trace[0][1:]
        trace = trace[1:]
    return LzTokens([t[1] for t in trace if t[0] == "lit"], [(t[1], t[2]) for t in trace if t[0] == "match"],
                    trace, out, pre)


def merged_matches(tok):
    """(length, offset, start position) of the matches with adjacent same-offset pieces joined (snappy
    writes a long match as several copies; deflate-style 258-byte pieces are not joined here)."""
    out, pos, prev_match = [], 0, False
    for e in tok.elements:
        if e[0] == "lit":
            pos += e[1]
            prev_match = False
        else:
            if prev_match and out[-1][1] == e[2]:
                out[-1] = (out[-1][0] + e[1], e[2], out[-1][2])
            else:
                out.append((e[1], e[2], pos))
            pos += e[1]
            prev_match = True
    return out


BloscStream = namedtuple("BloscStream", "block csize payload stored size")
BloscFrame = namedtuple("BloscFrame", "version versionlz flags typesize nbytes blocksize cbytes memcpyed comp streams")


def blosc_streams(frame):
    """The header fields and streams of a c-blosc 1.x frame (blosc.c blosc_d): per block its split
    streams, each (block index, csize, payload, stored?, decoded size); stored: csize equals the
    stream's decoded size. A memcpyed frame has no streams."""
    f = bytes(frame)
    ver, vlz, flags, ts = f[0], f[1], f[2], f[3]
    nbytes, bsize, cbytes = struct.unpack_from("<3I", f, 4)
    if cbytes != len(f):
        raise ValueError("cbytes %d, the frame has %d bytes" % (cbytes, len(f)))
    comp = {v: k for k, v in BF.COMP.items()}.get(flags >> 5, flags >> 5)
    if flags & 2:
        if cbytes != 16 + nbytes:
            raise ValueError("a memcpyed frame of %d bytes for %d" % (cbytes, nbytes))
        return BloscFrame(ver, vlz, flags, ts, nbytes, bsize, cbytes, True, comp, [])
    nblk = (nbytes + bsize - 1) // bsize if nbytes else 0
    bstarts = struct.unpack_from("<%di" % nblk, f, 16)
    streams = []
    for b in range(nblk):
        bs = min(bsize, nbytes - b * bsize)
        leftover = bs < bsize
        nsplit = ts if (not leftover and BF.cblosc_splits(not (flags & 0x10), ts, bsize)) else 1
        ne = bs // nsplit
        p = bstarts[b]
        for _ in range(nsplit):
            (cs,) = struct.unpack_from("<i", f, p)
            p += 4
            if cs < 0 or p + cs > len(f):
                raise ValueError("block %d: a stream of %d bytes at %d" % (b, cs, p))
            streams.append(BloscStream(b, cs, f[p:p + cs], cs == ne, ne))
            p += cs
    return BloscFrame(ver, vlz, flags, ts, nbytes, bsize, cbytes, False, comp, streams)
