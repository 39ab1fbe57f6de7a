"""zstd and zlib streams inside blosc frames, hand-placed: a wrapper over the builders of
tests/zstd_frames.py, tests/deflate_streams.py and tests/blosc_frames.py (no entropy coder of its own), the
block-alias rule of k_zstd_plan and the plane test of k_blosc_finish restated in plain Python, and the
cases made with them. tests/test_blosc_inner_model.py referees every case with c-blosc on the CPU;
tests/test_gpu_blosc_inner.py decodes them on the GPU.

A case is one blosc frame (one chunk of a call). Its streams are zstd frames (compressor 4), zlib
streams (compressor 3), or stored splits; the expected chunk is blosc_frames.unfiltered over the
concatenated decoded streams, block by block. The split layout follows c-blosc (blosc_frames.cblosc_splits;
the leftover block is never split).

The alias rule (zstd.hip, k_zstd_plan with ZstdScratch::alias): over all blocks of all frames of one
stream, from the last to the first, a block is a candidate when it is raw, RLE, or compressed without
sequences; decodes to at least XDIRECT bytes; lies in a frame without a content checksum; and no match
of a later block (explicit or repeat offset, wherever the offset was set) has a source position before
the block's end. The ZALIAS earliest candidates are aliased: k_zstd_direct leaves them out of the slot
and k_blosc_finish reads them in the frame, in the literal scratch, or as one byte value."""
from __future__ import annotations

import functools
import struct
from dataclasses import dataclass, field

import numpy as np

import blosc_frames as B
import deflate_streams as D
import zstd_frames as Z

ZLIB, ZSTD = 3, 4     # c-blosc's compressor codes (the header's flags >> 5)
XDIRECT = 4096        # zstd.hip
ZALIAS = 2            # zstd_params.hpp
SLOT_ROUND = 256      # plan_exec.cpp: sub_slot = round_up(max_ne, 256)
OK, CORRUPT = B.OK, B.CORRUPT
SOURCES = ("raw", "rle", "lit_raw", "lit_rle", "lit_huf")
POSITIONS = ("on_plane", "inside_plane", "two_planes", "mid_to_mid", "one_before_boundary", "one_after_boundary")
PLANE = 8192          # the byte plane of both alias geometries: typesize 4 x 32768, typesize 2 x 16384


def sub_slot(max_ne: int) -> int:
    """The blosc stage's slot per stream, and the slot_bytes its zstd scratch is sized for."""
    return (max_ne + SLOT_ROUND - 1) & ~(SLOT_ROUND - 1)


def _rnd(n, seed, hi=256):
    return np.random.default_rng(seed).integers(0, hi, n, dtype=np.uint8).tobytes()


# ---------------------------------------------------------------------------------------------------
# the rule, restated
# ---------------------------------------------------------------------------------------------------
def frames_of(buf: bytes):
    """[(has_checksum, [(type, size field, payload offset, payload length)])] per zstd frame of buf;
    skippable frames are passed over (zstd_frames.walk, with the frame's checksum flag)."""
    out, p = [], 0
    while p < len(buf):
        magic = struct.unpack_from("<I", buf, p)[0]
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            p += 8 + struct.unpack_from("<I", buf, p + 4)[0]
            continue
        assert magic == Z.MAGIC, hex(magic)
        n, ck = Z._frame_header_len(buf, p)
        p += 4 + n
        blks = []
        while True:
            bh = buf[p] | buf[p + 1] << 8 | buf[p + 2] << 16
            p += 3
            t, size = (bh >> 1) & 3, bh >> 3
            plen = size if t != Z.RLE else 1
            blks.append((t, size, p, plen))
            p += plen
            if bh & 1:
                break
        p += 4 if ck else 0
        out.append((ck, blks))
    assert p == len(buf)
    assert [b for _, b in out] == Z.walk(buf)
    return out


def _spec_trace(fr: Z.Frame, base: int):
    """(decoded size, least match source position in the stream or None) per block of a hand-built
    frame that starts at decoded position `base`: RFC 8878 3.1.1.5 over the spec's sequences."""
    res, pos, rep = [], base, [1, 4, 8]
    for b in fr.blocks:
        start, least = pos, None
        if b.kind == Z.RAW:
            pos += len(b.data)
        elif b.kind == Z.RLE:
            pos += b.n
        else:
            for ll, ml, ov in b.seqs:
                pos += ll
                if ov > 3:
                    off = ov - 3
                    rep = [off, rep[0], rep[1]]
                else:
                    k = ov - 1 + (1 if ll == 0 else 0)
                    if k == 0:
                        off = rep[0]
                    elif k == 1:
                        off, rep = rep[1], [rep[1], rep[0], rep[2]]
                    elif k == 2:
                        off, rep = rep[2], [rep[2], rep[0], rep[1]]
                    else:
                        off = rep[0] - 1
                        rep = [off, rep[0], rep[1]]
                least = pos - off if least is None else min(least, pos - off)
                pos += ml
            pos = start + len(b.literals()) + sum(s[1] for s in b.seqs)
        res.append((pos - start, least))
    return res


@dataclass
class Blk:
    type: int
    off: int        # decoded position in the stream
    size: int       # decoded size
    nseq: int
    ck: bool        # its frame carries a content checksum
    least: int | None   # the least source position of its matches (None: it has none)
    source: str     # one of SOURCES: where an alias of it would read


def stream_blocks(payload: bytes, parts=None):
    """The blocks of a zstd stream, or None. parts: per frame, its zstd_frames.Frame spec, or None for
    a frame of libzstd's. This module decodes no sequences: a frame of libzstd's with any leaves the
    sizes and match sources of its blocks untold, and the stream has no block list here."""
    frames = frames_of(payload)
    parts = list(parts) if parts is not None else [None] * len(frames)
    assert len(parts) == len(frames), (len(parts), len(frames))
    secs = iter(Z.sections(payload))
    out, pos = [], 0
    for (ck, fb), sp in zip(frames, parts):
        tr = _spec_trace(sp, pos) if isinstance(sp, Z.Frame) else None
        assert tr is None or len(tr) == len(fb)
        for i, (t, size, _, _) in enumerate(fb):
            if t == Z.CMP:
                ltype, regen, nseq = next(secs)
                if tr is None and nseq:
                    return None
                osz, least = tr[i] if tr is not None else (regen, None)
                src = ("lit_raw", "lit_rle", "lit_huf", "lit_huf")[ltype]
            else:
                osz, nseq, least, src = size, 0, None, "raw" if t == Z.RAW else "rle"
            out.append(Blk(t, pos, osz, nseq, ck, least, src))
            pos += osz
    return out


def alias_rule(payload: bytes, parts=None):
    """The alias entries k_zstd_plan writes for a stream it plans: [(offset, length, source)], at most
    ZALIAS, the earliest. Returns (entries, exact). exact is False only for a stream without a block
    list (stream_blocks) that holds a raw, RLE or literal-only block of XDIRECT bytes: libzstd's own
    sequences would decide about it. Without such a block there is no candidate whatever they do."""
    blks = stream_blocks(payload, parts)
    if blks is None:
        shaped = [1 for (t, s) in Z.blocks(payload) if t != Z.CMP and s >= XDIRECT]
        shaped += [1 for (_, regen, nseq) in Z.sections(payload) if nseq == 0 and regen >= XDIRECT]
        return [], not shaped
    if len(blks) > 64 * 64:  # k_zstd_plan takes no cuts and no aliases past 4096 blocks
        return [], True
    least, cand = None, []
    for b in reversed(blks):
        if b.type == Z.CMP and b.nseq:  # the backward minimum of the match sources, repeat offsets resolved
            v = max(b.least, 0)
            least = v if least is None else min(least, v)
        shaped = b.size >= XDIRECT and (b.type != Z.CMP or b.nseq == 0) and not b.ck
        if shaped and (least is None or least >= b.off + b.size):
            cand.insert(0, (b.off, b.size, b.source))
    return cand[:ZALIAS], True


def plane_relation(l: int, neb: int, entries) -> str:
    """k_blosc_finish's test of one byte plane [l, l + neb) of a stream against its alias entries:
    'outside' all of them, 'inside' one, or 'straddle' (the block then takes the byte loop)."""
    rel = "outside"
    for ao, al, _ in entries:
        if l + neb <= ao or l >= ao + al:
            continue
        if l < ao or l + neb > ao + al:
            return "straddle"
        rel = "inside"
    return rel


# ---------------------------------------------------------------------------------------------------
# streams and cases
# ---------------------------------------------------------------------------------------------------
@dataclass
class Stream:
    """One split's stream. dec: what the payload decodes to (None: its decoder refuses it); kind: zstd,
    zlib, stored; parts: the zstd frames' specs (stream_blocks); parallel: a zstd stream meant for the
    block-parallel pipeline (None: it does not fit the scratch and takes the serial decoder); want: the
    alias entries the stream was built to get."""
    payload: bytes
    dec: bytes | None
    kind: str
    parts: list | None = None
    parallel: bool | None = True
    want: list | None = None

    def aliases(self):
        if self.kind != "zstd" or self.dec is None:
            return [], True
        return alias_rule(self.payload, self.parts)


@dataclass
class Case:
    id: str
    family: str
    size: int            # the chunk's bytes
    frame: bytes
    expect: bytes | None  # status OK: the chunk
    status: str
    comp: int
    ts: int
    bs: int
    mode: int
    blocks: list         # [block][split] -> (ne, Stream)
    tags: dict = field(default_factory=dict)  # what the case was built for (the model test checks them)

    def streams(self):
        return [(b, j, ne, s) for b, bl in enumerate(self.blocks) for j, (ne, s) in enumerate(bl)]

    def planes(self):
        """{(block, plane): relation} of every byte-shuffled typesize-2 / -4 block (the blocks whose
        planes k_blosc_finish's fast path looks at)."""
        out = {}
        if self.mode != 1 or self.ts not in (2, 4):
            return out
        for b, bl in enumerate(self.blocks):
            bsize = sum(ne for ne, _ in bl)
            neb, ne = bsize // self.ts, bl[0][0]
            for i in range(self.ts):
                j, l = divmod(i * neb, ne)
                s = bl[j][1]
                ent = s.aliases()[0] if s.parallel else []
                out[(b, i)] = plane_relation(l, neb, ent)
        return out

    def n_zstd(self):
        return sum(1 for *_, s in self.streams() if s.kind == "zstd") if self.comp == ZSTD else 0

    def alias_count(self):
        """(lo, hi) of the alias entries k_zstd_plan writes for this chunk: a stream that fits the
        block-parallel pipeline gets its rule's entries; one that does not (parallel None) takes the
        serial decoder and gets none, unless the library plans it after all (hi)."""
        lo = hi = 0
        for *_, s in self.streams():
            if s.kind != "zstd" or s.dec is None or self.comp != ZSTD:
                continue
            n = len(s.aliases()[0])
            hi += n
            lo += n if s.parallel else 0
        return lo, hi


def make(cid, fam, blocks, *, comp, ts, bs, nbytes, mode=0, split=False, memcpy=False, tags=None) -> Case:
    """A case from [block][split] -> Stream, laid out as c-blosc lays a chunk of nbytes out."""
    nfull, lo = divmod(nbytes, bs)
    assert len(blocks) == nfull + (1 if lo else 0)
    ns_full = ts if B.cblosc_splits(split, ts, bs) else 1
    sb, out_blocks, chunk, good = [], [], b"", True
    for b, bl in enumerate(blocks):
        left = b == nfull
        ns = 1 if left or memcpy else ns_full
        bsize = lo if left else bs
        assert len(bl) == ns and bsize % ns == 0, (cid, b, len(bl), ns)
        ne = bsize // ns
        row, laid, dec = [], [], b""
        for s in bl:
            if s.kind == "zstd" and len(s.payload) == ne:  # csize == ne would read as stored
                s = Stream(Z.skippable(b"") + s.payload, s.dec, s.kind, s.parts, s.parallel, s.want)
            assert (s.kind == "stored") == (len(s.payload) == ne), (cid, b, s.kind, len(s.payload), ne)
            row.append(B.S(s.payload, ne, s.kind == "stored"))
            laid.append((ne, s))
            good &= s.dec is not None and len(s.dec) == ne
            dec += s.dec or b""
        sb.append(row)
        out_blocks.append(laid)
        if good:
            chunk += dec if memcpy else B.unfiltered(dec, ts, mode)  # a memcpyed frame holds the chunk as it is
    fr = B.assemble(sb, comp=comp, typesize=ts, nbytes=nbytes, blocksize=bs, mode=mode, split=split, memcpy=memcpy)
    assert not good or len(chunk) == nbytes
    return Case(cid, fam, nbytes, fr.data, chunk if good else None, OK if good else CORRUPT, comp, ts, bs, mode,
                out_blocks, dict(tags or {}))


def stored(data: bytes) -> Stream:
    return Stream(bytes(data), bytes(data), "stored")


def one_zstd(cid, fam, s: Stream, n: int, tags=None) -> Case:
    """The stream as the single stream of a one-block, typesize-1, unshuffled frame of n bytes."""
    return make(cid, fam, [[s]], comp=ZSTD, ts=1, bs=n, nbytes=n, tags=tags)


# ---------------------------------------------------------------------------------------------------
# zstd streams with hand-placed blocks
# ---------------------------------------------------------------------------------------------------
def _fillers(n: int, seed: int, tail_match=True):
    """Blocks that decode to n bytes and are no alias candidates: raw blocks under XDIRECT bytes, and
    (n >= 64) a last compressed block whose one match reads its own literals."""
    out, r = [], np.random.default_rng(seed)
    cmp_n = 58 if tail_match and n >= 64 else 0
    left = n - cmp_n
    while left:
        k = min(left, int(r.integers(1500, 3500)))
        out.append(Z.raw(r.integers(0, 256, k, dtype=np.uint8).tobytes()))
        left -= k
    if cmp_n:
        out.append(Z.cmp_block(r.integers(0, 256, 48, dtype=np.uint8).tobytes(), [(20, 10, 8 + 3)]))
    return out


@functools.lru_cache(None)
def _huf_frame(n: int, seed: int):
    """A frame of libzstd's with one compressed block: n Huffman literals, no sequences."""
    data = _rnd(n, seed, 96)
    enc = Z.stream_frame(data, n)
    assert Z.sections(enc) == [(2, n, 0)] and Z.literal_types(enc) == [2] and n >= XDIRECT, Z.sections(enc)
    return enc, data


def _source_block(source: str, n: int, seed: int):
    """A block (or, for Huffman literals, a whole frame of libzstd's) of n decoded bytes."""
    if source == "raw":
        return Z.raw(_rnd(n, seed))
    if source == "rle":
        return Z.rle(seed % 251 + 1, n)
    if source == "lit_raw":
        return Z.cmp_block(_rnd(n, seed))
    if source == "lit_rle":
        return Z.cmp_block(lit_rle=(seed % 241 + 7, n))
    assert source == "lit_huf"
    return _huf_frame(n, seed)[0]


def zstream(total: int, spans, seed: int, tail_match=True) -> Stream:
    """A zstd stream of `total` decoded bytes: the spans [(offset, length, source)] are one block each,
    fillers between them. Hand-built blocks share frames; a Huffman span is a frame of its own."""
    frames, cur, pos = [], [], 0

    def close():
        nonlocal cur
        if cur:
            frames.append(Z.Frame(cur, "fcs4"))
            cur = []

    for k, (off, n, source) in enumerate(sorted(spans)):
        assert off >= pos
        cur += _fillers(off - pos, seed * 101 + k, tail_match)
        blk = _source_block(source, n, seed * 7 + k)
        if isinstance(blk, bytes):
            close()
            frames.append(blk)
        else:
            cur.append(blk)
        pos = off + n
    cur += _fillers(total - pos, seed * 101 + 99, tail_match)
    close()
    payload = b"".join(f if isinstance(f, bytes) else Z.build(f) for f in frames)
    dec = b"".join(Z.zstd_decompress(f, total) if isinstance(f, bytes) else Z.execute([f]) for f in frames)
    assert len(dec) == total
    want = [(o, n, s) for o, n, s in sorted(spans) if n >= XDIRECT][:ZALIAS]
    return Stream(payload, dec, "zstd", [None if isinstance(f, bytes) else f for f in frames], True, want)


def _position_spans(pos: str, nplanes: int, source: str):
    """The span of one aliasable block at a named position among `nplanes` planes of PLANE bytes."""
    P = PLANE
    return {"on_plane": [(P, P, source)],
            "inside_plane": [(P + 1000, 4500, source)],
            "two_planes": [(P if nplanes > 2 else 0, 2 * P, source)],
            "mid_to_mid": [(P // 2, P, source)],
            "one_before_boundary": [(P - 1, 5000, source)],
            "one_after_boundary": [(P + 1 - 5000, 5000, source)]}[pos]


GEOMS = ((4, 32768), (2, 16384))  # (typesize, blocksize): byte-shuffled, unsplit, planes of PLANE bytes


@functools.lru_cache(None)
def plane_streams(ts: int, bs: int):
    """{name: (Stream, tags)} of the alias_planes family at one geometry."""
    out, seed = {}, ts * 1000
    for pos in POSITIONS:
        for source in SOURCES:
            seed += 1
            out[f"{pos}_{source}"] = (zstream(bs, _position_spans(pos, ts, source), seed), {"position": pos, "source": source})
    P = PLANE
    for name, spans in (("two_in_one_plane", [(P - 8192, 4096, "raw"), (P - 4096, 4096, "lit_raw")]),
                        ("two_in_two_planes", [(0, P, "lit_huf"), (P, P, "raw")]),
                        ("rle_beside_raw", [(100, 4200, "rle"), (4300, 4300, "raw")])):
        seed += 1
        out[name] = (zstream(bs, spans, seed), {"position": name, "source": "+".join(s for _, _, s in spans)})
    return out


def _shuffled_case(cid, fam, s: Stream, ts, bs, tags, mode=1):
    return make(cid, fam, [[s]], comp=ZSTD, ts=ts, bs=bs, nbytes=bs, mode=mode, tags=tags)


def _alias_planes():
    return [_shuffled_case(f"planes_ts{ts}_{name}", "alias_planes", s, ts, bs, tags)
            for ts, bs in GEOMS for name, (s, tags) in plane_streams(ts, bs).items()]


# ---------------------------------------------------------------------------------------------------
# the rule's edges
# ---------------------------------------------------------------------------------------------------
def _reader_stream(via: str, delta: int, total=32768) -> Stream:
    """A raw candidate C of XDIRECT bytes that a later match reads (delta -1: the match source begins at
    C's last byte) or just misses (delta 0: at the first byte after it). via 'explicit': the match's own
    offset; 'rep0' / 'rep1' / 'rep2': a repeat offset that a block in FRONT of C set (the history runs
    across C: a raw block changes none of it) and a one-sequence block after C uses."""
    r = np.random.default_rng(len(via) * 10 + delta + 5)
    rb = lambda n: r.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    head = [Z.raw(rb(3000)), Z.raw(rb(3000))]
    gap, ll, ml = 1000, 10, 8
    T = gap + ll - delta  # y + ll - T == end of C + delta, y = end of C + gap
    offs = {"rep0": (600, 700, T), "rep1": (600, T, 700), "rep2": (T, 600, 700)}.get(via, (600, 700, 800))
    x = Z.cmp_block(rb(3 * 5 + 2), [(5, 6, o + 3) for o in offs])  # offset values 512 .. 1023: one code
    pos = 6000 + 3 * 11 + 2
    c_off = pos
    c = Z.raw(rb(XDIRECT))
    f = Z.raw(rb(gap))
    ov = T + 3 if via == "explicit" else {"rep0": 1, "rep1": 2, "rep2": 3}[via]
    y = Z.cmp_block(rb(ll + 3), [(ll, ml, ov)])
    used = c_off + XDIRECT + gap + ll + ml + 3
    blks = head + [x, c, f, y] + _fillers(total - used, 77 + delta)
    fr = Z.Frame(blks, "fcs4")
    dec = Z.execute([fr])
    assert len(dec) == total
    want = [(c_off, XDIRECT, "raw")] if delta == 0 else []
    return Stream(Z.build(fr), dec, "zstd", [fr], True, want)


def _alias_rule():
    out, ts, bs = [], 4, 32768

    def add(name, s, **tags):
        out.append(_shuffled_case(f"rule_{name}", "alias_rule", s, ts, bs, tags))

    for n in (XDIRECT - 1, XDIRECT, XDIRECT + 1):
        for source in ("raw", "rle", "lit_raw"):
            add(f"size_{n}_{source}", zstream(bs, [(PLANE, n, source)], n + len(source)), size=n, source=source)
    for k in (3, 4):
        spans = [(i * PLANE + 100 * i, XDIRECT + 8 * i, ("raw", "rle", "lit_raw", "lit_rle")[i]) for i in range(k)]
        add(f"{k}_candidates", zstream(bs, spans, 40 + k), candidates=k)
    for via in ("explicit", "rep0", "rep1", "rep2"):
        for delta, word in ((-1, "reads_last_byte"), (0, "starts_after")):
            add(f"match_{via}_{word}", _reader_stream(via, delta), via=via, delta=delta)
    # the checksummed twin of a stream whose blocks would all be candidates: libzstd's raw blocks
    noise = _rnd(bs, 4242)
    for ck in (False, True):
        enc = Z.stream_frame(noise, PLANE, checksum=ck)
        assert Z.blocks(enc) == [(Z.RAW, PLANE)] * 4 and frames_of(enc)[0][0] == ck
        want = [] if ck else [(0, PLANE, "raw"), (PLANE, PLANE, "raw")]
        add(f"raw_blocks_{'checksummed' if ck else 'plain'}", Stream(enc, noise, "zstd", None, True, want), checksum=ck)
    a = zstream(PLANE, [(0, PLANE, "raw")], 51, tail_match=False)
    b = zstream(bs - PLANE, [(1000, 5000, "rle")], 52)
    two = Stream(a.payload + b.payload, a.dec + b.dec, "zstd", a.parts + b.parts, True,
                 [(0, PLANE, "raw"), (PLANE + 1000, 5000, "rle")])
    add("two_frames", two, frames=len(two.parts))
    add("skippable_in_front", Stream(Z.skippable() + two.payload, two.dec, "zstd", two.parts, True, two.want), skippable=True)
    return out


# ---------------------------------------------------------------------------------------------------
# the plane streams in other layouts
# ---------------------------------------------------------------------------------------------------
def _alias_layouts():
    out = []
    ps = plane_streams(4, 32768)
    # split blocks: four frames of PLANE bytes, each with an alias of its own: plane i is stream i
    quarter = [zstream(PLANE, spans, 300 + i, tail_match=i % 2 == 0)
               for i, spans in enumerate(([(0, PLANE, "raw")], [(2000, 4500, "lit_huf")], [(0, 4096, "rle"), (4096, 4096, "lit_raw")],
                                          [(1, PLANE - 1, "lit_rle")]))]
    out.append(make("layout_split_ts4", "alias_layouts", [quarter], comp=ZSTD, ts=4, bs=32768, nbytes=32768, mode=1, split=True,
                    tags={"layout": "split"}))
    pick = ("on_plane_raw", "inside_plane_lit_huf", "two_planes_rle", "mid_to_mid_lit_raw", "one_before_boundary_lit_rle",
            "one_after_boundary_raw", "two_in_two_planes", "rle_beside_raw")
    for ts in (1, 3, 8, 16):
        for name in pick:
            out.append(make(f"layout_ts{ts}_{name}", "alias_layouts", [[ps[name][0]]], comp=ZSTD, ts=ts, bs=32768, nbytes=32768,
                            mode=1, tags={"layout": f"ts{ts}"}))
    for name in pick:
        out.append(make(f"layout_bitshuffle_{name}", "alias_layouts", [[ps[name][0]]], comp=ZSTD, ts=4, bs=32768, nbytes=32768,
                        mode=2, tags={"layout": "bitshuffle"}))
    # blocksize 32776: block 1 starts at 8 mod 16 and the u32 fast path must refuse it
    bs = 32776
    for name, spans in (("on_plane", [(8194, 8194, "raw")]), ("two_planes", [(8194, 16388, "lit_raw")]),
                        ("rle_plane", [(3 * 8194, 8194, "rle")])):
        blocks = [[zstream(bs, spans, 500 + b + len(name))] for b in range(2)]
        out.append(make(f"layout_bs32776_{name}", "alias_layouts", blocks, comp=ZSTD, ts=4, bs=bs, nbytes=2 * bs, mode=1,
                        tags={"layout": "bs32776"}))
    # two full blocks and a leftover block of 5000 bytes that carries an alias
    for source in SOURCES:
        blocks = [[ps["on_plane_" + source][0]], [ps["mid_to_mid_" + source][0]],
                  [zstream(5000, [(500, 4200, source)], 600 + len(source), tail_match=False)]]
        out.append(make(f"layout_leftover_{source}", "alias_layouts", blocks, comp=ZSTD, ts=4, bs=32768, nbytes=2 * 32768 + 5000,
                        mode=1, tags={"layout": "leftover", "source": source}))
    return out


# ---------------------------------------------------------------------------------------------------
# every hand-built zstd frame and DEFLATE stream, wrapped
# ---------------------------------------------------------------------------------------------------
ZSTD_WRAP_MAX = 65536


def _zstd_wrapped():
    out = []
    for f in Z.FAMILIES:
        for c in Z.FAMILIES[f]():
            n = len(c.expect)
            if n > ZSTD_WRAP_MAX:
                continue
            s = Stream(c.enc, c.expect, "zstd", c.specs, c.parallel)
            out.append(one_zstd(f"zstd_{f}_{c.name}", "zstd_wrapped", s, n, {"zstd_family": f, "zstd_case": c.name}))
    return out


def _zlib_stream(c: D.Case) -> Stream:
    return Stream(c.enc("zlib"), c.expect if c.status == D.OK else (c.decoded if c.status == D.SIZE else None), "zlib")


def _zlib_wrapped():
    out, small = [], []
    for f in D.FAMILIES:
        for c in D.family(f):
            s = _zlib_stream(c)
            out.append(make(f"zlib_{f}_{c.name}", "zlib_wrapped", [[s]], comp=ZLIB, ts=1, bs=c.size, nbytes=c.size,
                            tags={"deflate_family": f, "deflate_status": c.status}))
            if c.status == D.OK and c.size == 4096:
                small.append((f"{f}_{c.name}", s))
    for k in range(0, len(small) - len(small) % 4, 4):
        four = small[k:k + 4]
        out.append(make(f"zlib_split4_{k // 4}_{four[0][0]}", "zlib_wrapped", [[s for _, s in four]], comp=ZLIB, ts=4, bs=16384,
                        nbytes=16384, mode=1, split=True, tags={"split4": [n for n, _ in four]}))
    if len(small) % 4:  # the last ones again, with the first to fill the block
        four = (small[-(len(small) % 4):] + small)[:4]
        out.append(make(f"zlib_split4_last_{four[0][0]}", "zlib_wrapped", [[s for _, s in four]], comp=ZLIB, ts=4, bs=16384,
                        nbytes=16384, mode=1, split=True, tags={"split4": [n for n, _ in four]}))
    base = small[0][1]
    flipped = bytearray(base.payload)
    flipped[-2] ^= 0x10
    out.append(make("zlib_adler32_byte_flipped", "zlib_wrapped", [[Stream(bytes(flipped), None, "zlib")]], comp=ZLIB, ts=1, bs=4096,
                    nbytes=4096, tags={"trailer": "flipped"}))
    out.append(make("zlib_trailer_past_the_end", "zlib_wrapped", [[Stream(base.payload[:-2], None, "zlib")]], comp=ZLIB, ts=1,
                    bs=4096, nbytes=4096, tags={"trailer": "cut"}))
    return out


# ---------------------------------------------------------------------------------------------------
# wrong sizes
# ---------------------------------------------------------------------------------------------------
SIZES_NE = 4000  # sub_slot 4096


def _sized(kind: str, n: int, seed: int) -> Stream:
    """A stream of `kind` that decodes to n bytes, with no alias candidate in it."""
    if kind == "zstd":
        fr = Z.Frame(_fillers(n, seed), "fcs4")
        return Stream(Z.build(fr), Z.execute([fr]), "zstd", [fr])
    data = _rnd(n, seed)
    blocks = [D.Stored(data[o:o + 3000]) for o in range(0, n, 3000)]
    return Stream(D.zlib_wrap(D.deflate(blocks)[0], data), data, "zlib")


def _sizes():
    out, ne = [], SIZES_NE
    for kind, comp in (("zstd", ZSTD), ("zlib", ZLIB)):
        for tag, n in (("ne_minus_1", ne - 1), ("exact", ne), ("ne_plus_1", ne + 1), ("sub_slot_plus_1", sub_slot(ne) + 1)):
            out.append(make(f"sizes_{kind}_{tag}", "sizes", [[_sized(kind, n, n)]], comp=comp, ts=1, bs=ne, nbytes=ne,
                            tags={"kind": kind, "decodes_to": n, "ne": ne}))
        # far too long, in a leftover block whose ne is far below sub_slot
        blocks = [[_sized(kind, 3000, 31)], [_sized(kind, 20000, 32)]]
        out.append(make(f"sizes_{kind}_far_too_long_in_leftover", "sizes", blocks, comp=comp, ts=1, bs=3000, nbytes=ne,
                        tags={"kind": kind, "decodes_to": 20000, "ne": ne - 3000}))
        blocks = [[_sized(kind, 3000, 33)], [_sized(kind, 1000, 34)]]
        out.append(make(f"sizes_{kind}_leftover_exact", "sizes", blocks, comp=comp, ts=1, bs=3000, nbytes=ne,
                        tags={"kind": kind, "decodes_to": 1000, "ne": ne - 3000}))
    return out


def interleave(cases):
    """The cases in the order v c v c ..: every corrupt one beside valid ones, while there are any."""
    good, bad = [c for c in cases if c.status == OK], [c for c in cases if c.status != OK]
    out = []
    while good or bad:
        if good:
            out.append(good.pop(0))
        if bad:
            out.append(bad.pop(0))
    return out


# ---------------------------------------------------------------------------------------------------
# every compressor in one call
# ---------------------------------------------------------------------------------------------------
def _mixed():
    n, ts = 16384, 4
    out = []
    four = [zstream(4096, [(0, 4096, "raw")], 701, tail_match=False), zstream(4096, [], 702), zstream(4096, [(0, 4096, "rle")], 703,
                                                                                                        tail_match=False),
            zstream(4096, [], 704)]
    out.append(make("mixed_zstd_split", "mixed", [list(four)], comp=ZSTD, ts=ts, bs=n, nbytes=n, mode=1, split=True, tags={"kind": "zstd"}))
    zl = [_sized("zlib", 4096, 710 + i) for i in range(4)]
    out.append(make("mixed_zlib_split", "mixed", [zl], comp=ZLIB, ts=ts, bs=n, nbytes=n, mode=1, split=True, tags={"kind": "zlib"}))
    fr, chunk, _ = B.grid_frame("lz4", n, n, ts, True, mode=1, seed=5)
    out.append(Case("mixed_lz4", "mixed", n, fr.data, chunk, OK, B.COMP["lz4"], ts, n, 1, [], {"kind": "lz4"}))
    data = _rnd(n, 720)
    out.append(make("mixed_memcpy", "mixed", [[stored(data)]], comp=ZSTD, ts=ts, bs=n, nbytes=n, mode=1, memcpy=True, tags={"kind": "memcpy"}))
    one_stored = [four[0], stored(_rnd(4096, 721)), four[2], four[3]]
    out.append(make("mixed_zstd_one_stored_split", "mixed", [one_stored], comp=ZSTD, ts=ts, bs=n, nbytes=n, mode=1, split=True,
                    tags={"kind": "zstd+stored"}))
    return out


FAMILIES = {"zstd_wrapped": _zstd_wrapped, "alias_planes": _alias_planes, "alias_rule": _alias_rule,
            "alias_layouts": _alias_layouts, "zlib_wrapped": _zlib_wrapped, "sizes": _sizes, "mixed": _mixed}
ZSTD_FAMILIES = ("zstd_wrapped", "alias_planes", "alias_rule", "alias_layouts", "sizes", "mixed")
_cache = {}


def family(name):
    """The family's cases, built once."""
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
        assert len({c.id for c in _cache[name]}) == len(_cache[name]), name
    return _cache[name]


def all_cases():
    return [c for f in FAMILIES for c in family(f)]
