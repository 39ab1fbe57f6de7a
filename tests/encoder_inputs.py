"""Inputs that steer the GPU encoders (k_gzip_encode, k_zstd_encode_seg, k_lz4_encode<FMT>) to the
edges of their formats. Test infrastructure, no GPU, seeded, nothing on disk.

A Case is an input, the codec it goes through and its `intent`: [(the edge the case exists for, a
predicate over the view tests/encoded_inspect.py gives of the encoded chunk)], after
deflate_streams.Case.intent. tests/test_gpu_encoder_edges.py encodes every case on the GPU, decodes the
result with an independent decoder and asserts the intent.

The encoders parse 64 positions a step: every lane hashes the 4 bytes at its position (12 bits,
multiplicative), reads the bucket, then writes its own position; the parse of the step is greedy from
the lowest lane. So what an input makes the encoder do is decided by its 4-byte strings alone. The
inputs are put together by Buf from
  * fresh bytes: every 4-byte string they complete is new to the input, so no match can start there;
  * zero filler: one hash bucket, swallowed by matches among the zeros (whose distances depend on
    which lane's write to that bucket lands last: no intent looks at them);
  * planted copies of earlier fresh bytes at an exact distance and length, ended by a fresh byte.
The case builders check (Buf.bucket_holds) that the copy's source is what the bucket holds when the
copy's first position reads it: no other position hashes there between the source's step and the copy (the zero
filler included), so the outcome does not depend on the order of same-bucket writes within a step.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import encoded_inspect as I
import zstd_frames as ZF

HBITS = 12  # the three encoders' hash: (u32 at p * 0x9E3779B1) >> (32 - HBITS)


def hash4(g):
    return ((g * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - HBITS)


def gram(b, p):
    return b[p] | b[p + 1] << 8 | b[p + 2] << 16 | b[p + 3] << 24


class Unsteered(Exception):
    """A seed's input does not steer the encoder as meant: _retry takes the next seed."""


class Buf:
    """The input under construction. `seen`: every 4-byte string so far; `plants`: (source, position,
    length) of the planted copies."""

    def __init__(self, seed):
        self.b = bytearray()
        self.seen = set()
        self.rng = np.random.default_rng(seed)
        self.plants = []

    def __len__(self):
        return len(self.b)

    def _push(self, v, fresh):
        """Append byte v; fresh: refuse (False) if it completes a 4-byte string seen before."""
        self.b.append(v)
        if len(self.b) >= 4:
            g = gram(self.b, len(self.b) - 4)
            if fresh and g in self.seen:
                self.b.pop()
                return False
            self.seen.add(g)
        return True

    def fresh(self, n, alphabet=None, p=None, ne=None, before=None):
        """n bytes drawn from `alphabet` (default 1..255: never the filler's zero) with weights p, each
        completing a new 4-byte string; the first one differs from `ne` when given. before: the source of
        a copy planted next: the last byte differs from the byte before that source, and the string it
        forms with the source's first three bytes is new."""
        alphabet = np.arange(1, 256) if alphabet is None else np.asarray(alphabet)
        start = len(self.b)
        draws = iter(())
        while len(self.b) < start + n:
            for _ in range(200):
                v = next(draws, None)
                if v is None:
                    draws = iter(self.rng.choice(alphabet, 4096, p=p).tolist())
                    v = next(draws)
                if len(self.b) == start and ne is not None and v == ne:
                    continue
                if before is not None and len(self.b) == start + n - 1 and (
                        (before and v == self.b[before - 1]) or
                        v | int.from_bytes(self.b[before:before + 3], "little") << 8 in self.seen):
                    continue
                if self._push(v, True):
                    break
            else:
                raise AssertionError("the alphabet cannot continue without a repeated 4-byte string")
        return start

    def fresh_counts(self, symbols, counts):
        """Every symbols[i] exactly counts[i] times, each byte completing a new 4-byte string: drawn by
        what is left of each, stepping back a byte where nothing fits."""
        left, start, total = list(counts), len(self.b), sum(counts)
        tried = [set()]
        for _ in range(100 * total):
            if len(self.b) - start == total:
                return start
            cand = [i for i in range(len(symbols)) if left[i] and i not in tried[-1]]
            while cand:
                w = np.array([left[i] for i in cand], float)
                i = cand[int(self.rng.choice(len(cand), p=w / w.sum()))]
                tried[-1].add(i)
                if self._push(symbols[i], True):
                    left[i] -= 1
                    tried.append(set())
                    break
                cand.remove(i)
            else:
                if len(self.b) == start:
                    break
                v = self.b[-1]
                if len(self.b) >= 4:
                    self.seen.discard(gram(self.b, len(self.b) - 4))
                self.b.pop()
                left[list(symbols).index(v)] += 1
                tried.pop()
        raise Unsteered("no arrangement of the counts without a repeated 4-byte string")

    def fresh_to(self, pos, **kw):
        assert pos >= len(self.b), (pos, len(self.b))
        return self.fresh(pos - len(self.b), **kw)

    def zeros(self, n, v=0):
        """Filler of one byte value (zero unless the case's own alphabet holds it). The strings across
        its front edge are new when the byte before it is fresh and not the filler's; (v,v,v,v) repeats
        by design."""
        start = len(self.b)
        k = min(n, 8)
        for _ in range(k):
            self._push(v, False)
        self.b += bytes([v]) * (n - k)
        return start

    def zeros_to(self, pos, v=0):
        assert pos >= len(self.b), (pos, len(self.b))
        return self.zeros(pos - len(self.b), v)

    def extend_fresh(self, data):
        """Bytes made elsewhere (perm_bytes) that must be new here as well."""
        start = len(self.b)
        for x in data:
            if not self._push(x, True):
                raise Unsteered("a 4-byte string of the block occurred before")
        return start

    def raw(self, data):
        """Bytes as they are (runs, periodic patterns): repeats allowed."""
        start = len(self.b)
        for v in data:
            self._push(v, False)
        return start

    def plant(self, src, n, end=True):
        """A copy of the n bytes at src (it may overlap its own output), then, with `end`, one fresh byte
        that differs from the byte after the source: the copy is exactly n long. The byte before the copy
        must differ from the byte before the source, so no match can start earlier."""
        dst = len(self.b)
        assert 0 <= src < dst
        if src and self.b[src - 1] == self.b[dst - 1]:
            raise Unsteered("the bytes before the source and before the copy agree")
        if src >> 6 == dst >> 6:
            raise Unsteered("source and copy in one step: the copy's lane reads the bucket before the source's writes")
        for k in range(n):
            # the strings that reach back over the copy's front edge must be new, or a match starts early
            if not self._push(self.b[src + k], k < 3 and dst >= 3):
                raise Unsteered("a string across the copy's front edge occurred before")
        if end:
            self.fresh(1, ne=self.b[src + n])
        self.plants.append((src, dst, n))
        return dst

    def bytes(self):
        return bytes(self.b)

    # ---- build-time checks -------------------------------------------------------------------------
    def bucket_holds(self, src, dst, lo=0, skipped=lambda q: False):
        """True when the bucket of the string at src still names src when position dst reads it: no
        position q in [first position of src's step, dst) other than src, at or after `lo` (a segment's
        first inserted position) and not `skipped` (never inserted), has a string of the same hash."""
        b, n = self.b, len(self.b)
        h = hash4(gram(b, src))
        a = np.frombuffer(bytes(b) + b"\0\0\0", np.uint8).astype(np.uint64)
        g = a[:-3] | a[1:-2] << 8 | a[2:-1] << 16 | a[3:] << 24
        hs = ((g * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - HBITS)
        first = max(lo, src & ~63)  # steps start at multiples of 64 in all three encoders
        for q in np.nonzero(hs[first:min(dst, n - 3)] == h)[0] + first:
            if q != src and not skipped(int(q)):
                return False
        return True


def perm_bytes(symbols, reps, seed):
    """Every symbol exactly `reps` times (equal frequencies, so equal or adjacent Huffman code lengths
    in symbol order), as shuffled permutations, no 4-byte string twice."""
    rng = np.random.default_rng(seed)
    out, seen = bytearray(), set()
    for _ in range(reps):
        for _ in range(100):
            perm = rng.permutation(symbols).astype(np.uint8).tobytes()
            t = bytes(out[-3:]) + perm
            gs = [t[i:i + 4] for i in range(len(t) - 3)]
            if len(set(gs)) == len(gs) and not seen & set(gs):
                seen |= set(gs)
                out += perm
                break
        else:
            raise AssertionError("no fresh permutation")
    return bytes(out)


@dataclass
class Case:
    name: str
    codec: str          # gzip zlib zstd zstd_ck blosc-lz4 blosc-lz4hc blosc-blosclz blosc-snappy blosc-zlib blosc-zstd
    data: bytes
    intent: list        # [(the edge, predicate over view(case, enc))]
    blosc: dict = field(default_factory=dict)  # shuffle, typesize, blocksize of a blosc case


def blosc_conf(case):
    c = {"shuffle": "noshuffle", "typesize": 1, "blocksize": 0, "clevel": 5}
    c.update(case.blosc)
    return {"name": "blosc", "configuration": dict(c, cname=case.codec.split("-", 1)[1])}


def codec_metadata(case):
    """The zarr codec metadata after [bytes little] of the case's chain."""
    if case.codec == "gzip":
        return {"name": "gzip", "configuration": {"level": 1}}
    if case.codec == "zlib":
        return {"name": "numcodecs.zlib", "configuration": {"level": 1}}
    if case.codec in ("zstd", "zstd_ck"):
        return {"name": "zstd", "configuration": {"level": 3, "checksum": case.codec == "zstd_ck"}}
    return blosc_conf(case)


# ---------------------------------------------------------------------------------------------------
# views: what the intents look at
# ---------------------------------------------------------------------------------------------------
@dataclass
class DeflateView:
    blocks: list
    decoded: bytes
    matches: list = field(default_factory=list)   # (position, length, distance, length code, block index)
    literals: set = field(default_factory=set)    # positions coded as literals (stored bytes are not)
    starts: list = field(default_factory=list)    # the decoded position each block starts at

    def at(self, pos):
        return [m for m in self.matches if m[0] == pos]

    def covering(self, lo, hi):
        """The matches overlapping [lo, hi)."""
        return [m for m in self.matches if m[0] < hi and m[0] + m[1] > lo]


def deflate_view(blocks, decoded):
    v = DeflateView(blocks, decoded)
    pos = 0
    for i, b in enumerate(blocks):
        v.starts.append(pos)
        if b.btype == 0:
            pos += b.size
            continue
        for t in b.tokens:
            if t[0] == "L":
                v.literals.add(pos)
                pos += 1
            else:
                v.matches.append((pos, t[1], t[2], t[3], i))
                pos += t[1]
    assert pos == len(decoded)
    return v


@dataclass
class ZstdView:
    frame: object
    blocks: list
    seqs: list = field(default_factory=list)   # (position of the match, ll, ml, offset, block index)
    starts: list = field(default_factory=list)

    def at(self, pos):
        return [s for s in self.seqs if s[0] == pos]


def zstd_view(enc):
    (fr,) = I.zstd_frames(enc)
    v = ZstdView(fr, fr.blocks)
    pos = 0
    for i, b in enumerate(fr.blocks):
        v.starts.append(pos)
        if b.type == ZF.CMP:
            q = pos
            for ll, ml, ov in b.seqs:
                q += ll
                v.seqs.append((q, ll, ml, ov - 3, i))
                q += ml
        pos += b.size
    return v


@dataclass
class BloscView:
    frame: object
    streams: list          # per stream: None (stored), LzTokens, DeflateView or ZstdView
    matches: list = field(default_factory=list)  # lz streams: (stream, position in it, length, offset), pieces joined


def blosc_view(case, enc):
    f = I.blosc_streams(enc)
    kind = case.codec.split("-", 1)[1]
    v = BloscView(f, [])
    for i, s in enumerate(f.streams):
        if s.stored:
            v.streams.append(None)
        elif kind in ("lz4", "lz4hc", "blosclz", "snappy"):
            t = I.lz_tokens("lz4" if kind == "lz4hc" else kind, s.payload)
            assert len(t.decoded) == s.size
            v.streams.append(t)
            v.matches += [(i, p, ln, off) for ln, off, p in I.merged_matches(t)]
        elif kind == "zlib":
            v.streams.append(deflate_view(*I.zlib_stream(s.payload)))
        else:
            v.streams.append(zstd_view(s.payload))
    return v


def view(case, enc):
    if case.codec == "gzip":
        return deflate_view(*I.gzip_member(enc))
    if case.codec == "zlib":
        return deflate_view(*I.zlib_stream(enc))
    if case.codec.startswith("zstd"):
        return zstd_view(enc)
    return blosc_view(case, enc)


# ---------------------------------------------------------------------------------------------------
# gzip / zlib (k_gzip_encode): 16-bit hash positions, a 32 KiB window, matches of 4..258 bytes, blocks
# cut once more than 16384 - 64 symbols are pending at the end of a step
# ---------------------------------------------------------------------------------------------------
GZ_CUT = 16384 - 64


def _gz_skipped(q):
    return (q + 1) & 0xFFFF == 0  # k_gzip_encode never inserts these positions


def _retry(build, tries=40):
    """build(seed) -> value or None (a build-time check failed: a bucket shared, say); first success."""
    for seed in range(tries):
        try:
            out = build(seed)
        except Unsteered:
            continue
        if out is not None:
            return out
    raise AssertionError("no seed gives a steered input")


def _one_plant(src_pos, dist, n, seed, head=64, tail=24, zero_fill=True, **kw):
    """fresh head, the source A (n fresh bytes) at src_pos, zero filler (or fresh bytes), A again at
    src_pos + dist, a fresh tail; kw: the fresh bytes' alphabet. Returns (Buf, source, copy position)."""
    def build(k):
        B = Buf(1000 * seed + k)
        if src_pos >= head + 8:
            B.fresh(head, **kw)
            B.zeros_to(src_pos - 4)
        B.fresh_to(src_pos, **kw)
        a = B.fresh(n, **kw)
        B.fresh(1, **kw)
        if zero_fill and a + dist - 1 > len(B) + 2:
            B.zeros_to(a + dist - 1)
        else:
            B.fresh_to(a + dist - 1, **kw)
        B.fresh(1)
        assert len(B) == a + dist
        d = B.plant(a, n)
        B.fresh(tail, **kw)
        ok = all(B.bucket_holds(a + k0, d + k0, skipped=_gz_skipped) for k0 in range(0, max(n - 3, 1), 258))
        return (B, a, d) if ok and hash4(gram(B.b, a)) != 0 else None
    return _retry(build)


def _exact(pos, n, dist):
    """The planted copy is coded from its first byte as matches of that distance: 258s, then the rest
    (a rest below 4 bytes: literals)."""
    def pred(v):
        p, left = pos, n
        while left >= 4:
            m = v.at(p)
            if not m or m[0][2] != dist or m[0][1] != min(left, 258):
                return False
            p, left = p + m[0][1], left - m[0][1]
        return all(q in v.literals for q in range(p, p + left))
    return pred


def _only_literals(lo, hi):
    return lambda v: all(q in v.literals for q in range(lo, hi))


def _sane(v):
    return all(4 <= m[1] <= 258 and 1 <= m[2] <= 32768 for m in v.matches)


SANE = ("every match is 4..258 bytes long (the parse takes none below 4) at a distance of 1..32768", _sane)


def gzip_cases():
    out = []

    def add(name, B, intent, codec="gzip"):
        out.append(Case(name, codec, B.bytes() if isinstance(B, Buf) else bytes(B), [SANE] + intent))

    # ---- G1 window
    B, a, d = _one_plant(100, 32768, 40, 1)
    add("g1_dist_32768", B, [("a copy 32768 bytes back is a match at that distance", _exact(d, 40, 32768))])
    add("g1_dist_32768_zlib", B, [("a copy 32768 bytes back is a match at that distance", _exact(d, 40, 32768))], "zlib")
    B, a, d = _one_plant(100, 32769, 40, 2)
    add("g1_dist_32769", B, [("a copy 32769 bytes back is out of the window: literals", _only_literals(d, d + 40))])
    B = Buf(3)
    B.fresh(63)
    x = B.raw(bytes([77]) * 300)
    B.fresh(30, ne=77)
    add("g1_dist_1", B, [("a run whose first byte is a step's last lane: distance 1, 258 long",
                          lambda v, x=x: v.at(x + 1)[:1] == [(x + 1, 258, 1, 285, 0)] and x in v.literals)])
    # the position with (p + 1) % 65536 == 0 is never inserted: a copy of bytes starting there is found
    # one byte late; its neighbours are found whole
    for off, late in ((65534, 0), (65535, 1), (65536, 0)):
        B, a, d = _one_plant(off, 1000, 40, 10 + off % 8)
        add("g1_src_%d" % off, B,
            [("the source at %d %s" % (off, "is never inserted: the copy is a literal and a 39-byte match" if late
                                      else "is found whole"),
              (lambda v, d=d: d in v.literals and [m[:3] for m in v.at(d + 1)] == [(d + 1, 39, 1000)]) if late
              else _exact(d, 40, 1000))])
    # the cand >= p branch: the source's 16-bit position is above the copy's
    for page in (1, 2):
        B, a, d = _one_plant(65536 * page - 100, 300, 40, 20 + page)
        add("g1_wrap_page%d" % page, B, [("source below %d, copy above it: the candidate is rebuilt one 64 KiB page down"
                                         % (65536 * page), _exact(d, 40, 300))])
    B, a, d = _one_plant(65536 - 520, 500, 40, 23)
    assert d < 65536 < d + 40
    add("g1_copy_straddles_65536", B, [("a copy across position 65536", _exact(d, 40, 500))])

    # ---- G2 lengths: source, end byte, the copy, end byte, one after the other
    lens = (4, 5, 10, 11, 130, 131, 257, 258, 259, 261, 262, 516)

    def build(k):
        B = Buf(200 + k)
        B.fresh(70)
        spots = []
        for n in lens:
            a = B.fresh(n)
            B.fresh_to(max(len(B) + 2, (a | 63) + 1))  # the copy starts in a later step than its source
            d = B.plant(a, n)
            B.fresh(3)
            spots.append((a, d, n))
        ok = all(B.bucket_holds(a + k0, d + k0, skipped=_gz_skipped) for a, d, n in spots for k0 in range(0, n - 3, 258))
        return (B, spots) if ok else None
    B, spots = _retry(build)
    intent = [("a copy of %d bytes: %s" % (n, "258 and %d" % (n - 258) if n > 258 else "one match"), _exact(d, n, d - a))
              for a, d, n in spots]
    intent.append(("257 is code 284, 258 is code 285", lambda v: {m[3] for m in v.matches if m[1] == 257} == {284} and
                   {m[3] for m in v.matches if m[1] == 258} == {285} and len([m for m in v.matches if m[1] == 258]) >= 6))
    add("g2_lengths", B, intent)
    add("g2_lengths_zlib", B, intent, "zlib")

    # ---- G3 blocks: a block is cut when more than 16320 symbols are pending after a step. Inputs without
    # a repeated 4-byte string are all literals, one symbol a byte: n = 16384 is cut at its very end.
    skew = 1.0 / np.arange(8, 136)
    skewed = {"alphabet": np.arange(128), "p": skew / skew.sum()}  # about 6.4 bits a byte: a dynamic block pays
    for kind, kw in (("flat", {"alphabet": np.arange(256)}), ("skewed", skewed)):
        for n in (16320, 16384, 16448):
            B = Buf(300 + n)
            B.fresh(n, **kw)
            sizes = [n] if n <= GZ_CUT else [16384, n - 16384]
            bt = 0 if kind == "flat" else 2
            add("g3_%s_%d" % (kind, n), B, [
                ("blocks of %s bytes, the last one %s" % (sizes, "empty and fixed" if sizes[-1] == 0 else "not empty"),
                 lambda v, sizes=sizes, bt=bt: [b.size for b in v.blocks] == sizes and
                 # 64 literals never pay a dynamic header: the rest of 16448 is stored
                 [b.btype for b in v.blocks] == [bt if s > 64 else 0 if s else 1 for s in sizes] and not v.matches)])
    # a match that begins in the step that fills the block and ends beyond it
    def build(k):
        B = Buf(330 + k)
        a = B.fresh(100)
        B.fresh_to(16350)
        d = B.plant(a, 100)
        B.fresh(600)
        return (B, a, d) if B.bucket_holds(a, d, skipped=_gz_skipped) else None
    B, a, d = _retry(build)
    add("g3_match_across_cut", B, [("the step that fills the block ends in a 100-byte match: the block ends with it",
                                    lambda v, d=d: _exact(d, 100, d)(v) and v.at(d)[0][4] == 0 and v.starts[1] == d + 100
                                    and v.blocks[0].tokens[-1][0] == "M")])
    # dynamic, stored, dynamic, stored: a stored block's header in the middle of a byte
    B = Buf(340)
    for i in range(2):
        B.fresh(16384, **skewed)
        B.fresh(16384 if i == 0 else 5000, alphabet=np.arange(256))
    add("g3_mixed_blocks", B, [
        ("dynamic, stored, dynamic, stored", lambda v: [b.btype for b in v.blocks] == [2, 0, 2, 0]),
        ("a stored block's header starts inside a byte and is padded", lambda v: any(
            b.btype == 0 and (b.bitpos + 3) % 8 for b in v.blocks))])

    # ---- G4 headers
    # all 16 4-bit strings once: 19 bytes of {0, 255} without a repeated 4-byte string
    db = [0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1, 0, 0, 0]
    two = bytes(255 * x for x in db)
    assert len({two[i:i + 4] for i in range(16)}) == 16
    add("g4_two_symbols", two, [
        ("literals 0 and 255 only: 254 zero lengths between them are an 18 of 138 and a second run",
         lambda v: len(v.blocks) == 1 and v.blocks[0].btype == 2 and not v.matches and
         [c for c in v.blocks[0].clsyms if c[0] >= 17][:2] == [(18, 138), (18, 116)]),
        ("no distance code used: HDIST padded to two one-bit codes", lambda v: v.blocks[0].dd == [1, 1])])
    geo = 0.7 ** np.arange(12)  # skewed literals, so that the dynamic block pays for its header
    B, a, d = _one_plant(70, 200, 30, 41, tail=40, zero_fill=False, alphabet=np.arange(12) + 40, p=geo / geo.sum())
    add("g4_one_distance_code", B, [
        ("one match, one distance code used, a second one-bit code beside it",
         lambda v, d=d: _exact(d, 30, 200)(v) and len({I.DIST_BASE.index(max(x for x in I.DIST_BASE if x <= m[2]))
                                                        for m in v.matches}) == 1 and
         sorted(x for x in v.blocks[0].dd if x) == [1, 1])])
    out.append(_all_codes_case())
    out.append(fib_distances_case())
    for name, groups in (("a", [(1, 3), (0, 3), (1, 6), (0, 10), (1, 7), (0, 11), (1, 4), (0, 138), (1, 74)]),
                         ("b", [(1, 5), (0, 139), (1, 112)])):
        syms, runs, i = [], {0: [], 1: []}, 0
        for present, n in groups:
            if present:
                syms += range(i, i + n)
            runs[present].append(n)
            i += n
        assert i == 256
        data = perm_bytes(syms, 24, 400 + len(groups))
        add("g4_runs_" + name, data, [
            ("literal code lengths: zero runs of %s and equal lengths over %s symbols in a row" % (runs[0], runs[1][:-1]),
             lambda v, groups=groups: _has_runs(v.blocks[0].ll, groups)),
            ("the header's run-length coding is zlib's scan_tree / send_tree of those lengths",
             lambda v: all(b.clsyms == zlib_rle(b.ll) + zlib_rle(b.dd) for b in v.blocks if b.btype == 2))])
    return out


def _has_runs(ll, groups):
    """The code lengths have the groups' shape: zero exactly where a symbol is absent, and one length
    over each of the present groups but the last."""
    i = 0
    for k, (present, n) in enumerate(groups):
        part = ll[i:i + n]
        if present and (0 in part or (k < len(groups) - 1 and len(set(part)) != 1)):
            return False
        if not present and set(part) != {0}:
            return False
        i += n
    return True


def zlib_rle(lens):
    """zlib trees.c scan_tree / send_tree over one sequence of code lengths, as (symbol,) / (16 | 17 |
    18, repeat count): the reference k_gzip_encode's rle_lengths is held to."""
    out, n = [], len(lens)
    prevlen, count = -1, 0
    nextlen = lens[0]
    max_count, min_count = (138, 3) if nextlen == 0 else (7, 4)
    for i in range(n):
        curlen = nextlen
        nextlen = lens[i + 1] if i + 1 < n else -1
        count += 1
        if count < max_count and curlen == nextlen:
            continue
        if count < min_count:
            out += [(curlen,)] * count
        elif curlen != 0:
            if curlen != prevlen:
                out.append((curlen,))
                count -= 1
            out.append((16, count))
        elif count <= 10:
            out.append((17, count))
        else:
            out.append((18, count))
        count, prevlen = 0, curlen
        if nextlen == 0:
            max_count, min_count = 138, 3
        elif curlen == nextlen:
            max_count, min_count = 6, 3
        else:
            max_count, min_count = 7, 4
    return out


def _all_codes_case():
    """One block using every distance code (30) and every length code the parse can reach (258..285: it
    takes no 3-byte match, so 257 never occurs). Distances below 64 come from periodic runs whose first
    period ends a step (the next step's first lane finds the run's first position); the others from
    planted copies; the lengths from copies right behind their sources."""
    len_bases = I.LEN_BASE[1:]

    def build(k):
        B = Buf(500 + k)
        spots, small = [], []
        B.fresh(64)
        for dist in [x for x in I.DIST_BASE if x < 64]:
            B.fresh_to(len(B) + (-len(B) - dist) % 64 + (64 if (-len(B) - dist) % 64 < 8 else 0))
            assert (len(B) + dist) % 64 == 0
            s = len(B)
            B.fresh(dist)
            for j in range(40):
                B._push(B.b[s + j], False)
            B.fresh(1, ne=B.b[s + 40])
            small.append((s + dist, dist))
        srcs = {}
        for dist in sorted((x for x in I.DIST_BASE if x >= 64), reverse=True):  # the nearest source last
            B.fresh(4)
            srcs[dist] = B.fresh(12)
        B.fresh(4)
        for dist in sorted(srcs):
            tgt = srcs[dist] + dist
            if tgt - len(B) >= 8:
                B.fresh(2)
                B.zeros_to(tgt - 2)
            B.fresh_to(tgt)
            spots.append((srcs[dist], B.plant(srcs[dist], 12), 12))
        B.fresh(5)
        for n in len_bases:
            a = B.fresh(n)
            B.fresh_to(max(len(B) + 2, (a | 63) + 1))
            spots.append((a, B.plant(a, n), n))
        B.fresh(9)
        ok = all(B.bucket_holds(a, d, skipped=_gz_skipped) for a, d, n in spots)
        ok = ok and all(B.bucket_holds(p - dist, p) for p, dist in small)
        return (B, spots, small) if ok else None
    B, spots, small = _retry(build)
    intent = [SANE,
              ("every planted copy is one match at its distance", lambda v: all(_exact(d, n, d - a)(v) for a, d, n in spots)),
              ("every periodic run is a match at its period", lambda v: all(
                  any(m[2] == dist for m in v.at(p)) for p, dist in small)),
              ("all 30 distance codes and 28 of the 29 length codes (258..285; 257 is a 3-byte match) in one "
               "dynamic block", lambda v: len(v.blocks) == 1 and
               v.blocks[0].btype == 2 and all(v.blocks[0].dd[c] for c in range(30)) and v.blocks[0].hdist == 30 and
               {m[3] for m in v.matches} == set(range(258, 286)))]
    return Case("g4_all_codes", "gzip", B.bytes(), intent)


# ---------------------------------------------------------------------------------------------------
# zstd (k_zstd_encode_seg, k_zstd_frame): blocks of 64 KiB, superblocks of 512 KiB, segments of 1 MiB
# (each warming its hash table with the 16 KiB before it); matches of 4 bytes and more that never cross
# a block end; 16-bit literal and match lengths in a sequence record
# ---------------------------------------------------------------------------------------------------
ZBLK, ZSB, ZSEG, ZWARM = 65536, 8 * 65536, 1 << 20, 16384


def _seq(pos, ll=None, ml=None, off=None):
    """A sequence whose match starts at pos, with the given fields (None: any)."""
    def pred(v):
        return any((ll is None or s[1] == ll) and (ml is None or s[2] == ml) and (off is None or s[3] == off)
                   for s in v.at(pos))
    return pred


NO_REPEAT = ("every Offset_Value is 4 or more: no repeat-offset codes", lambda v: all(s[3] >= 1 for s in v.seqs))


def _second_block(seed, lits, src_len=100, fill=0, tail_plant=True):
    """Block 0: fresh bytes holding a source, then filler to 64 KiB. Block 1: `lits` (a callable adding
    them to the Buf) and a planted copy of the source, which ends the input: the block's literals are
    exactly what `lits` added. Returns (Buf, first literal, copy position)."""
    def build(k):
        B = Buf(7000 + 100 * seed + k)
        B.fresh(70, alphabet=np.arange(2, 254))
        # many literals evict most buckets: several candidate sources, the first that survives is planted
        srcs = []
        for _ in range(48):
            srcs.append(B.fresh(src_len, alphabet=np.arange(2, 254)))
            B.fresh(2, alphabet=np.arange(2, 254))
        B.zeros_to(ZBLK, fill)
        a = len(B)
        lits(B)
        for s in srcs:
            if B.bucket_holds(s, len(B)) and hash4(gram(B.b, s)) != hash4(fill * 0x01010101) and \
                    B.b[s - 1] != B.b[-1]:
                return B, a, B.plant(s, src_len, end=False)
        return None
    return _retry(build)


def _lit_block(name, seed, lits, intent, fill=0, codec="zstd"):
    B, a, d = _second_block(seed, lits, fill=fill)
    n = d - a
    return Case(name, codec, B.bytes(), [NO_REPEAT, ("block 1 holds the %d literals and one sequence" % n,
                                                     lambda v, n=n, d=d: v.blocks[1].type == ZF.CMP and
                                                     v.blocks[1].regen == n and v.blocks[1].nseq == 1 and
                                                     _seq(d, n, 100)(v))] + intent)


def zstd_cases():
    out = []
    # ---- Z1 frame header and block structure
    for n in (255, 256, 65791, 65792, 65535, 65536, 65537, 131072, 131073):
        B = Buf(600 + n % 97)
        B.fresh(min(n, 100))
        B.zeros_to(n - 8)
        B.fresh_to(n)
        fcs = 1 if n <= 255 else 2 if n <= 65791 else 4
        nb = -(-n // ZBLK)
        sizes = [ZBLK] * (nb - 1) + [n - ZBLK * (nb - 1)]
        for codec in ("zstd", "zstd_ck") if n in (256, 65792, 65537) else ("zstd",):
            out.append(Case("z1_n%d%s" % (n, "_ck" if codec == "zstd_ck" else ""), codec, B.bytes(), [NO_REPEAT, (
                "a content size field of %d bytes, %d blocks of %s" % (fcs, nb, sizes),
                lambda v, fcs=fcs, sizes=sizes, n=n, ck=codec == "zstd_ck": v.frame.fcs_bytes == fcs and
                v.frame.content_size == n and [b.size for b in v.blocks] == sizes and v.frame.checksum == ck and
                [b.last for b in v.blocks] == [False] * (len(sizes) - 1) + [True])]))

    # ---- Z2 literals section headers
    for n, hdr in ((31, 1), (32, 2), (4095, 2), (4096, 3)):
        flat = perm_bytes(np.arange(256), 16, 610 + n)[:n]
        for codec in ("zstd", "zstd_ck") if n == 32 else ("zstd",):
            out.append(_lit_block("z2_raw_%d%s" % (n, "_ck" if codec == "zstd_ck" else ""), n,
                                  lambda B, flat=flat: B.extend_fresh(flat),
                                  [("%d flat literals: a raw section with a %d-byte header" % (n, hdr),
                                    lambda v, hdr=hdr: (v.blocks[1].ltype, v.blocks[1].lhdr) == (0, hdr))], codec=codec))

    def rle_block(k):
        B = Buf(620 + k)
        B.fresh(70)
        s1 = B.fresh(100)
        B.fresh(2)
        s2 = B.fresh(100)
        B.fresh(2)
        B.zeros_to(ZBLK)
        spots = []
        for s in (s1, s2):
            B.raw(b"\x07")
            if B.b[s + 100] == 7 or B.b[s - 1] == 7:
                return None
            spots.append((s, B.plant(s, 100, end=False)))
        B.raw(b"\x07")
        return (B, spots) if all(B.bucket_holds(s, d) for s, d in spots) else None
    B, spots = _retry(rle_block)
    out.append(Case("z2_rle_literals", "zstd", B.bytes(), [NO_REPEAT, (
        "three literals of one value around two matches: an RLE literals section",
        lambda v, spots=spots: (v.blocks[1].ltype, v.blocks[1].regen, v.blocks[1].nseq) == (1, 3, 2) and
        all(_seq(d, 1, 100)(v) for _, d in spots))]))
    skew = 1.0 / np.arange(8, 136)
    for n, streams, sf in ((1023, 1, 0), (1024, 4, 2), (1025, 4, 2), (1026, 4, 2), (1027, 4, 2), (16383, 4, 2), (16384, 4, 3)):
        for codec in ("zstd", "zstd_ck") if n == 1024 else ("zstd",):
            out.append(_lit_block("z2_huf_%d%s" % (n, "_ck" if codec == "zstd_ck" else ""), n,
                                  lambda B, n=n: B.fresh(n, alphabet=np.arange(128), p=skew / skew.sum()),
                                  [("%d skewed literals: Huffman, %d stream(s), Size_Format %d" % (n, streams, sf),
                                    lambda v, streams=streams, sf=sf: (v.blocks[1].ltype, v.blocks[1].streams, v.blocks[1].sf)
                                    == (2, streams, sf))], codec=codec))

    # ---- Z3 tree descriptions
    db = [0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1, 0, 0, 0]  # every 4-bit string once
    for a, b, tree in ((0, 1, "direct"), (254, 255, "fse"), (0, 255, "fse")):
        two = bytes(b if x else a for x in db)
        out.append(_lit_block("z3_two_symbols_%d_%d" % (a, b), a + b, lambda B, two=two: B.raw(two),
                              [("literals of {%d, %d} only: Huffman with a %s tree description" % (a, b, tree),
                                lambda v, tree=tree: (v.blocks[1].ltype, v.blocks[1].tree) == (2, tree))], fill=0x80))
    geo = 0.6 ** np.arange(8)
    for codec, ck in (("zstd", ""), ("zstd_ck", "_ck")):  # the checksum trailer behind each kind of tree
        out.append(_lit_block("z3_direct_weights" + ck, 31, lambda B: B.fresh(500, alphabet=np.arange(8), p=geo / geo.sum()),
                              [("the 8 lowest symbols, skewed: 4-bit weights (an FSE description cannot be shorter)",
                                lambda v: (v.blocks[1].ltype, v.blocks[1].tree) == (2, "direct"))], fill=0x80, codec=codec))
    bell = np.exp(-((np.arange(256) - 128.0) / 18) ** 2 / 2)
    for codec, ck in (("zstd", ""), ("zstd_ck", "_ck")):
        out.append(_lit_block("z3_fse_weights" + ck, 32, lambda B: B.fresh(6000, alphabet=np.arange(256), p=bell / bell.sum()),
                              [("a bell curve over the byte range: FSE-compressed weights",
                                lambda v: (v.blocks[1].ltype, v.blocks[1].tree) == (2, "fse"))], fill=0, codec=codec))
    flat200 = perm_bytes(np.arange(200) + 20, 40, 633)
    out.append(_lit_block("z3_flat_200", 33, lambda B: B.extend_fresh(flat200),
                          [("8000 literals flat over 200 symbols (codes of 7 and 8 bits): the FSE description pays, "
                            "Huffman literals", lambda v: (v.blocks[1].ltype, v.blocks[1].tree) == (2, "fse"))]))
    # Fibonacci frequencies 1, 1, 2, .. 233 over 13 symbols (an optimal code 12 deep) under 11 symbols of
    # 250 each: 24 symbols whose optimal code is 14 bits deep, so the encoder's sits at Max_Number_of_Bits.
    # The equal heavy symbols leave room for 3359 literals without a repeated 4-byte string.
    fib = [1, 1]
    while len(fib) < 13:
        fib.append(fib[-1] + fib[-2])
    for codec, ck in (("zstd", ""), ("zstd_ck", "_ck")):
        out.append(_lit_block("z3_fibonacci_24" + ck, 34, lambda B: B.fresh_counts(list(range(1, 25)), fib + [250] * 11),
                              [("Fibonacci frequencies under 11 equal ones, 24 symbols: Huffman literals with codes at "
                                "the 11-bit limit", lambda v: (v.blocks[1].ltype, v.blocks[1].max_bits) == (2, 11))],
                              fill=0x80, codec=codec))

    # ---- Z4 sequences
    for ns in (127, 128):
        def build(k, ns=ns):
            B = Buf(640 + ns + 10 * k)
            B.fresh(70)
            s = B.fresh(12)
            B.fresh(2)
            B.zeros_to(ZBLK)
            for _ in range(ns):
                B.fresh(3, ne=B.b[s + 12], before=s)
                B.plant(s, 12, end=False)
            B.fresh(5)
            return B
        B = _retry(build)
        out.append(Case("z4_nseq_%d" % ns, "zstd", B.bytes(), [NO_REPEAT, (
            "%d sequences in block 1: Number_of_Sequences in %d byte(s)" % (ns, 1 if ns < 128 else 2),
            lambda v, ns=ns: v.blocks[1].nseq == ns and all(s[2] == 12 and s[1] == 3 for s in v.seqs if s[4] == 1))]))
    # offsets 1..4: a run of that period whose first period ends a step
    B = Buf(650)
    B.fresh(64)
    runs = []
    for d in (1, 2, 3, 4):
        B.fresh_to(len(B) + (-len(B) - d) % 64 + (64 if (-len(B) - d) % 64 < 8 else 0))
        s = B.fresh(d)
        for j in range(50):
            B._push(B.b[s + j], False)
        B.fresh(1, ne=B.b[s + 50])
        runs.append((s + d, d))
    B.fresh(20)
    for codec in ("zstd", "zstd_ck"):
        out.append(Case("z4_offsets_1_to_4" + ("_ck" if codec == "zstd_ck" else ""), codec, B.bytes(), [NO_REPEAT] + [
            ("a run of period %d: a 50-byte match at offset %d, Offset_Value %d" % (d, d, d + 3), _seq(p, None, 50, d))
            for p, d in runs]))

    def offsets_case(k):
        B = Buf(660 + k)
        B.fresh(64)
        # sources: the farthest pair first; within a pair the two sources 16 apart, as their copies are
        srcs = []
        for kk in (19, 17, 16, 13, 10, 7):
            for o in ((1 << kk) - 4, (1 << kk) - 3):
                B.fresh(4)
                srcs.append((o, B.fresh(12)))
        srcs.sort(key=lambda t: -(t[0] + t[1]))
        spots = []
        for o, s in reversed(srcs):
            if s + o - len(B) >= 12:
                B.fresh(2)
                B.zeros_to(s + o - 2)
            B.fresh_to(s + o)
            if (len(B) & 0xFFFF) > 0xFFFF - 16:
                return None  # the copy would cross a block end
            spots.append((s, B.plant(s, 12), o))
        B.fresh(8)
        return (B, spots) if all(B.bucket_holds(s, d) for s, d, _ in spots) else None
    B, spots = _retry(offsets_case)
    out.append(Case("z4_offset_code_edges", "zstd", B.bytes(), [NO_REPEAT] + [
        ("offset %d = 2^k - %d: Offset_Value %d, the %s of its code" % (o, 3 if (o + 3) & (o + 2) == 0 else 4, o + 3,
                                                                          "first" if (o + 3) & (o + 2) == 0 else "last"),
         _seq(d, None, 12, o)) for s, d, o in spots]))

    def adjacent(k):
        B = Buf(670 + k)
        B.fresh(70)
        s1 = B.fresh(20)
        B.fresh(3)
        s2 = B.fresh(20)
        B.fresh(40)
        if B.b[s1 + 20] == B.b[s2]:
            return None
        d1 = B.plant(s1, 20, end=False)
        d2 = B.plant(s2, 20)
        B.fresh(10)
        return (B, d1, d2) if B.bucket_holds(s1, d1) and B.bucket_holds(s2, d2) else None
    B, d1, d2 = _retry(adjacent)
    out.append(Case("z4_adjacent_matches", "zstd", B.bytes(), [NO_REPEAT, (
        "a match right behind another: a literal length of 0 (no repeat code meant by it)",
        lambda v, d1=d1, d2=d2: _seq(d1, None, 20)(v) and _seq(d2, 0, 20)(v))]))

    lls = (15, 16, 23, 24, 31, 32, 47, 48, 63, 64)
    mls = (34, 35, 42, 43, 50, 51, 66, 67, 98, 99, 130, 131)

    def codes_case(k):
        B = Buf(680 + k)
        B.fresh(64)
        s0 = B.fresh(8)
        B.fresh(3)
        srcs = []
        for ml in mls:
            srcs.append((B.fresh(ml), ml))
            B.fresh(3)
        B.fresh_to((len(B) | 63) + 1, before=s0)
        d0 = B.plant(s0, 8, end=False)  # a first match, so that the next literal length is exact
        spots, prev = [], s0 + 8
        for i, (s, ml) in enumerate(srcs):
            ll = lls[i % len(lls)]
            B.fresh(ll, ne=B.b[prev], before=s)
            spots.append((s, B.plant(s, ml, end=False), ml, ll))
            prev = s + ml
        B.fresh(12, ne=B.b[prev])
        return (B, spots) if all(B.bucket_holds(s, d) for s, d, _, _ in spots) and B.bucket_holds(s0, d0) else None
    B, spots = _retry(codes_case)
    for codec in ("zstd", "zstd_ck"):
        out.append(Case("z4_ll_ml_code_edges" + ("_ck" if codec == "zstd_ck" else ""), codec, B.bytes(), [NO_REPEAT] + [
            ("literal length %d and match length %d, at the edges of their codes" % (ll, ml), _seq(d, ll, ml, d - s))
            for s, d, ml, ll in spots]))
    out.append(Case("z4_zero_blocks", "zstd", bytes(2 * ZBLK), [NO_REPEAT, (
        "64 KiB of zeros behind zeros: one match at the 16-bit limit of 65535 and one literal",
        lambda v: v.blocks[1].type == ZF.CMP and [s[1:3] for s in v.seqs if s[4] == 1] == [(0, 65535)] and
        v.blocks[1].regen == 1)]))

    def across(k):
        B = Buf(690 + k)
        B.fresh(70)
        s = B.fresh(40)
        B.fresh(2)
        B.zeros_to(ZBLK - 22)
        B.fresh(2)
        d = B.plant(s, 40)
        B.fresh(30)
        return (B, s, d) if B.bucket_holds(s, d) and B.bucket_holds(s + 20, d + 20) else None
    B, s, d = _retry(across)
    assert d == ZBLK - 20
    out.append(Case("z4_copy_across_block_end", "zstd", B.bytes(), [NO_REPEAT, (
        "a 40-byte copy across a block end: 20 bytes in each block, the second with no literals before it",
        lambda v, s=s, d=d: _seq(d, None, 20, d - s)(v) and _seq(d + 20, 0, 20, d - s)(v))]))

    # ---- Z5 superblocks and segments: 1 MiB + 70 KiB
    for name, back, found in (("in", ZWARM, True), ("out", ZWARM + 1, False)):
        def seg_case(k, back=back):
            B = Buf(700 + k + back)
            B.fresh(70)
            s_blk = B.fresh(24)
            B.fresh(3)
            s_sb = B.fresh(24)
            B.fresh(3)
            B.zeros_to(ZBLK + 500 - 2)
            B.fresh(2)
            d_blk = B.plant(s_blk, 24)
            B.zeros_to(ZSB + 500 - 2)
            B.fresh(2)
            d_sb = B.plant(s_sb, 24)
            B.zeros_to(ZSEG - back - 2)
            B.fresh(2)
            s_seg = B.fresh(24)
            B.fresh(2)
            B.zeros_to(ZSEG + 1000 - 2)
            B.fresh(2)
            d_seg = B.plant(s_seg, 24)
            B.zeros_to(ZSEG + 70 * 1024 - 8)
            B.fresh(8)
            ok = B.bucket_holds(s_blk, d_blk) and B.bucket_holds(s_sb, d_sb)
            ok = ok and B.bucket_holds(s_seg + (back - ZWARM), d_seg + (back - ZWARM), lo=ZSEG - ZWARM)
            return (B, (s_blk, d_blk), (s_sb, d_sb), (s_seg, d_seg)) if ok else None
        B, blk, sb, seg = _retry(seg_case)
        intent = [NO_REPEAT,
                  ("a source in the previous block is found", _seq(blk[1], None, 24, blk[1] - blk[0])),
                  ("a source in the previous superblock is found", _seq(sb[1], None, 24, sb[1] - sb[0])),
                  ("18 blocks: 16 in the first segment, 2 in the second", lambda v: len(v.blocks) == 18)]
        if found:
            intent.append(("a source at the first warmed-up position before the segment is found",
                           _seq(seg[1], None, 24, seg[1] - seg[0])))
        else:
            intent.append(("a source one byte before the warm-up: found from its second byte",
                           _seq(seg[1] + 1, None, 23, seg[1] - seg[0])))
        out.append(Case("z5_segments_warm_" + name, "zstd", B.bytes(), intent))
        if found:
            out.append(Case("z5_segments_warm_in_ck", "zstd_ck", B.bytes(), intent))
            # blocks of 1 MiB + 4 KiB and a short last one: the zstd streams of one launch have unequal
            # lengths, the short one leaves its second (item, segment) unit idle
            # the first stream holds every planted copy at the position it has in the chunk, and its second
            # segment starts where the chunk's does: the same sequences are asked of it
            first = [(text, lambda v, pred=pred: pred(v.streams[0])) for text, pred in intent[:3] + intent[4:]]
            out.append(Case("z5_blosc_zstd_unequal_streams", "blosc-zstd", B.bytes(), [
                ("two streams of unequal length, both compressed", lambda v: [s is not None for s in v.streams] == [True, True]
                 and [s.size for s in v.frame.streams] == [ZSEG + 4096, 70 * 1024 - 4096]),
                ("no repeat-offset codes in the second stream either, which is two blocks",
                 lambda v: NO_REPEAT[1](v.streams[1]) and [b.size for b in v.streams[1].blocks] == [ZBLK, 2048]),
                ("the first stream has 17 blocks: 16 in its first segment, one of 4 KiB in its second",
                 lambda v: [b.size for b in v.streams[0].blocks] == [ZBLK] * 16 + [4096])] + first,
                blosc={"blocksize": ZSEG + 4096}))
    return out


# ---------------------------------------------------------------------------------------------------
# blosc (k_lz4_encode<FMT>; blosc_enc.hip's framing): noshuffle, typesize 1 and the automatic block size
# make a chunk of up to 128 KiB one block and one stream
# ---------------------------------------------------------------------------------------------------
LZ_FMTS = ("lz4", "blosclz", "snappy")


def _lz_sane(v):
    """No match starts in a stream's last 12 bytes or reaches into its last 5 (the LZ4 block format's
    rule, which the encoder keeps for all three formats), and none is shorter than 4."""
    size = {i: s.size for i, s in enumerate(v.frame.streams)}
    return all(ln >= 4 and p < size[i] - 12 and p + ln <= size[i] - 5 and off >= 1 for i, p, ln, off in v.matches)


LZ_SANE = ("no match starts in the last 12 bytes or reaches the last 5; none is shorter than 4", _lz_sane)


def _lz_match(pos, ln=None, off=None, stream=0):
    return lambda v: any(m[0] == stream and m[1] == pos and (ln is None or m[2] == ln) and (off is None or m[3] == off)
                         for m in v.matches)


def _lz_literal(lo, hi, stream=0):
    """No match covers any of [lo, hi)."""
    return lambda v: not any(m[0] == stream and m[1] < hi and m[1] + m[2] > lo for m in v.matches)


def _runs_case(seed, lls, mls, first_src=8):
    """Sources of the lengths mls, then from a step's first lane: a short first match, and per length a
    literal run (lls, cycled) and the planted copy. Returns (Buf, [(source, copy position, ml, ll)])."""
    def build(k):
        B = Buf(seed + k)
        B.fresh(64)
        s0 = B.fresh(first_src)
        B.fresh(3)
        srcs = []
        for ml in mls:
            srcs.append((B.fresh(ml), ml))
            B.fresh(3)
        B.fresh_to((len(B) | 63) + 1, before=s0)
        d0 = B.plant(s0, first_src, end=False)
        spots, prev = [], s0 + first_src
        for i, (s, ml) in enumerate(srcs):
            ll = lls[i % len(lls)]
            B.fresh(ll, ne=B.b[prev], before=s)
            spots.append((s, B.plant(s, ml, end=False), ml, ll))
            prev = s + ml
        B.fresh(40, ne=B.b[prev])
        ok = all(B.bucket_holds(s, d) for s, d, _, _ in spots) and B.bucket_holds(s0, d0)
        return (B, spots) if ok else None
    return _retry(build, 200)


def blosc_cases():
    out = []

    def add(name, fmt, data, intent, **blosc):
        out.append(Case(name, "blosc-" + fmt, bytes(data), intent, blosc=blosc))

    memcpyed = ("nothing to gain: a memcpyed frame", lambda v: v.frame.memcpyed)
    # ---- B1 common to the three formats (lz4hc takes lz4's kernel: one case)
    for fmt in LZ_FMTS + ("lz4hc",):
        if fmt != "lz4hc":
            for n in list(range(1, 14)) + [16, 17]:
                add("b1_%s_%dbytes" % (fmt, n), fmt, bytes([65]) * n if n % 2 else bytes(range(1, n + 1)), [memcpyed])

        def tail_case(k, start_back, ln):
            B = Buf(800 + k)
            B.fresh(64)
            s = B.fresh(ln)
            B.fresh_to(192 - start_back, before=s)
            d = B.plant(s, ln, end=False)
            assert len(B) <= 192
            B.fresh_to(192)
            return (B, s, d) if B.bucket_holds(s, d) else None
        B, s, d = _retry(lambda k: tail_case(k, 12, 8))
        add("b1_%s_copy_in_last_12" % fmt, fmt, B.bytes(), [LZ_SANE, (
            "a copy starting 12 bytes before the end stays literals", _lz_literal(d, d + 8))])
        B, s, d = _retry(lambda k: tail_case(k, 30, 30))
        add("b1_%s_copy_into_last_5" % fmt, fmt, B.bytes(), [LZ_SANE, (
            "a copy that runs to the end is cut 5 bytes before it: 25 of its 30 bytes", _lz_match(d, 25, d - s))])
        B, spots = _runs_case(810, (14, 15, 16, 269, 270, 271), (18, 19, 20, 273, 274, 275, 40, 120))
        intent = [LZ_SANE] + [("%d literals, then a match of %d" % (ll, ml), _lz_match(d, ml, d - s)) for s, d, ml, ll in spots]
        if fmt in ("lz4", "lz4hc"):
            intent.append(("literal runs of 14 / 15.. / 270.. take 0 / 1 / 2 length bytes, matches of 18 / 19.. / 274.. too",
                           lambda v: {(e[1], e[2]) for e in v.streams[0].elements if e[0] == "lit"} >=
                           {(14, 0), (15, 1), (16, 1), (269, 1), (270, 2), (271, 2)} and
                           {(e[1], e[3]) for e in v.streams[0].elements if e[0] == "match"} >=
                           {(18, 0), (19, 1), (20, 1), (273, 1), (274, 2), (275, 2)}))
        add("b1_%s_runs_and_matches" % fmt, fmt, B.bytes(), intent)

    # ---- B2 lz4: the 16-bit offset
    for fmt in ("lz4", "lz4hc"):
        B, a, d = _one_plant(100, 65535, 40, 31)
        add("b2_%s_offset_65535" % fmt, fmt, B.bytes(), [LZ_SANE, ("a copy 65535 bytes back is found", _lz_match(d, 40, 65535))])
        B, a, d = _one_plant(100, 65536, 40, 32)
        add("b2_%s_offset_65536" % fmt, fmt, B.bytes(), [LZ_SANE, ("a copy 65536 bytes back stays literals",
                                                                   _lz_literal(d, d + 40))])
    B, a, d = _one_plant(100, 65536, 40, 32)
    add("b4_snappy_offset_65536", "snappy", B.bytes(), [LZ_SANE, ("a copy 65536 bytes back stays literals",
                                                                 _lz_literal(d, d + 40))])

    # ---- B3 blosclz
    B, spots = _runs_case(830, (32, 33, 64, 65), (8, 9, 263, 264, 265))
    add("b3_blosclz_lengths", "blosclz", B.bytes(), [LZ_SANE] + [
        ("%d literals, then a match of %d" % (ll, ml), _lz_match(d, ml, d - s)) for s, d, ml, ll in spots] + [
        ("matches of 8 / 9, 263 / 264, 265 take 0 / 1 / 2 length bytes; literal runs are cut at 32",
         lambda v: {(e[1], e[3][1]) for e in v.streams[0].elements if e[0] == "match"} >=
         {(8, 0), (9, 1), (263, 1), (264, 2), (265, 2)} and max(v.streams[0].lits) == 32)])
    for dist, found in ((8191, True), (8192, True), (8193, True), (73727, True), (73728, False)):
        B, a, d = _one_plant(100, dist, 40, 840 + dist % 7)
        form = "near" if dist <= 8191 else "far"
        add("b3_blosclz_distance_%d" % dist, "blosclz", B.bytes(), [LZ_SANE, (
            ("a copy %d bytes back: a %s match" % (dist, form)) if found else "a copy 73728 bytes back stays literals",
            (lambda v, d=d, dist=dist, form=form: _lz_match(d, 40, dist)(v) and
             any(e[0] == "match" and e[2] == dist and e[3][0] == form for e in v.streams[0].elements))
            if found else _lz_literal(d, d + 40))])

    # ---- B4 snappy
    B, spots = _runs_case(850, (60, 61, 256, 257), (64, 65, 67, 68, 128, 129))
    pieces = {64: [64], 65: [60, 5], 67: [60, 7], 68: [64, 4], 128: [64, 64], 129: [64, 60, 5]}

    def sn_pieces(v, spots=spots):
        el, pos, at = v.streams[0].elements, 0, {}
        for e in el:
            at.setdefault(pos, e)
            pos += e[1]
        for s, d, ml, ll in spots:
            got, p = [], d
            while sum(got) < ml:
                if p not in at or at[p][0] != "match" or at[p][2] != d - s:
                    return False
                got.append(at[p][1])
                p += at[p][1]
            if got != pieces[ml]:
                return False
        return True
    add("b4_snappy_literals_and_copies", "snappy", B.bytes(), [LZ_SANE] + [
        ("%d literals, then a match of %d" % (ll, ml), _lz_match(d, ml, d - s)) for s, d, ml, ll in spots] + [
        ("matches of 64, 65, 67, 68, 128, 129 are the copies %s" % pieces, sn_pieces),
        ("literals of 60 / 61.. / 257 take 0 / 1 / 2 length bytes", lambda v: {(e[1], e[2]) for e in
                                                                              v.streams[0].elements if e[0] == "lit"} >=
         {(60, 0), (61, 1), (256, 1), (257, 2)})])
    for ln in (11, 12):
        for off in (2047, 2048):
            B, a, d = _one_plant(100, off, ln, 860 + ln + off % 5)
            tag = 1 if ln <= 11 and off < 2048 else 2
            add("b4_snappy_copy_%d_at_%d" % (ln, off), "snappy", B.bytes(), [LZ_SANE, (
                "a copy of %d at offset %d: tag %d" % (ln, off, tag),
                lambda v, d=d, ln=ln, off=off, tag=tag: ("match", ln, off, tag) in v.streams[0].elements and
                _lz_match(d, ln, off)(v))])
    for n, pre in ((127, 1), (128, 2), (16383, 2), (16384, 3)):
        def pre_case(k, n=n):
            B = Buf(870 + k + n)
            s = B.fresh(40)
            B.fresh_to(64, before=s)
            d = B.plant(s, 40)
            if n > 1000:
                B.zeros_to(n - 20)
            B.fresh_to(n)
            return (B, d) if B.bucket_holds(s, d) else None
        B, d = _retry(pre_case)
        add("b4_snappy_preamble_%d" % n, "snappy", B.bytes(), [LZ_SANE, (
            "a stream of %d bytes: a length preamble of %d byte(s)" % (n, pre),
            lambda v, n=n, pre=pre, d=d: v.streams[0].preamble == (n, pre) and _lz_match(d, 40, 64)(v))])

    # ---- B5 framing
    rng = np.random.default_rng(880)
    vals = rng.integers(0, 256, 2 * 1024 + 250).astype("<u4")  # the low byte plane random, the others zero
    for fmt in LZ_FMTS:
        add("b5_%s_split_and_leftover" % fmt, fmt, vals.tobytes(), [LZ_SANE, (
            "two split blocks of 4 streams and an unsplit short last block; the random byte planes stored, the others "
            "compressed", lambda v: [s.block for s in v.frame.streams] == [0] * 4 + [1] * 4 + [2] and
            not v.frame.flags & 0x10 and [s.stored for s in v.frame.streams] == [True, False, False, False] * 2 + [False]
            and [s.size for s in v.frame.streams] == [1024] * 8 + [1000])], shuffle="shuffle", typesize=4, blocksize=4096)
        add("b5_%s_memcpyed" % fmt, fmt, rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(), [memcpyed])
    # ---- G5 through blosc: zlib streams of incompressible bytes never beat the bytes themselves, so
    # the frame is memcpyed (framing only: blosc's zlib streams are not held to zlib's bound)
    for n in (65535, 65536, 100000):
        add("g5_blosc_zlib_%d" % n, "zlib", rng.integers(0, 256, n, dtype=np.uint8).tobytes(), [memcpyed])
    return out


def zlib_bounded_cases():
    """G5: incompressible bytes through numcodecs.zlib, whose streams k_gzip_encode holds to zlib's
    compressBound (zlib_bounded). These inputs do NOT run the rewrite into 65,535-byte stored blocks: a
    block is cut after 16,321 to 16,384 symbols, pure literals make it 16,384 bytes, and 5 bytes a stored
    block of 16,384 is the bound's own slope, so the first pass stays within it and its 16 KiB stored
    blocks meet the intent. Only blocks shorter than 16,384 bytes (one cut right behind a match that
    ran into its step) exceed the slope, by a byte per MiB or so: it takes incompressible input of more
    than 6 MiB with such a match in nearly every block to pass the bound, beyond the sizes of this
    suite. The rewrite stays untested."""
    rng = np.random.default_rng(890)
    out = []
    for n in (65535, 65536, 100000):
        bound = n + (n >> 12) + (n >> 14) + (n >> 25) + 13
        out.append(Case("g5_zlib_incompressible_%d" % n, "zlib", rng.integers(0, 256, n, dtype=np.uint8).tobytes(), [SANE, (
            "stored blocks of at most 65535 bytes (and at most one empty fixed block), within zlib's bound of %d" % bound,
            lambda v: all(b.btype == 0 and b.size <= 65535 or (b.btype == 1 and b.size == 0) for b in v.blocks))]))
    return out


# The names of all_cases(), in order, written out: a test module parametrises over them without building
# the inputs at collection (all_cases() checks the list; tests/test_encoded_inspect_model.py runs it).
NAMES = tuple("""
    g1_dist_32768 g1_dist_32768_zlib g1_dist_32769 g1_dist_1 g1_src_65534 g1_src_65535 g1_src_65536
    g1_wrap_page1 g1_wrap_page2 g1_copy_straddles_65536 g2_lengths g2_lengths_zlib g3_flat_16320 g3_flat_16384
    g3_flat_16448 g3_skewed_16320 g3_skewed_16384 g3_skewed_16448 g3_match_across_cut g3_mixed_blocks
    g4_two_symbols g4_one_distance_code g4_all_codes g4_fibonacci_distances g4_runs_a g4_runs_b
    g5_zlib_incompressible_65535 g5_zlib_incompressible_65536 g5_zlib_incompressible_100000 z1_n255 z1_n256
    z1_n256_ck z1_n65791 z1_n65792 z1_n65792_ck z1_n65535 z1_n65536 z1_n65537 z1_n65537_ck z1_n131072 z1_n131073
    z2_raw_31 z2_raw_32 z2_raw_32_ck z2_raw_4095 z2_raw_4096 z2_rle_literals z2_huf_1023 z2_huf_1024
    z2_huf_1024_ck z2_huf_1025 z2_huf_1026 z2_huf_1027 z2_huf_16383 z2_huf_16384 z3_two_symbols_0_1
    z3_two_symbols_254_255 z3_two_symbols_0_255 z3_direct_weights z3_direct_weights_ck z3_fse_weights
    z3_fse_weights_ck z3_flat_200 z3_fibonacci_24 z3_fibonacci_24_ck z4_nseq_127 z4_nseq_128 z4_offsets_1_to_4
    z4_offsets_1_to_4_ck z4_offset_code_edges z4_adjacent_matches z4_ll_ml_code_edges z4_ll_ml_code_edges_ck
    z4_zero_blocks z4_copy_across_block_end z5_segments_warm_in z5_segments_warm_in_ck
    z5_blosc_zstd_unequal_streams z5_segments_warm_out b1_lz4_1bytes b1_lz4_2bytes b1_lz4_3bytes b1_lz4_4bytes
    b1_lz4_5bytes b1_lz4_6bytes b1_lz4_7bytes b1_lz4_8bytes b1_lz4_9bytes b1_lz4_10bytes b1_lz4_11bytes
    b1_lz4_12bytes b1_lz4_13bytes b1_lz4_16bytes b1_lz4_17bytes b1_lz4_copy_in_last_12 b1_lz4_copy_into_last_5
    b1_lz4_runs_and_matches b1_blosclz_1bytes b1_blosclz_2bytes b1_blosclz_3bytes b1_blosclz_4bytes
    b1_blosclz_5bytes b1_blosclz_6bytes b1_blosclz_7bytes b1_blosclz_8bytes b1_blosclz_9bytes b1_blosclz_10bytes
    b1_blosclz_11bytes b1_blosclz_12bytes b1_blosclz_13bytes b1_blosclz_16bytes b1_blosclz_17bytes
    b1_blosclz_copy_in_last_12 b1_blosclz_copy_into_last_5 b1_blosclz_runs_and_matches b1_snappy_1bytes
    b1_snappy_2bytes b1_snappy_3bytes b1_snappy_4bytes b1_snappy_5bytes b1_snappy_6bytes b1_snappy_7bytes
    b1_snappy_8bytes b1_snappy_9bytes b1_snappy_10bytes b1_snappy_11bytes b1_snappy_12bytes b1_snappy_13bytes
    b1_snappy_16bytes b1_snappy_17bytes b1_snappy_copy_in_last_12 b1_snappy_copy_into_last_5
    b1_snappy_runs_and_matches b1_lz4hc_copy_in_last_12 b1_lz4hc_copy_into_last_5 b1_lz4hc_runs_and_matches
    b2_lz4_offset_65535 b2_lz4_offset_65536 b2_lz4hc_offset_65535 b2_lz4hc_offset_65536 b4_snappy_offset_65536
    b3_blosclz_lengths b3_blosclz_distance_8191 b3_blosclz_distance_8192 b3_blosclz_distance_8193
    b3_blosclz_distance_73727 b3_blosclz_distance_73728 b4_snappy_literals_and_copies b4_snappy_copy_11_at_2047
    b4_snappy_copy_11_at_2048 b4_snappy_copy_12_at_2047 b4_snappy_copy_12_at_2048 b4_snappy_preamble_127
    b4_snappy_preamble_128 b4_snappy_preamble_16383 b4_snappy_preamble_16384 b5_lz4_split_and_leftover
    b5_lz4_memcpyed b5_blosclz_split_and_leftover b5_blosclz_memcpyed b5_snappy_split_and_leftover
    b5_snappy_memcpyed g5_blosc_zlib_65535 g5_blosc_zlib_65536 g5_blosc_zlib_100000
""".split())


def all_cases():
    out = gzip_cases() + zlib_bounded_cases() + zstd_cases() + blosc_cases()
    assert tuple(c.name for c in out) == NAMES, "NAMES is out of date"
    return out


def _dist_code(d):
    return max(i for i in range(30) if I.DIST_BASE[i] <= d)


def fib_distances_case():
    """G4: distances whose codes have Fibonacci frequencies, so that the optimal distance code is 16 bits
    deep and the encoder's sits at DEFLATE's 15-bit limit. The input is a sequence of 16-byte words, 24
    different ones; a word seen g words ago (g >= 4: an earlier step) is a 16-byte match at distance
    16 g. A greedy schedule picks, word by word, a reuse whose distance code still has quota (the rarest
    code first), else the most recent word that may be reused; a word whose last use sits right behind the
    previous word's is never taken, so no two matches merge."""
    import collections
    import zstd_huf_model as M
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    codes = list(range(11, 28))  # distances 49..64 up to 12289..16384
    quota = dict(zip(codes, sorted(fib, reverse=True)))
    rng = np.random.default_rng(900)
    last, seq, t = {}, [], 0  # word -> time of its last use; (word, the last use's time or None)
    while sum(quota.values()):
        free = [(w, lt) for w, lt in last.items() if t - lt >= 4 and 16 * (t - lt) <= 32768 and
                not (seq and seq[-1][1] is not None and seq[-1][1] == lt - 1)]
        want = [(-_dist_code(16 * (t - lt)), rng.random(), w, lt) for w, lt in free if quota.get(_dist_code(16 * (t - lt)), 0)]
        if want:
            _, _, w, lt = min(want)
            quota[_dist_code(16 * (t - lt))] -= 1
        elif len(last) >= 24 and free:
            w, lt = max(free, key=lambda x: x[1])
        else:
            w, lt = len(last), None
        seq.append((w, lt))
        last[w] = t
        t += 1
    plan = collections.Counter(_dist_code(16 * (i - lt)) for i, (w, lt) in enumerate(seq) if lt is not None)
    f = [plan.get(c, 0) for c in range(30)]
    assert max(M.huff_lengths(f, 40)) > 15 and len(plan) == 17
    # the words' bytes: a first byte of its own, 12 random ones and a common 3-byte ending, so that the
    # 4-byte strings of the data are the 16 of each word whatever word follows which; a word is redrawn
    # until its 16 strings hash to buckets no other string uses: every lookup finds the last use
    end = bytes([251, 252, 253])
    words, used = {}, set()
    for w in range(len(last)):
        while True:
            cand = bytes([10 + w]) + rng.integers(1, 250, 12, dtype=np.uint8).tobytes() + end
            hs = {hash4(gram(end + cand, i)) for i in range(16)}
            if len(hs) == 16 and not hs & used:
                break
        used |= hs
        words[w] = cand
    data = end + b"".join(words[w] for w, lt in seq)
    def histogram(v):
        return collections.Counter(_dist_code(m[2]) for m in v.matches)
    return Case("g4_fibonacci_distances", "gzip", data, [
        SANE, ("one dynamic block whose matches are the %d planned ones, Fibonacci over 17 distance codes: a word "
               "(16 bytes), or behind a new word that word's ending too (19)" % sum(plan.values()),
               lambda v: len(v.blocks) == 1 and v.blocks[0].btype == 2 and histogram(v) == plan and
               all(m[1] in (16, 19) for m in v.matches)),
        ("the distance code lengths reach the 15-bit limit", lambda v: max(v.blocks[0].dd) == 15)])
