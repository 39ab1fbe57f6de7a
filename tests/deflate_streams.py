"""Hand-assembled DEFLATE streams for k_gzip (kernels/inflate.hip): what RFC 1951 allows and zlib's
encoder never emits, at the edges the decoder has code of its own for. Test infrastructure, no GPU.

  * BitWriter and a token-level assembler: stored blocks (chosen padding bits and LEN/NLEN), fixed
    blocks, dynamic blocks with caller-chosen literal/length and distance code lengths, a chosen
    code-length alphabet and a chosen encoding of the header (which runs use 16/17/18, HCLEN, raw
    HLIT/HDIST fields). Tokens: an int (a literal), ("m", len, dist[, length code]) (a match, the
    length code forced when given: 284 + extra 31 for 258), ("raw", code) (a literal/length code
    emitted as it is), ("mraw", len, bits, nbits) (a length followed by raw distance bits).
  * Wrappers: a gzip member (CRC-32, ISIZE), an RFC 1950 zlib stream (Adler-32), each with or without
    a trailing crc32c of the stream.
  * execute(): the byte-at-a-time LZ77 reference over the token lists, the `expect` of valid cases.
  * Case: name, the stream, `expect` or `status`, and `intent`: (what the case is for, a predicate over
    the CPU model's trace of the stream - tools/gzip_seg_model.py with the kernel's constants) pairs.
    A control next to an edge states that the model does NOT reach the state. FAMILIES groups them.

Every valid case is padded by a final stored block to one of the decoded sizes of SIZES, so that a
family decodes in a few calls.

The executor_ring cases were built to reach the executor's ring edge (a batch with RING - 30 or more
unflushed bytes), where the kernel decoded wrong bytes while BATCH_CAP was RING / 2. The kernel's
constants now exclude that state, so those cases carry two intents: `intent_ring_half` (the state,
under the model run with BATCH_CAP = RING / 2) and `intent` = SAFE (no stream reaches it under the
kernel's constants).
"""
from __future__ import annotations

import os
import struct
import sys
import zlib
from dataclasses import dataclass, field

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gzip_seg_model as M  # noqa: E402

OK, CORRUPT, SIZE = "OK", "CORRUPT_STREAM", "DECODED_SIZE_MISMATCH"
# decoded sizes: the distance-32768 and 48-bit-symbol cases need 40960, the 65535-byte stored block 65536
SIZES = (4096, 16384, 40960, 65536)


# ---- bits ---------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.v = 0
        self.n = 0

    def bits(self, val, k):  # LSB first (header fields, extra bits)
        assert 0 <= val < (1 << k) or k == 0
        self.v |= val << self.n
        self.n += k

    def code(self, c, k):  # a Huffman code, MSB first
        self.bits(int(format(c, "0%db" % k)[::-1], 2) if k else 0, k)

    def align(self, pad=0):
        k = -self.n % 8
        self.bits(pad & ((1 << k) - 1), k)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canon(lens):
    """{symbol: (code, length)} of the canonical code (RFC 1951 3.2.2); the lengths may be incomplete
    or over-subscribed (corrupt cases): the codes are then just what the recurrence gives."""
    mx = max(lens) if lens else 0
    cnt = [0] * (mx + 2)
    for ln in lens:
        if ln:
            cnt[ln] += 1
    code, nxt = 0, [0] * (mx + 2)
    for b in range(1, mx + 1):
        code = (code + cnt[b - 1]) << 1 if b > 1 else 0
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lens):
        if ln:
            out[s] = (nxt[ln] & ((1 << ln) - 1), ln)
            nxt[ln] += 1
    return out


def complete_lens(n):
    """n code lengths of a complete code, as flat as possible (shorter ones first)."""
    if n == 1:
        return [1]
    k = n.bit_length() - 1
    if n == 1 << k:
        return [k] * n
    short = (1 << (k + 1)) - n
    return [k] * short + [k + 1] * (n - short)


def spread(n_alphabet, symbols, lens):
    """A length list of n_alphabet entries giving symbols[i] the length lens[i]."""
    out = [0] * n_alphabet
    for s, ln in zip(symbols, lens):
        out[s] = ln
    return out


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def len_code(n, forced=None):
    if forced is not None:
        i = forced - 257
    elif n == 258:
        i = 28
    else:
        i = max(k for k in range(28) if M.LEN_BASE[k] <= n)
    x = n - M.LEN_BASE[i]
    assert 0 <= x < (1 << M.LEN_EXTRA[i]) or (x == 0 and M.LEN_EXTRA[i] == 0), (n, forced)
    return 257 + i, x, M.LEN_EXTRA[i]


def dist_code(d):
    i = max(k for k in range(30) if M.DIST_BASE[k] <= d)
    return i, d - M.DIST_BASE[i], M.DIST_EXTRA[i]


def used_symbols(tokens):
    ll, dd = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            ll.add(t)
        elif t[0] == "m":
            ll.add(len_code(t[1], t[3] if len(t) > 3 else None)[0])
            dd.add(dist_code(t[2])[0])
    return sorted(ll), sorted(dd)


def flat_lens(tokens):
    """(literal/length lengths, distance lengths): a flat complete code over the symbols the tokens use
    (two distance codes at least, as zlib emits)."""
    ll, dd = used_symbols(tokens)
    if len(ll) == 1:
        ll = sorted(set(ll) | {0})
    while len(dd) < 2:
        dd = sorted(set(dd) | {min(set(range(30)) - set(dd))})
    return spread(max(ll) + 1, ll, complete_lens(len(ll))), spread(max(dd) + 1, dd, complete_lens(len(dd)))


# ---- blocks -------------------------------------------------------------------------------------
@dataclass
class Stored:
    data: bytes
    pad: int = 0           # the padding bits before LEN
    len_field: int | None = None
    nlen_field: int | None = None
    present: int | None = None  # bytes of data actually emitted (a block running past the input)
    btype: int = 0


@dataclass
class Fixed:
    tokens: list
    eob: bool = True


@dataclass
class Dynamic:
    tokens: list
    ll: list | None = None     # literal/length code lengths (HLIT = their number); default flat_lens
    dd: list | None = None     # distance code lengths (HDIST = their number)
    cl: list | None = None     # the 19 code-length code lengths; default: flat over the symbols used
    ops: list | None = None    # the header's symbols: (0..15,), (16, rep), (17, rep), (18, rep); default plain
    rle: bool = False          # default ops: greedy runs over the concatenated lengths instead of plain
    hclen: int | None = None
    hlit_field: int | None = None
    hdist_field: int | None = None
    eob: bool = True


def plain_ops(seq):
    return [(v,) for v in seq]


def rle_ops(seq):
    """Greedy runs over the whole sequence (so a 16 may carry across the literal/distance boundary)."""
    ops, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            r = min(run, 138)
            ops.append((18, r) if r >= 11 else (17, r))
            i += r
        elif ops and run >= 3 and i > 0 and seq[i - 1] == v:
            r = min(run, 6)
            ops.append((16, r))
            i += r
        else:
            ops.append((v,))
            i += 1
    return ops


def auto_cl(ops):
    used = sorted({o[0] for o in ops})
    if len(used) == 1:
        used = sorted(set(used) | ({0} if used[0] else {1}))
    freq = {s: sum(o[0] == s for o in ops) for s in used}
    order = sorted(used, key=lambda s: -freq[s])
    return spread(19, order, complete_lens(len(order)))


def _emit_tokens(w, tokens, ll, dd, eob):
    lc, dc = canon(ll), canon(dd)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lc[t])
        elif t[0] == "m":
            s, x, xb = len_code(t[1], t[3] if len(t) > 3 else None)
            w.code(*lc[s])
            w.bits(x, xb)
            d, y, yb = dist_code(t[2])
            w.code(*dc[d])
            w.bits(y, yb)
        elif t[0] == "raw":
            w.code(*lc[t[1]])
        elif t[0] == "mraw":
            s, x, xb = len_code(t[1])
            w.code(*lc[s])
            w.bits(x, xb)
            w.bits(t[2], t[3])
        else:
            raise ValueError(t)
    if eob:
        w.code(*lc[256])


def deflate(blocks, final_last=True):
    """The raw DEFLATE stream of the blocks (the last one final) and the bit offset of each block's
    first symbol (stored blocks: of their first data byte)."""
    w, starts = BitWriter(), []
    for i, b in enumerate(blocks):
        w.bits(1 if (final_last and i == len(blocks) - 1) else 0, 1)
        if isinstance(b, Stored):
            w.bits(b.btype, 2)
            if b.btype == 3:
                continue
            w.align(b.pad)
            n = len(b.data) if b.len_field is None else b.len_field
            w.bits(n, 16)
            w.bits((n ^ 0xFFFF) if b.nlen_field is None else b.nlen_field, 16)
            starts.append(w.n)
            for x in b.data[:len(b.data) if b.present is None else b.present]:
                w.bits(x, 8)
        elif isinstance(b, Fixed):
            w.bits(1, 2)
            starts.append(w.n)
            _emit_tokens(w, b.tokens, FIXED_LL, FIXED_D, b.eob)
        else:
            w.bits(2, 2)
            ll, dd = b.ll, b.dd
            if ll is None or dd is None:
                fl, fd = flat_lens(b.tokens)
                ll, dd = ll if ll is not None else fl, dd if dd is not None else fd
            seq = list(ll) + list(dd)
            ops = b.ops if b.ops is not None else (rle_ops(seq) if b.rle else plain_ops(seq))
            cl = b.cl if b.cl is not None else auto_cl(ops)
            hclen = b.hclen if b.hclen is not None else max(4, 1 + max(i for i, s in enumerate(M.CLEN_ORDER) if cl[s]))
            w.bits(len(ll) - 257 if b.hlit_field is None else b.hlit_field, 5)
            w.bits(len(dd) - 1 if b.hdist_field is None else b.hdist_field, 5)
            w.bits(hclen - 4, 4)
            for i in range(hclen):
                w.bits(cl[M.CLEN_ORDER[i]], 3)
            cc = canon(cl)
            for o in ops:
                w.code(*cc[o[0]])
                if o[0] == 16:
                    w.bits(o[1] - 3, 2)
                elif o[0] == 17:
                    w.bits(o[1] - 3, 3)
                elif o[0] == 18:
                    w.bits(o[1] - 11, 7)
            starts.append(w.n)
            _emit_tokens(w, b.tokens, ll, dd, b.eob)
    return w.bytes(), starts


def execute(blocks):
    """The decoded bytes of the blocks' tokens: a byte-at-a-time LZ77 copy."""
    out = bytearray()
    for b in blocks:
        if isinstance(b, Stored):
            out += b.data
            continue
        for t in b.tokens:
            if isinstance(t, int):
                out.append(t)
            else:
                assert t[0] == "m" and 1 <= t[2] <= len(out), t
                for _ in range(t[1]):
                    out.append(out[-t[2]])
    return bytes(out)


def gzip_wrap(raw, data):
    return (b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF))


def zlib_wrap(raw, data):
    return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(data) & 0xFFFFFFFF)


def with_crc32c(enc):
    import oracle
    return enc + struct.pack("<I", oracle.crc32c(enc))


# ---- cases --------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    raw: bytes                 # the DEFLATE stream
    size: int                  # the chunk size it is decoded as (one of SIZES)
    expect: bytes | None = None   # status OK: the decoded bytes (len == size)
    status: str = OK
    decoded: bytes = b""       # what the stream decodes to (the trailer's checksums; a size case's bytes)
    intent: list = field(default_factory=list)  # [(text, predicate over the model's stats)]
    # the same over a model run with BATCH_CAP = RING / 2, the value under which the executor's ring
    # edge was reachable (the state these cases were built to reach and the kernel's constants now exclude)
    intent_ring_half: list = field(default_factory=list)
    ring: bool = False         # an executor-ring case (also run as a lone item)

    def enc(self, kind):
        """kind: gz, gz_crc, zlib, zlib_crc."""
        d = self.expect if self.expect is not None else self.decoded
        e = gzip_wrap(self.raw, d) if kind.startswith("gz") else zlib_wrap(self.raw, d)
        return with_crc32c(e) if kind.endswith("_crc") else e


def _rng(seed):
    return np.random.default_rng(seed)


def _rand(seed, n, lo=0, hi=256):
    return _rng(seed).integers(lo, hi, n, dtype=np.uint8).tobytes()


def valid(name, blocks, size=None, intent=(), ring=False):
    """A valid case: the blocks, then a final stored block of random bytes up to the decoded size."""
    data = execute(blocks)
    size = size or next(s for s in SIZES if s > len(data))
    assert len(data) < size, (name, len(data))
    pad = _rand(len(name) + len(data), size - len(data))
    blocks = list(blocks) + [Stored(pad, pad=0x55)]
    raw, _ = deflate(blocks)
    return Case(name, raw, size, expect=data + pad, intent=list(intent), ring=ring)


def corrupt(name, blocks, size=4096, cut=None):
    """A corrupt case: the blocks as they are (the last one final), cut to `cut` bytes when given."""
    raw, _ = deflate(blocks)
    if cut is not None:
        raw = raw[:cut]
    return Case(name, raw, size, status=CORRUPT)


def from_raw(name, raw, data, size):
    """A case around a finished raw DEFLATE stream (zlib's): padded by appending to the data first."""
    assert len(data) == size
    return Case(name, raw, size, expect=data)


# ---- model predicates -----------------------------------------------------------------------------
def short_unflushed(st):
    """A match of at most 32 bytes whose source starts older than the ring (the kernel's per-match
    test sends it to the flushed output) and whose last source byte is not flushed yet."""
    return any(m["len"] <= 32 and not m["start_in_ring"] and not m["last_flushed"]
               for b in st["batches"] for m in b["matches"])


def long_unflushed(st):
    return any(m["len"] > 32 and not m["start_in_ring"] and not m["last_flushed"]
               for b in st["batches"] for m in b["matches"])


def long_straddle(st):
    """A match longer than 32 whose source starts older than the ring and ends inside it."""
    return any(m["len"] > 32 and not m["start_in_ring"] and m["last"] + M.RING >= b["pos"] + b["B"]
               for b in st["batches"] for m in b["matches"])


def old_source(st):
    return any(not m["start_in_ring"] and m["last"] + M.RING < b["pos"] + b["B"]
               for b in st["batches"] for m in b["matches"])


def flush_head_stale(st):
    """A batch ending in a flush whose first 16-B piece (from `flushed` rounded down) reaches back to
    bytes whose ring slots the batch has overwritten."""
    return any(b["flushed"] % 16 and b["B"] + b["f"] >= M.FLUSH_MIN
               and (b["flushed"] & ~15) + M.RING < b["pos"] + b["B"] for b in st["batches"])


def max_bf(st):
    return max((b["B"] + b["f"] for b in st["batches"]), default=0)


def no(pred):
    return lambda st: not pred(st)


# what the kernel's constants guarantee for every stream (the static_assert beside BATCH_CAP)
SAFE = [("B + f stays below RING - 30", lambda st: max_bf(st) <= M.RING - 31),
        ("no short match's source starts older than the ring and ends unflushed", no(short_unflushed)),
        ("no flush's first piece starts at overwritten ring bytes", no(flush_head_stale))]


# ---- family: executor_ring --------------------------------------------------------------------------
def _ring_blocks(slen, dist, total, prefix):
    """The issue's construction: `prefix` (P bytes, everything flushed at its end), then a fixed block:
    63 literals and a match (192, 1500) - a batch of 64 symbols and 255 bytes, left pending - then
    the matches (258, 300), (b, 300), (slen, dist), (258, 300) in one batch of B = total - 255 bytes."""
    b = total - 255 - 258 - 258 - slen
    assert 3 <= b <= 258 and 258 + b + slen < 512, (slen, total, b)
    lits = list(_rand(slen * 1000 + dist, 63))
    return prefix + [Fixed(lits + [("m", 192, 1500), ("m", 258, 300), ("m", b, 300), ("m", slen, dist),
                                   ("m", 258, 300), 7, 8, 9])]


def _ring_hits(slen, dist, total, P):
    b = total - 255 - 258 - 258 - slen
    q = P + 255 + 258 + b          # where the short match writes
    end = P + total                # the batch's end; flushed = P
    src = q - dist
    return src + 1024 < end and src + min(slen, dist) - 1 >= P


def _stored_prefix(seed, n=2000):
    return [Stored(_rand(seed, n))]


def _dynamic_prefix(seed, n=2048):
    """n literals through a flat dynamic code: 32 batches of 64 bytes, the last one flushed."""
    return [Dynamic(list(_rand(seed, n)))]


def family_executor_ring():
    cases = []

    def add(name, slen, dist, total, prefix, P, extra=()):
        hit = _ring_hits(slen, dist, total, P)
        if slen > 32:
            intent = [("wave-copy control: no short match in the state", no(short_unflushed)),
                      ("a long match: source start older than the ring, source end not flushed", long_unflushed)]
        elif hit:
            intent = [("short match, source start older than the ring, source end at or past flushed", short_unflushed),
                      ("B + f == %d" % total, lambda st, t=total: max_bf(st) == t)]
        else:
            intent = [("control: no short match in the state", no(short_unflushed)),
                      ("B + f == %d" % total, lambda st, t=total: max_bf(st) == t)]
        c = valid(name, _ring_blocks(slen, dist, total, prefix), 4096, list(SAFE), ring=hit or slen > 32 or bool(extra))
        c.intent_ring_half = intent + list(extra)
        cases.append(c)

    P = 2000
    for D in range(735, 776):  # B + f = 1021, a 20-byte match: D 747..762 reach the state
        add(f"ring_D{D}", 20, D, 1021, _stored_prefix(D), P)
    for slen in (3, 8, 9, 20, 32, 33):
        for total in (993, 994, 1021, 1024):
            if total - 255 - 516 - slen > 258 or 258 + (total - 255 - 516 - slen) + slen >= 512:
                continue
            b = total - 255 - 516 - slen
            q = P + 513 + b
            # the source end at flushed - 1, flushed and flushed + 1 (flushed = P)
            for k in (-1, 0, 1):
                D = q - (P + k - (slen - 1))
                add(f"ring_L{slen}_T{total}_end{k:+d}", slen, D, total, _stored_prefix(slen * 7 + total + k), P)
    for D in (745, 747, 750, 762, 763):  # the same after a dynamic block of 2048 literals
        add(f"ring_dyn_D{D}", 20, D + 0, 1021, _dynamic_prefix(D), 2048)
    # A flush whose first 16-B piece starts at bytes flushed earlier (`flushed` = P is not a multiple of
    # 16) after the ring has wrapped over them: B + f > 1024 - (P mod 16). Controls one byte below.
    for P, total in ((2001, 1024), (2008, 1024), (2015, 1024), (2015, 1010), (2015, 1009), (2001, 1021)):
        stale = total > 1024 - P % 16
        add(f"ring_P{P}_T{total}", 20, 735, total, _stored_prefix(P + total, P), P,
            [("the flush's first 16-B piece starts at ring bytes already overwritten", flush_head_stale) if stale else
             ("control: the flush's first piece is intact in the ring", no(flush_head_stale))])
    # long matches whose source straddles the ring's edge, or lies wholly before it
    for D in range(1020, 1031):
        blocks = _stored_prefix(D, 2000) + [Fixed(list(_rand(D, 63)) + [("m", 258, D), 1, 2, 3])]
        cases.append(valid(f"ring_long_D{D}", blocks, 4096,
                           [("a long match's source straddles the ring edge", long_straddle) if D <= 1023 else
                            ("a long match's source lies before the ring", old_source)]))
    blocks = [Stored(_rand(5, 33000)), Fixed(list(_rand(6, 63)) + [("m", 258, 32768), ("m", 20, 32768), 1, 2, 3])]
    cases.append(valid("ring_long_D32768", blocks, 40960, [("sources 32768 back, before the ring", old_source)]))
    return cases


# ---- family: executor_deps --------------------------------------------------------------------------
def _deep_batch(st):
    """A batch of 64 matches, each one's source inside the previous one's output."""
    for b in st["batches"]:
        m = b["matches"]
        if b["syms"] == 64 and len(m) == 64 and all(0 < m[i]["dist"] <= m[i - 1]["len"] for i in range(1, 64)):
            return True
    return False


def family_executor_deps():
    cases = []
    lits = list(_rand(11, 64))
    cases.append(valid("deps_chain63", [Fixed(lits + [("m", 3, 3)] * 64 + [5])], 4096,
                       [("64 matches in one batch, each copying the one before: depth 63", _deep_batch)]))
    cases.append(valid("deps_chain63_mixed", [Fixed(lits + [("m", 3 + i % 5, 1 + i % 3) for i in range(64)] + [5])],
                       4096, [("64 matches in one batch, each copying the one before", _deep_batch)]))
    for lo in (1, 4, 7):  # distances 1..9 x lengths 3..40, three distances a case
        toks = list(_rand(lo, 16))
        for d in range(lo, lo + 3):
            for ln in range(3, 41):
                toks += [("m", ln, d), (ln * 7 + d) & 255]
        cases.append(valid(f"deps_d{lo}to{lo + 2}_len3to40", [Fixed(toks)], 4096))
    toks = list(_rand(3, 300))
    for d in (1, 2, 3, 5, 7, 255, 256, 257, 258):
        toks += [("m", 258, d), d & 255, 77]
    cases.append(valid("deps_len258", [Fixed(toks)], 4096))
    cases.append(valid("deps_dist_eq_pos", [Fixed(list(range(10)) + [("m", 5, 10), ("m", 30, 15), 9])], 4096))
    bad = Fixed(list(range(10)) + [("m", 5, 11), 9])
    cases.append(corrupt("deps_dist_pos_plus1", [bad]))
    cases.append(corrupt("deps_match_first", [Fixed([("m", 3, 1), 9])]))
    bad = [Stored(_rand(1, 700)), Fixed([1, 2, 3, ("m", 40, 704), 9])]
    cases.append(corrupt("deps_long_dist_pos_plus1", bad))
    return cases


# ---- family: codes ----------------------------------------------------------------------------------
SKEW16 = list(range(1, 16)) + [15]


def _tables(key, pred):
    return lambda st: any(pred(t[key]) for t in st["tables"])


def _lsub_lens():
    """A complete literal/length set of 283 symbols whose second-level tables total 324 entries under a
    9-bit root (zlib's bound for 286 symbols is 340, which LSUB covers): 3 bits for the end-of-block
    code and the lengths 3..8, 4/5/6/9 bits for the literals 0..3, 10..14 bits for 4..17 and 15 bits
    for the 258 others."""
    counts = {3: 7, 4: 1, 5: 1, 6: 1, 9: 1, 10: 4, 11: 1, 12: 3, 13: 5, 14: 1, 15: 258}
    syms = [256] + list(range(257, 263)) + list(range(256)) + list(range(263, 283))
    return spread(283, syms, [ln for ln in sorted(counts) for _ in range(counts[ln])])


def _dsub_lens(tail):
    """Distance lengths 1..8 for codes 0..7, then `tail` under the last root prefix."""
    return list(range(1, 9)) + tail


def family_codes():
    cases = []
    # 15-bit literal/length codes: the skewed set 1, 2, .., 14, 15, 15
    syms = list(range(65, 78)) + [256, 257, 258]  # 13 literals, EOB (14 bits), lengths 3 and 4 (15 bits)
    ll = spread(259, syms, SKEW16)
    r = _rng(21)
    toks = [65 + int(x) for x in r.integers(0, 13, 40)]
    for i in range(300):
        toks += [65 + int(x) for x in r.integers(0, 13, 3)] + [("m", 3 + i % 2, 1 + int(r.integers(0, 32)))]
    dd = spread(10, range(10), complete_lens(10))
    cases.append(valid("codes_skew15", [Dynamic(toks, ll=ll, dd=dd)], 4096,
                       [("literal/length codes reach 15 bits", _tables("lmax", lambda v: v == 15))]))
    # subtables of several hundred entries (a valid set cannot outgrow LSUB)
    ll = _lsub_lens()
    r = _rng(5)
    body = list(range(256))
    for i in range(400):
        body += [int(r.integers(0, 256)), int(r.integers(0, 256)), ("m", 3 + i % 6, 1 + i % 90)]
    dd = spread(14, range(14), complete_lens(14))
    cases.append(valid("codes_lsub324", [Dynamic(body, ll=ll, dd=dd)], 4096,
                       [("literal/length subtables total 324", _tables("lsub", lambda v: v == 324))]))
    # distance sets with 9..15-bit codes: subtables of 16, exactly 32 (DSUB) and more (lane_canon)
    for tail, total, name in (([9, 10, 11, 12, 12], 16, "codes_dsub16"), ([9, 10, 11, 12, 13, 13], 32, "codes_dsub32"),
                              ([9, 10, 11, 12, 13, 14, 14], 64, "codes_dsub64_slow"),
                              ([9, 10, 11, 12, 13, 14, 15, 15], 128, "codes_dsub128_slow")):
        dd = _dsub_lens(tail)
        r = _rng(total)
        body = list(_rand(total, 600))
        for i in range(260):
            c = i % len(dd)
            d = M.DIST_BASE[c] + int(r.integers(0, 1 << M.DIST_EXTRA[c]))
            body += [("m", 3 + i % 9, d), int(r.integers(0, 256))]
        ll, _ = flat_lens(body)
        cases.append(valid(name, [Dynamic(body, ll=ll, dd=dd)], 4096,
                           [("distance subtables total %d" % total, _tables("dsub", lambda v, t=total: v == t)),
                            ("distance codes reach %d bits" % max(tail), _tables("dmax", lambda v, t=max(tail): v == t))]))
    # the distance alphabet's edges
    lits = list(_rand(31, 50))
    ll, _ = flat_lens(lits + [("m", 10, 1), ("m", 4, 1)])
    cases.append(valid("codes_one_dist_code", [Dynamic(lits + [("m", 10, 1), lits[3], ("m", 4, 1), lits[5]], ll=ll, dd=[1])], 4096,
                       [("a single 1-bit distance code", _tables("dmax", lambda v: v == 1))]))
    cases.append(corrupt("codes_one_dist_code_unused", [Dynamic(lits + [("mraw", 10, 1, 1), lits[3]], ll=ll, dd=[1])]))
    cases.append(valid("codes_no_dist_code", [Dynamic(lits + lits[:5], ll=ll, dd=[0])], 4096,
                       [("HDIST 1 with length 0", _tables("dmax", lambda v: v == 0))]))
    cases.append(corrupt("codes_no_dist_code_length", [Dynamic(lits + [("mraw", 10, 0, 1), lits[3]], ll=ll, dd=[0])]))
    # a 1-bit literal code: 512 symbols a lane region, every region stops at SEGCAP
    ll = spread(257, [65, 66, 256], [1, 2, 2])
    body = [66 if i % 97 == 0 else 65 for i in range(3000)]
    cases.append(valid("codes_one_bit_literal", [Dynamic(body, ll=ll, dd=[0])], 4096,
                       [("every round is one lane region stopped at SEGCAP",
                         lambda st: st["cap_hits"] >= 30 and st["valid_lanes"] == st["rounds"])]))
    # back-to-back 48-bit symbols: 15-bit length code + 5 extra, 15-bit distance code + 13 extra
    ll = spread(286, list(range(13)) + [256, 281, 282], SKEW16)
    dd = spread(30, list(range(14)) + [28, 29], SKEW16)
    r = _rng(48)
    body = [0, 1, 2]
    for i in range(40):
        c = 281 + i % 2
        body.append(("m", M.LEN_BASE[c - 257] + int(r.integers(0, 32)), M.DIST_BASE[28 + i % 2] + int(r.integers(0, 8192))))
    cases.append(valid("codes_48bit_symbols", [Stored(_rand(7, 32768)), Dynamic(body, ll=ll, dd=dd)], 40960,
                       [("15-bit codes in both alphabets", lambda st: any(t["lmax"] == 15 and t["dmax"] == 15
                                                                           for t in st["tables"]))]))
    # 258 as code 284 + extra 31 (zlib takes it)
    cases.append(valid("codes_284_extra31", [Fixed(list(_rand(9, 300)) + [("m", 258, 300, 284), 1, ("m", 258, 1, 284)])],
                       4096))
    # codes the alphabets do not have
    for c in (286, 287):
        cases.append(corrupt(f"codes_fixed_{c}", [Fixed(list(range(20)) + [("raw", c), 1])]))
    for d in (30, 31):
        cases.append(corrupt(f"codes_fixed_dist{d}", [Fixed(list(range(20)) + [("mraw", 5, int(format(d, "05b")[::-1], 2), 5), 1])]))
    return cases


# ---- family: headers --------------------------------------------------------------------------------
def _hdr(pred):
    return lambda st: any(pred(h) for h in st["hdr"])


def _first_len_index(h):
    """[(symbol, index of its first length)] of a header."""
    out, n = [], 0
    for s, _, rep in h["syms"]:
        out.append((s, n))
        n += rep
    return out


def _win16_after(kinds):
    """A later window starting with a 16 whose previous window ended with a symbol of `kinds`."""
    def pred(h):
        w = h["windows"]
        return any(w[i]["take"][0] == 16 and w[i - 1]["take"][-1] in kinds for i in range(1, len(w)))
    return pred


LITS255 = spread(257, list(range(255)) + [256], [8] * 256)  # literals 0..254 and EOB, 8 bits each


def family_headers():
    cases = []
    body = list(_rand(41, 200, 0, 255))
    # HCLEN 4 can only give the lengths 0: no end-of-block code. 5 (adds 8) is the least valid one.
    cl4 = spread(19, [16, 17, 18, 0], [2, 2, 2, 2])
    cases.append(corrupt("hdr_hclen4", [Dynamic([], ll=[0] * 257, dd=[0], cl=cl4, hclen=4, rle=True, eob=False)]))
    cl5 = spread(19, [16, 17, 18, 0, 8], [3, 3, 2, 2, 2])
    cases.append(valid("hdr_hclen5", [Dynamic(body, ll=LITS255, dd=[0], cl=cl5, rle=True)], 4096,
                       [("HCLEN 5", _hdr(lambda h: h["hclen"] == 5))]))
    toks = body + [("m", 20, 100), ("m", 3, 1)]
    cases.append(valid("hdr_hclen19", [Dynamic(toks, hclen=19, rle=True)], 4096,
                       [("HCLEN 19", _hdr(lambda h: h["hclen"] == 19))]))
    # 7-bit code-length codes
    fl, fd = flat_lens(toks)
    ops = rle_ops(fl + fd)
    used = sorted({o[0] for o in ops}, key=lambda s: -sum(o[0] == s for o in ops))
    extra = [s for s in (1, 2, 3, 4, 5, 6, 7, 10, 11, 12) if s not in used]
    order = (used + extra)[:8]
    cases.append(valid("hdr_clen7", [Dynamic(toks, ll=fl, dd=fd, ops=ops, cl=spread(19, order, [1, 2, 3, 4, 5, 6, 7, 7]))],
                       4096, [("code-length codes of 7 bits", _hdr(lambda h: h["clmax"] == 7))]))
    # 1-bit code-length symbols: 63 symbol starts in a window, 32 taken
    ll = spread(258, list(range(254)) + [254, 255, 256, 257], [8] * 254 + [9] * 4)
    cl = spread(19, [8, 9, 0], [1, 2, 2])
    cases.append(valid("hdr_one_bit_clen", [Dynamic(list(_rand(42, 300)), ll=ll, dd=[0], cl=cl)], 4096,
                       [("more than 32 symbols start in one 63-bit window",
                         _hdr(lambda h: any(w["starts"] > 32 and len(w["take"]) == 32 for w in h["windows"])))]))
    cases.append(corrupt("hdr_16_first", [Dynamic(body, ll=LITS255, dd=[0], ops=[(16, 3)] + plain_ops(LITS255[3:] + [0]),
                                                  cl=spread(19, [16, 8, 0], [2, 1, 2]))]))
    # a 16 carrying across the literal/distance boundary
    ll = spread(258, list(range(239)) + [256, 257], [8] * 240 + [4])
    toks16 = list(_rand(43, 100, 0, 239)) + [("m", 3, d) for d in (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65)]
    cases.append(valid("hdr_16_across_boundary", [Dynamic(toks16, ll=ll, dd=[4] * 16, rle=True)], 4096,
                       [("a 16 writes the first distance length",
                         _hdr(lambda h: any(s == 16 and n == h["hlit"] for s, n in _first_len_index(h))))]))
    # A 16 as the first symbol of a later window. The lengths: 128 zeros, then 7 bits for the literals
    # 128..254 and the end-of-block code; the code-length codes 0, 7, 16, 17 take 2 bits each, so the
    # header's encoding alone places the window boundaries (a window takes the symbols starting within
    # its first 63 bits).
    ll7 = [0] * 128 + [7] * 127 + [0, 7]
    cl4 = spread(19, [0, 7, 16, 17], [2, 2, 2, 2])
    lits7 = [128 + b % 127 for b in _rand(44, 300)]
    # after an explicit length: 17 runs for the zeros, one explicit 7, then (7, 16 x 6) pairs of 6 bits
    ops = [(17, 10)] * 12 + [(17, 8)] + [(7,)] + [(7,), (16, 6)] * 18 + [(0,), (7,), (0,)]
    assert _ops_lens(ops) == ll7 + [0]
    cases.append(valid("hdr_16_window_after_len", [Dynamic(lits7, ll=ll7, dd=[0], ops=ops, cl=cl4)], 4096,
                       [("a later window starts with a 16 after an explicit length", _hdr(_win16_after(set(range(16)))))]))
    # after a 17: two explicit zeros, then (17 x 3, 16 x 3) pairs of 9 bits: the 7th pair's 16 starts at bit 63
    ops = [(0,)] * 2 + [(17, 3), (16, 3)] * 21 + [(7,)] + [(7,), (16, 6)] * 18 + [(0,), (7,), (0,)]
    assert _ops_lens(ops) == ll7 + [0]
    cases.append(valid("hdr_16_window_after_run", [Dynamic(lits7, ll=ll7, dd=[0], ops=ops, cl=cl4)], 4096,
                       [("a later window starts with a 16 after a 17", _hdr(_win16_after({17, 18})))]))
    # an 18 of 138 that starts at bit 60 of a window (its 31st symbol) and ends past the window
    ll138 = [6] * 10 + [7] * 20 + [0] * 138 + [7] * 87 + [0, 7]
    ops = plain_ops(ll138[:30]) + [(18, 138)] + plain_ops(ll138[168:] + [0])
    used = [s for s in range(255) if ll138[s]]
    cases.append(valid("hdr_18_run138_out_of_window",
                       [Dynamic([used[b % len(used)] for b in _rand(45, 300)], ll=ll138, dd=[0], ops=ops,
                                cl=spread(19, [0, 6, 7, 18], [2, 2, 2, 2]))], 4096,
                       [("an 18 of 138 starts inside a window and ends past its 63 bits",
                         _hdr(lambda h: any(w["take"][-1] == 18 and w["last_end"] > 63 for w in h["windows"])
                              and any(s == 18 and rep == 138 for s, _, rep in h["syms"])))]))
    # corrupt headers
    cases.append(corrupt("hdr_run_past_end", [Dynamic(body, ll=LITS255, dd=[0],
                                                      ops=plain_ops(LITS255) + [(17, 4)], cl=spread(19, [8, 0, 17], [1, 2, 2]))]))
    cases.append(corrupt("hdr_hlit_287", [Dynamic(body, ll=LITS255, dd=[0], hlit_field=30)]))
    cases.append(corrupt("hdr_hlit_288", [Dynamic(body, ll=LITS255, dd=[0], hlit_field=31)]))
    cases.append(corrupt("hdr_hdist_31", [Dynamic(body, ll=LITS255, dd=[0], hdist_field=30)]))
    cases.append(corrupt("hdr_hdist_32", [Dynamic(body, ll=LITS255, dd=[0], hdist_field=31)]))
    cases.append(corrupt("hdr_no_eob", [Dynamic(body, ll=spread(257, range(256), [8] * 256), dd=[0], eob=False)]))
    over = spread(257, list(range(255)) + [255, 256], [8] * 255 + [8, 7])
    cases.append(corrupt("hdr_oversubscribed", [Dynamic(body, ll=over, dd=[0])]))
    inc = spread(257, list(range(200)) + [256], [8] * 201)
    cases.append(corrupt("hdr_incomplete_litlen", [Dynamic([b % 200 for b in body], ll=inc, dd=[0])]))
    cases.append(corrupt("hdr_incomplete_dist", [Dynamic(body, ll=LITS255, dd=[2, 2, 2])]))
    cases.append(corrupt("hdr_oversubscribed_dist", [Dynamic(body, ll=LITS255, dd=[1, 1, 1])]))
    cases.append(corrupt("hdr_incomplete_clen", [Dynamic(body, ll=LITS255, dd=[0], cl=spread(19, [8, 0], [1, 2]))]))
    cases.append(corrupt("hdr_oversubscribed_clen", [Dynamic(body, ll=LITS255, dd=[0], cl=spread(19, [8, 0, 1], [1, 1, 1]))]))
    return cases




def _ops_lens(ops):
    """The code lengths a header's symbols write."""
    out = []
    for o in ops:
        if o[0] < 16:
            out.append(o[0])
        elif o[0] == 16:
            out += [out[-1]] * o[1]
        else:
            out += [0] * o[1]
    return out


# ---- family: blocks ---------------------------------------------------------------------------------
def _eob_at(lane, off):
    """The end-of-block code of some block starts `off` bits into lane `lane`'s region (off < 0: that
    many bits before it, in the previous lane's region)."""
    if off >= 0:
        return lambda st: any(e["lane"] == lane and e["off"] == off for e in st["eob"])
    return lambda st: any(e["lane"] == lane - 1 and e["to_end"] == -off for e in st["eob"])


def _fixed_bits(nbits, seed):
    """Literals of a fixed block taking exactly nbits (8-bit ones below 144, 9-bit ones from 144)."""
    b = nbits % 8
    a = (nbits - 9 * b) // 8
    assert a >= 0 and 8 * a + 9 * b == nbits
    r = _rng(seed)
    toks = [int(x) for x in r.integers(0, 144, a)] + [int(x) for x in r.integers(144, 256, b)]
    return [toks[i] for i in r.permutation(len(toks))]


def family_blocks():
    cases = []
    # zlib's own streams flushed every 16..64 input bytes: many tiny blocks and empty stored blocks
    for mode, name in ((zlib.Z_SYNC_FLUSH, "sync"), (zlib.Z_FULL_FLUSH, "full")):
        for level in (1, 9):
            r = _rng(level)
            data = np.repeat(r.integers(0, 16, 1024, dtype=np.uint8), 4).tobytes()  # 4096, compressible
            co, raw, p = zlib.compressobj(level, zlib.DEFLATED, -15), b"", 0
            while p < len(data):
                n = int(r.integers(16, 65))
                raw += co.compress(data[p:p + n]) + co.flush(mode)
                p += n
            raw += co.flush()
            cases.append(from_raw(f"blocks_zlib_{name}_flush_l{level}", raw, data, 4096))
    # stored blocks: lengths 0 and 65535, each of the 8 bit alignments before one (garbage padding bits)
    cases.append(valid("blocks_stored_len0", [Stored(b""), Fixed([1, 2, 3]), Stored(b"", pad=0xFF), Stored(b"abc"),
                                               Stored(b"")], 4096))
    cases.append(valid("blocks_stored_len65535", [Stored(_rand(65, 65535))], 65536))
    blocks = []
    for j in range(8):  # 3 + 8a + 9j + 7 + 3 bits before the padding: (5 + j) mod 8
        blocks += [Fixed([10 + j] * 3 + [200 + j] * j), Stored(_rand(j, 37 + j), pad=0xAA >> (j & 1))]
    cases.append(valid("blocks_stored_8_alignments", blocks, 4096))
    cases.append(corrupt("blocks_stored_nlen_mismatch", [Fixed([1, 2]), Stored(b"abcdef", nlen_field=0x1234)]))
    cases.append(corrupt("blocks_stored_past_input", [Fixed([1, 2]), Stored(_rand(1, 1000), present=100)]))
    cases.append(corrupt("blocks_type3", [Fixed([1, 2]), Stored(b"", btype=3)]))
    # the end-of-block code on the bits s_own - 2 .. s_own + 5 of lane 3's region, and inside lane 3's overlap
    for off in list(range(-2, 6)) + [-200, -380]:
        toks = _fixed_bits(3 * 512 + off, 1000 + off)
        cases.append(valid(f"blocks_eob_lane3_{'m' if off < 0 else 'p'}{abs(off)}", [Fixed(toks), Fixed([4, 5, 6])], 4096,
                           [("the end-of-block code starts at bit s_own %+d of lane 3" % off, _eob_at(3, off))]))
    # truncated streams: mid-symbol, mid-header
    body = list(_rand(71, 400)) + [("m", 30, 100)] * 5
    raw, starts = deflate([Dynamic(body)])
    cases.append(Case("blocks_truncated_mid_symbol", raw[:starts[0] // 8 + 150], 4096, status=CORRUPT))
    cases.append(Case("blocks_truncated_mid_header", raw[:starts[0] // 8 - 40], 4096, status=CORRUPT))
    cases.append(Case("blocks_truncated_fixed", deflate([Fixed(body)])[0][:200], 4096, status=CORRUPT))
    return cases


# ---- family: sync -----------------------------------------------------------------------------------
def family_sync():
    """Blocks of 44-bit symbols made almost wholly of one bits (the last codes of skewed 15-bit sets,
    extra bits all ones), so a lane that starts off the symbol grid stays off it through its 384-bit
    overlap: lanes start out of sync, are re-decoded, and a round runs out of its MAXREP repairs."""
    cases = []
    ll = spread(286, list(range(13)) + [256, 265, 266], SKEW16)   # 266: 15 ones, 1 extra bit
    dd = spread(30, list(range(14)) + [28, 29], SKEW16)           # 29: 15 ones, 13 extra bits
    for name, n, tail in (("sync_44bit_ones", 580, []), ("sync_44bit_ones_then_literals", 300, list(range(13)) * 40)):
        body = [0, 1, 2] + [("m", 14, 32768)] * n + tail
        cases.append(valid(name, [Stored(_rand(8, 32768)), Dynamic(body, ll=ll, dd=dd)], 40960,
                           [("lanes start out of sync: repairs > 0", lambda st: st["repairs"] > 0),
                            ("a round cut by MAXREP", lambda st: st["maxrep_cuts"] > 0)]))
    # the same grid with random extra bits: repairs without the cut
    r = _rng(9)
    body = [0, 1, 2] + [("m", 13 + int(r.integers(0, 2)), 24577 + int(r.integers(0, 8192))) for _ in range(500)]
    cases.append(valid("sync_44bit_random_extra", [Stored(_rand(8, 32768)), Dynamic(body, ll=ll, dd=dd)], 40960,
                       [("lanes start out of sync: repairs > 0", lambda st: st["repairs"] > 0)]))
    return cases


# ---- family: size -----------------------------------------------------------------------------------
def family_size():
    cases = []
    for name, blocks in (("size_short_fixed", [Fixed(list(_rand(81, 500)) + [("m", 100, 7)] * 20), Stored(_rand(82, 1595))]),
                         ("size_short_stored", [Stored(_rand(83, 4095))]),
                         ("size_long_match_crosses_end", [Stored(_rand(84, 3000)),
                                                          Fixed(list(_rand(85, 1000)) + [("m", 90, 50), ("m", 258, 300), 1])]),
                         ("size_long_stored", [Stored(_rand(86, 4097))])):
        data = execute(blocks)
        assert len(data) in (4095, 4097, 4349), (name, len(data))
        cases.append(Case(name, deflate(blocks)[0], 4096, status=SIZE, decoded=data))
    cases.append(valid("size_exact_after_mismatches", [Fixed(list(_rand(87, 300)) + [("m", 258, 300)] * 3)], 4096))
    return cases


FAMILIES = {
    "executor_ring": family_executor_ring,
    "executor_deps": family_executor_deps,
    "codes": family_codes,
    "headers": family_headers,
    "blocks": family_blocks,
    "sync": family_sync,
    "size": family_size,
}
_cache = {}


def family(name):
    """The family's cases, built once."""
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
        assert len({c.name for c in _cache[name]}) == len(_cache[name])
    return _cache[name]
