"""Hand-assembled bzip2 streams for the numcodecs.bz2 stage (kernels/bz2.hip): what the format allows
and libbz2's encoder never emits, at the edges the decoder has code of its own for. Test
infrastructure, no GPU.

  * BitWriter (MSB first) and an assembler at MTF-symbol level: a Block carries its symbol map, nGroups,
    the selector list, the code lengths of every table, the symbol sequence (RUNA = 0, RUNB = 1, MTF
    index + 1, end of block = alphabet - 1), origPtr, its CRC (computed or forced), the randomised bit;
    raw overrides (nGroups / nSelectors fields, unary selector values, the 5-bit start of a length
    list, the symbol map) build the corrupt cases. stream() joins blocks under a header digit, with the
    combined CRC (computed or forced) and trailing bytes; sections() gives every section's first bit.
  * rle1(), bwt(), mtf_symbols(): the naive forward transforms, to build small blocks from chosen bytes.
  * execute(): the byte-at-a-time reference over the blocks (runs, inverse MTF, inverse BWT through a
    stable sort, RLE1 inverse) and a trace of what it met: the `expect` of valid cases and the evidence
    for every case's `intent`.
  * Case: name, stream, `expect` (bytes) or `status`, `intent`: (text, predicate over the trace) pairs
    that must hold, `miss`: pairs that must not (a control beside an edge). FAMILIES groups them.
"""
from __future__ import annotations

from dataclasses import dataclass, field

OK, CORRUPT, SIZE = "OK", "CORRUPT_STREAM", "DECODED_SIZE_MISMATCH"
BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090
G = 50  # symbols per selector group
MAX_SEL = 18002


class BitWriter:
    def __init__(self):
        self.v = 0
        self.n = 0

    def bits(self, val, k):
        assert 0 <= val < (1 << k) or k == 0, (val, k)
        self.v = (self.v << k) | val
        self.n += k

    def bytes(self, pad=0):
        k = -self.n % 8
        return ((self.v << k) | (pad & ((1 << k) - 1))).to_bytes((self.n + k) // 8, "big")


_TAB = []
for _i in range(256):
    _c = _i << 24
    for _ in range(8):
        _c = ((_c << 1) ^ 0x04C11DB7 if _c & 0x80000000 else _c << 1) & 0xFFFFFFFF
    _TAB.append(_c)


def crc(data: bytes) -> int:
    """CRC-32/BZIP2: MSB first, polynomial 04C11DB7, initial value and final XOR FFFFFFFF."""
    c = 0xFFFFFFFF
    for b in data:
        c = ((c << 8) & 0xFFFFFFFF) ^ _TAB[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


def combine(crcs) -> int:
    c = 0
    for b in crcs:
        c = (((c << 1) | (c >> 31)) & 0xFFFFFFFF) ^ b
    return c


# ---- forward transforms -------------------------------------------------------------------------
def rle1(data: bytes) -> bytes:
    out, i = bytearray(), 0
    while i < len(data):
        j = i
        while j < len(data) and data[j] == data[i] and j - i < 255 + 4:
            j += 1
        n = j - i
        out += data[i:i + min(n, 4)]
        if n >= 4:
            out.append(n - 4)
        i = j
    return bytes(out)


def bwt(u: bytes):
    """(last column, origPtr) of the sorted rotations of u."""
    n = len(u)
    rot = sorted(range(n), key=lambda i: u[i:] + u[:i])
    return bytes(u[(i - 1) % n] for i in rot), rot.index(0)


def mtf_symbols(last: bytes, in_use):
    mtf, out, run = list(in_use), [], 0

    def flush():
        nonlocal run
        while run > 0:
            if run & 1:
                out.append(0)
                run = (run - 1) >> 1
            else:
                out.append(1)
                run = (run - 2) >> 1

    for b in last:
        j = mtf.index(b)
        if j == 0:
            run += 1
        else:
            flush()
            out.append(j + 1)
            mtf.insert(0, mtf.pop(j))
    flush()
    out.append(len(in_use) + 1)
    return out


def run_symbols(n):
    """RUNA / RUNB symbols (bijective base 2) of a run of n."""
    out = []
    while n > 0:
        if n & 1:
            out.append(0)
            n = (n - 1) >> 1
        else:
            out.append(1)
            n = (n - 2) >> 1
    return out


def flat_lens(n):
    """n code lengths of a complete code, as flat as possible."""
    k = n.bit_length() - 1
    if n == 1 << k:
        return [k] * n
    short = (1 << (k + 1)) - n
    return [k] * short + [k + 1] * (n - short)


def codes(lens):
    """hbAssignCodes: by length, then by symbol."""
    out, vec = {}, 0
    for n in range(min(lens), max(lens) + 1):
        for s, ln in enumerate(lens):
            if ln == n:
                out[s] = (vec, n)
                vec += 1
        vec <<= 1
    return out


# ---- blocks -------------------------------------------------------------------------------------
@dataclass
class Block:
    symbols: list
    in_use: list                     # byte values, ascending
    lens: list                       # per table: alphabet code lengths
    selectors: list                  # table of each group of 50 symbols
    orig: int = 0
    crc: int | None = None           # None: of the bytes the block decodes to
    randomised: int = 0
    n_groups_field: int | None = None
    n_sel_field: int | None = None
    sel_unary: list | None = None    # raw unary values instead of the MTF coding of `selectors`
    extra_selectors: int = 0         # more selectors than groups (all table 0)
    len_start: dict = field(default_factory=dict)  # table -> raw 5-bit start value
    used_map: list | None = None     # raw symbol map (16 + 16 x 16 bits as (used16, [rows]))

    @property
    def alpha(self):
        return len(self.in_use) + 2


def block_of(data: bytes, n_groups=2, lens=None, selectors=None, **kw) -> Block:
    """The block libbz2 would decode to `data`: RLE1, BWT, MTF with flat tables (or the given ones)."""
    u = rle1(data)
    last, orig = bwt(u)
    in_use = sorted(set(u))
    syms = mtf_symbols(last, in_use)
    ngrp = (len(syms) + G - 1) // G
    lens = lens or [flat_lens(len(in_use) + 2)] * n_groups
    selectors = selectors or [g % len(lens) for g in range(ngrp)]
    return Block(syms, in_use, lens, selectors, orig, **kw)


def raw_block(u: bytes, **kw) -> Block:
    """A block whose bytes before RLE1 are exactly u (an RLE1 form libbz2's encoder would not write)."""
    last, orig = bwt(u)
    in_use = sorted(set(u))
    syms = mtf_symbols(last, in_use)
    lens = kw.pop("lens", None) or [flat_lens(len(in_use) + 2)] * 2
    selectors = kw.pop("selectors", None) or [g % len(lens) for g in range((len(syms) + G - 1) // G)]
    return Block(syms, in_use, lens, selectors, orig, **kw)


def write_block(w: BitWriter, b: Block, crc_value: int, marks: dict):
    marks["magic"] = w.n
    w.bits(BLOCK_MAGIC, 48)
    marks["crc"] = w.n
    w.bits(crc_value, 32)
    w.bits(b.randomised, 1)
    marks["orig"] = w.n
    w.bits(b.orig, 24)
    marks["map"] = w.n
    if b.used_map is not None:
        used16, rows = b.used_map
    else:
        rows = [sum(1 << (15 - j) for j in range(16) if 16 * i + j in b.in_use) for i in range(16)]
        used16 = sum(1 << (15 - i) for i in range(16) if rows[i])
        rows = [r for r in rows if r]
    w.bits(used16, 16)
    for r in rows:
        w.bits(r, 16)
    marks["groups"] = w.n
    w.bits(len(b.lens) if b.n_groups_field is None else b.n_groups_field, 3)
    sels = list(b.selectors) + [0] * b.extra_selectors
    w.bits(len(sels) if b.n_sel_field is None else b.n_sel_field, 15)
    marks["selectors"] = w.n
    if b.sel_unary is not None:
        unary = b.sel_unary
    else:
        order, unary = list(range(6)), []
        for s in sels:
            j = order.index(s)
            unary.append(j)
            order.insert(0, order.pop(j))
    for j in unary:
        w.bits((1 << (j + 1)) - 2, j + 1)
    marks["lens"] = w.n
    for t, lens in enumerate(b.lens):
        cur = b.len_start.get(t, lens[0])
        w.bits(cur, 5)
        for ln in lens:
            while cur != ln:
                w.bits(2 if ln > cur else 3, 2)
                cur += 1 if ln > cur else -1
            w.bits(0, 1)
    marks["symbols"] = w.n
    tabs = [codes(lens) for lens in b.lens]
    for k, s in enumerate(b.symbols):
        c, n = tabs[b.selectors[k // G]][s]
        w.bits(c, n)
    marks["end"] = w.n


def stream(blocks, level=9, combined=None, trailer=b"", head=b"BZh", pad=0, marks=None) -> bytes:
    w = BitWriter()
    for c in head + bytes([48 + level]):
        w.bits(c, 8)
    crcs = []
    for k, b in enumerate(blocks):
        c = b.crc if b.crc is not None else crc(execute_block(b, {})[0])
        crcs.append(c)
        m = {}
        write_block(w, b, c, m)
        if marks is not None:
            marks[k] = m
    if marks is not None:
        marks["end_magic"] = w.n
    w.bits(END_MAGIC, 48)
    w.bits(combine(crcs) if combined is None else combined, 32)
    return w.bytes(pad) + trailer


# ---- the reference executor ---------------------------------------------------------------------
def un_rle1(u: bytes, tr: dict) -> bytes:
    out, c = bytearray(), 0
    counts, stretches, sync, k0 = [], [], 0, 0
    for i, b in enumerate(u):
        if i >= 2 and u[i] != u[i - 1] and u[i - 1] != u[i - 2]:
            sync += 1
        if c == 4:
            out += bytes([u[i - 1]]) * b
            counts.append((b, u[i - 1]))
            c = 0
            continue
        out.append(b)
        if c == 0 or b != u[i - 1]:
            if c:
                stretches.append(i - k0)
            k0, c = i, 1
        else:
            c += 1
            if c == 4:
                stretches.append(4)
    if c == 4:
        # libbz2 reads the count without looking for the block's end and then reports a data error
        # (unRLE_obuf_to_output_*: nblock_used passes save_nblock + 1)
        raise ValueError("the block ends between four equal bytes and their count")
    tr.update(rle1_counts=counts, rle1_sync=sync, rle1_len=len(u))
    return bytes(out)


def equal_stretches(u: bytes):
    """Lengths of the maximal stretches of equal bytes of u."""
    out, i = [], 0
    while i < len(u):
        j = i
        while j < len(u) and u[j] == u[i]:
            j += 1
        out.append(j - i)
        i = j
    return out


def execute_block(b: Block, tr: dict, level=9):
    """(decoded bytes, bytes before RLE1) of one block; raises ValueError where libbz2 reports an error."""
    mtf, last, run, n = list(b.in_use), bytearray(), 0, 1
    eob, limit = b.alpha - 1, 100000 * level
    runs, idx_max, ended = [], 0, False
    for s in b.symbols:
        if s <= 1:
            run += (s + 1) * n
            n *= 2
            continue
        if run:
            if len(last) + run > limit:
                raise ValueError("run past the block limit")
            last += bytes([mtf[0]]) * run
            runs.append(run)
            run, n = 0, 1
        if s == eob:
            ended = True
            break
        if len(last) >= limit:
            raise ValueError("block limit")
        idx_max = max(idx_max, s - 1)
        mtf.insert(0, mtf.pop(s - 1))
        last.append(mtf[0])
    if not ended:
        raise ValueError("no end-of-block symbol")
    if b.orig >= len(last):
        raise ValueError("origPtr")
    order = sorted(range(len(last)), key=lambda i: last[i])  # stable
    p, u = order[b.orig], bytearray()
    for _ in range(len(last)):
        u.append(last[p])
        p = order[p]
    info = {}
    out = un_rle1(bytes(u), info)
    tr.setdefault("blocks", []).append({**info, **{
        "nsym": len(b.symbols), "nblock": len(last), "runs": runs, "mtf_max": idx_max, "orig": b.orig,
        "n_groups": len(b.lens), "selectors": list(b.selectors), "alpha": b.alpha,
        "n_selectors": len(b.selectors) + b.extra_selectors,
        "len_used": sorted({b.lens[b.selectors[k // G]][s] for k, s in enumerate(b.symbols)}),
        "lens": b.lens, "eob_pos": len(b.symbols) - 1, "u": bytes(u), "last": bytes(last)}})
    return out, bytes(u)


def execute(blocks, level=9):
    tr = {}
    out = b"".join(execute_block(b, tr, level)[0] for b in blocks)
    return out, tr


# ---- cases --------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    stream: bytes
    expect: bytes | None = None
    status: str = OK
    trace: dict = field(default_factory=dict)
    intent: list = field(default_factory=list)
    miss: list = field(default_factory=list)
    n_blocks: int = 0
    level: int = 9


PAD = 4096  # every valid case up to this size is padded to it by one more block: a family decodes in few calls


def valid(name, blocks, intent=(), miss=(), level=9, **kw) -> Case:
    expect, tr = execute(blocks, level)
    if len(expect) < PAD:
        blocks = list(blocks) + [block_of(_text(PAD - len(expect), len(expect) + 1))]
        expect, tr = execute(blocks, level)
    return Case(name, stream(blocks, level, **kw), expect, OK, tr, list(intent), list(miss), len(blocks), level)


def corrupt(name, s: bytes, intent=(), trace=None) -> Case:
    return Case(name, s, None, CORRUPT, trace or {}, list(intent))


def _text(n, seed=1, alphabet=b"abcdefgh \n"):
    x, out = seed * 2654435761 % (1 << 32), bytearray()
    for _ in range(n):
        x = (x * 1103515245 + 12345) % (1 << 31)
        out.append(alphabet[(x >> 16) % len(alphabet)])
    return bytes(out)


def _syms_block(symbols, in_use, lens=None, selectors=None, orig=0, **kw) -> Block:
    alpha = len(in_use) + 2
    lens = lens or [flat_lens(alpha)] * 2
    selectors = selectors or [g % len(lens) for g in range((len(symbols) + G - 1) // G)]
    return Block(list(symbols), list(in_use), lens, selectors, orig, **kw)


def _blk(tr, k=0):
    return tr["blocks"][k]


def _fit_orig(b: Block, tries=64) -> Block:
    """libbz2 decodes a chosen symbol sequence for any origPtr below nblock (it just walks the successor
    vector); what it rejects is an RLE1 form that ends between four equal bytes and their count. Take
    the first origPtr whose bytes parse."""
    for orig in range(tries):
        b.orig = orig
        try:
            execute_block(b, {})
            return b
        except ValueError:
            continue
    raise AssertionError("no origPtr gives a parsable block")


def tables_family():
    data = _text(700, 3)
    full = bytes(range(256)) * 2 + _text(300, 5, bytes(range(256)))
    c = []
    # ngroups2 is also the control beside the other edges of this family: it must miss each of them
    c.append(valid("ngroups2", [block_of(data, 2)], [("2 tables", lambda t: _blk(t)["n_groups"] == 2)],
                   [("6 tables", lambda t: _blk(t)["n_groups"] == 6),
                    ("a 1-bit code is used", lambda t: 1 in _blk(t)["len_used"]),
                    ("a 20-bit code is used", lambda t: 20 in _blk(t)["len_used"]),
                    ("alphabet 258", lambda t: _blk(t)["alpha"] == 258),
                    ("alphabet 3", lambda t: _blk(t)["alpha"] == 3),
                    ("a table alternates 1 and 20", lambda t: any(set(l) == {1, 20} for l in _blk(t)["lens"])),
                    ("n_selectors > 18002", lambda t: _blk(t)["n_selectors"] > MAX_SEL)]))
    b6 = block_of(data, 6)
    c.append(valid("ngroups6_selector_change_every_group", [b6],
                   [("6 tables", lambda t: _blk(t)["n_groups"] == 6),
                    ("every group changes the table", lambda t: all(
                        a != b for a, b in zip(_blk(t)["selectors"], _blk(t)["selectors"][1:])))]))
    bm = block_of(data, 6)
    bm.selectors = [(5 * (g + 1)) % 6 for g in range(len(bm.selectors))]  # each the last of the MTF list
    c.append(valid("selector_mtf_maximum", [bm], [("unary 5 every time", lambda t: all(
        (5 * (g + 1)) % 6 == s for g, s in enumerate(_blk(t)["selectors"])))]))
    # a 20-bit code and a 1-bit code: lengths 1, 2, ..., 19, 20, 20 over the most frequent symbols
    u = rle1(_text(400, 7, bytes(range(19))))
    blk = raw_block(u)
    ladder = list(range(1, 21)) + [20]
    assert blk.alpha == 21, blk.alpha
    blk.lens = [ladder, ladder[::-1]]
    blk.selectors = [0] * len(blk.selectors)
    c.append(valid("code_1bit_and_20bit", [blk],
                   [("a 1-bit code is used", lambda t: 1 in _blk(t)["len_used"]),
                    ("a 20-bit code is used", lambda t: 20 in _blk(t)["len_used"])]))
    c.append(valid("all_258_symbols", [block_of(full, 3)], [("alphabet 258", lambda t: _blk(t)["alpha"] == 258),
                                                            ("index 255 referenced", lambda t: _blk(t)["mtf_max"] == 255)]))
    c.append(valid("one_byte_value_alphabet3", [block_of(b"qqq", 2)], [("alphabet 3", lambda t: _blk(t)["alpha"] == 3)]))
    # the delta coding walking 1 -> 20 -> 1 in a table no selector uses
    bw = block_of(data, 3)
    a = bw.alpha
    bw.lens = [bw.lens[0], [1 if k % 2 == 0 else 20 for k in range(a)], bw.lens[0]]
    bw.selectors = [0 if g % 2 == 0 else 2 for g in range(len(bw.selectors))]
    c.append(valid("length_deltas_1_20_1", [bw], [("a table alternates 1 and 20", lambda t: any(
        set(l) == {1, 20} for l in _blk(t)["lens"]))]))
    # more selectors than groups, and more than 18,002 of them (read and dropped)
    bx = block_of(data, 2, extra_selectors=MAX_SEL + 40)
    c.append(valid("selectors_beyond_18002", [bx], [("n_selectors > 18002", lambda t: _blk(t)["n_selectors"] > MAX_SEL),
                                                    ("more selectors than groups", lambda t: _blk(t)["n_selectors"] > -(-_blk(t)["nsym"] // G))]))
    return c


def groups_family():
    c = []
    for nsym in (50, 51, 100):
        # nsym - 1 MTF symbols of alternating indices, then the end of block: first of a group when nsym
        # is 51, last of one when it is 50 or 100
        in_use = [65, 66, 67]
        body = [2 + (k % 2) for k in range(nsym - 1)]
        b = _fit_orig(_syms_block(body + [4], in_use))
        c.append(valid(f"block_of_{nsym}_symbols", [b], [
            (f"{nsym} symbols", lambda t, n=nsym: _blk(t)["nsym"] == n),
            ("end of block first in its group" if nsym == 51 else "end of block last in its group",
             lambda t, n=nsym: _blk(t)["eob_pos"] % G == (0 if n == 51 else G - 1))]))
    ctl = _fit_orig(_syms_block([2 + (k % 2) for k in range(72)] + [4], [65, 66, 67]))
    c.append(valid("groups_control_73_symbols", [ctl], [("73 symbols", lambda t: _blk(t)["nsym"] == 73)],
                   [("end of block first in its group", lambda t: _blk(t)["eob_pos"] % G == 0),
                    ("end of block last in its group", lambda t: _blk(t)["eob_pos"] % G == G - 1),
                    ("a whole number of groups", lambda t: _blk(t)["nsym"] % G == 0)]))
    return c


def runs_family():
    c = []
    for n in (1, 2, 3, 255, 256, 65536):
        # a run of n equal bytes 'z' inside the BWT column, an 'a' after it
        in_use = [97, 122]
        syms = [2] + run_symbols(n) + [2, 3]  # 'z' (index 1), n more of it, 'a', end of block
        b = _fit_orig(_syms_block(syms, in_use))
        c.append(valid(f"run_{n}", [b], [(f"a run of {n}", lambda t, n=n: n in _blk(t)["runs"])], level=9))
    ctl = _fit_orig(_syms_block([2, 2, 2, 2, 2, 3], [97, 122]))
    c.append(valid("runs_control_no_run", [ctl], [("five symbols, no RUNA / RUNB", lambda t: _blk(t)["nblock"] == 5)],
                   [("any run", lambda t: bool(_blk(t)["runs"])),
                    ("nblock at the level's limit", lambda t: _blk(t)["nblock"] == 100000)]))
    lim = 100000
    b = _syms_block(run_symbols(lim) + [3], [97, 122])
    c.append(valid("run_to_the_block_limit", [b], [("nblock == 100,000 at level 1", lambda t: _blk(t)["nblock"] == 100000)],
                   level=1))
    b = _syms_block(run_symbols(lim + 1) + [3], [97, 122], crc=0)
    c.append(corrupt("run_past_the_block_limit", stream([b], 1, combined=0),
                     [("the run is one past level 1's limit", lambda t: t["run"] == t["limit"] + 1)],
                     {"run": lim + 1, "limit": 100000}))
    return c


def mtf_family():
    full = bytes(range(256))
    b = block_of(full + full[::-1] + full, 2)
    c = [valid("mtf_index_255", [b], [("index 255", lambda t: _blk(t)["mtf_max"] == 255)]),
         valid("mtf_control_small_alphabet", [block_of(_text(300, 19))], [],
               [("a 10-letter text never goes past index 9", lambda t: _blk(t)["mtf_max"] == 255)])]
    in_use = list(range(256))
    syms = [256 if k % 2 == 0 else 2 for k in range(600)] + [257]
    b2 = _fit_orig(_syms_block(syms, in_use))
    c.append(valid("mtf_alternating_front_back", [b2], [("index 255 and index 1 alternate", lambda t: _blk(t)["mtf_max"] == 255)]))
    return c


def bwt_family():
    data = _text(333, 11)
    c = []
    # rotate the input until the BWT's origPtr is 0 / nblock - 1
    u = rle1(data)
    hit = {}
    for r in range(len(u)):
        v = u[r:] + u[:r]
        _, o = bwt(v)
        if o == 0 and 0 not in hit:
            hit[0] = v
        if o == len(u) - 1 and "last" not in hit:
            hit["last"] = v
    c.append(valid("origptr_0", [raw_block(hit[0])], [("origPtr 0", lambda t: _blk(t)["orig"] == 0)]))
    c.append(valid("origptr_last", [raw_block(hit["last"])],
                   [("origPtr nblock - 1", lambda t: _blk(t)["orig"] == _blk(t)["nblock"] - 1)]))
    c.append(valid("bwt_control", [block_of(data)], [("nblock > 2", lambda t: _blk(t)["nblock"] > 2)],
                   [("origPtr 0", lambda t: _blk(t)["orig"] == 0),
                    ("origPtr nblock - 1", lambda t: _blk(t)["orig"] == _blk(t)["nblock"] - 1),
                    ("one byte value", lambda t: len(set(_blk(t)["last"])) == 1),
                    ("nblock 1", lambda t: _blk(t)["nblock"] == 1)]))
    c.append(valid("one_symbol", [block_of(b"x")], [("nblock 1", lambda t: _blk(t)["nblock"] == 1)]))
    c.append(valid("all_equal_stable_sort", [raw_block(b"kkk")],
                   [("one byte value, three entries", lambda t: set(_blk(t)["last"]) == {107} and _blk(t)["nblock"] == 3)]))
    return c


def rle1_family():
    c = []

    def case(name, u, intent, miss=()):
        c.append(valid(name, [raw_block(u)], intent, miss))

    for cnt in (0, 251, 255):
        case(f"four_equal_count_{cnt}", b"ab" + b"cccc" + bytes([cnt]) + b"de",
             [(f"count {cnt}", lambda t, cnt=cnt: (cnt, 99) in _blk(t)["rle1_counts"])])
    case("three_equal_then_change", b"abcccdcccd", [("no count byte", lambda t: not _blk(t)["rle1_counts"])],
         [("a control: no stretch of 4", lambda t: 4 in equal_stretches(_blk(t)["u"]))])
    case("count_equals_the_run_byte", b"xy" + b"aaaa" + bytes([97]) + b"z",
         [("count 97 of byte 97", lambda t: (97, 97) in _blk(t)["rle1_counts"]),
          ("five equal bytes before RLE1", lambda t: 5 in equal_stretches(_blk(t)["u"]))])
    for m in range(5):
        n = 10 + m
        case(f"stretch_mod5_{m}", b"q" + b"\x05" * n + b"r",
             [(f"a stretch of {n}", lambda t, n=n: n in equal_stretches(_blk(t)["u"]))])
    # four equal bytes that end a block without their count: libbz2 reports a data error
    open_run = raw_block(b"abc" + b"dddd", crc=crc(b"abcdddd"))
    c.append(corrupt("run_cut_by_the_block_end", stream([open_run], combined=combine([crc(b"abcdddd")])),
                     [("the bytes before RLE1 end in four equal bytes", lambda t: t["u"][-4:] == b"dddd" and t["u"][-5] != 100)],
                     {"u": b"abcdddd"}))
    # equal bytes across a block's end: each block parses afresh, so block 1's 'e' and 3 are literals
    c.append(valid("run_crossing_two_blocks", [raw_block(b"ab" + b"eee"), raw_block(b"e\x03" + b"ee" + b"fg")],
                   [("block 0 ends in three equal bytes", lambda t: _blk(t, 0)["u"].endswith(b"eee")),
                    ("block 1 goes on with the same byte", lambda t: _blk(t, 1)["u"].startswith(b"e")),
                    ("no count byte in either", lambda t: not _blk(t, 0)["rle1_counts"] and not _blk(t, 1)["rle1_counts"])]))
    long = (b"\x04" * 4 + b"\x04") * 500  # 2,500 equal bytes: four literals and a count of 4, 500 times
    case("long_input_without_sync_point", long, [("no synchronisation point", lambda t: _blk(t)["rle1_sync"] == 0),
                                                 ("2,500 bytes", lambda t: _blk(t)["rle1_len"] == 2500)],
         [("a control: every count is 4", lambda t: any(v != 4 for v, _ in _blk(t)["rle1_counts"]))])
    alt = bytes((k * 7 + k // 3) % 251 for k in range(1500))
    assert all(alt[k] != alt[k - 1] for k in range(1, len(alt)))
    case("every_position_a_sync_point", alt, [("all but the first two", lambda t: _blk(t)["rle1_sync"] == _blk(t)["rle1_len"] - 2)])
    return c


def magic_family():
    c = []
    # 254 codes of 8 bits and 4 of 9: symbol s < 254 has code s, so symbols 0x31 0x41 0x59 0x26 0x53 0x59
    # spell the block magic inside the payload
    lens = [8] * 254 + [9] * 4
    data = bytes(range(256)) * 3
    b = block_of(data, 2, lens=[lens, lens])
    spell = [0x31, 0x41, 0x59, 0x26, 0x53, 0x59]
    at = 150
    b.symbols[at:at] = spell
    b.selectors = [g % 2 for g in range((len(b.symbols) + G - 1) // G)]
    _fit_orig(b)
    inside = valid("block_magic_inside_the_payload", [b])
    inside.intent = [("the block magic occurs once more than there are blocks",
                      lambda t, s=inside.stream, n=inside.n_blocks: _bit_count(s, BLOCK_MAGIC) == n + 1)]
    c.append(inside)
    ctl = valid("magic_control", [block_of(data, 2, lens=[lens, lens])])
    ctl.miss = [("no magic beyond the blocks' own", lambda t, s=ctl.stream, n=ctl.n_blocks: _bit_count(s, BLOCK_MAGIC) != n)]
    c.append(ctl)
    plain = block_of(_text(500, 13))
    junk = BitWriter()
    junk.bits(5, 3)
    junk.bits(BLOCK_MAGIC, 48)
    junk.bits(0x1234567, 29)
    c.append(valid("block_magic_in_trailing_junk", [plain],
                   [], trailer=junk.bytes() + b"tail"))
    c[-1].intent = [("the block magic occurs in the trailing bytes, not byte-aligned", lambda t, s=c[-1].stream, n=c[-1].n_blocks:
                     _bit_count(s, BLOCK_MAGIC) == n + 1 and _bit_count(s[-len(junk.bytes()) - 4:], BLOCK_MAGIC) == 1)]
    second = stream([block_of(b"second stream, ignored")])
    c.append(valid("second_stream_ignored", [plain], [], trailer=second))
    c[-1].intent = [("a whole stream follows: two end magics, one more block", lambda t, s=c[-1].stream, n=c[-1].n_blocks:
                     s.endswith(second) and _bit_count(s, END_MAGIC) == 2 and _bit_count(s, BLOCK_MAGIC) == n + 1)]
    return c


def _bit_count(s: bytes, magic: int) -> int:
    v, n = int.from_bytes(s, "big"), len(s) * 8
    return sum(1 for k in range(n - 47) if (v >> (n - 48 - k)) & ((1 << 48) - 1) == magic)


def corrupt_family():
    data = _text(900, 17)
    base = block_of(data, 3)
    marks = {}
    good = stream([base], marks=marks)
    c = []
    m = marks[0]
    order = ["magic", "crc", "orig", "map", "groups", "selectors", "lens", "symbols", "end"]
    inside = ("the cut lies inside the section", lambda t: t["lo"] < t["cut_bits"] < t["hi"])

    def cut_case(name, nbytes, lo, hi):
        c.append(corrupt(name, good[:nbytes], [inside], {"cut_bits": 8 * nbytes, "lo": lo, "hi": hi}))

    for sec in order[1:-1]:
        cut_case(f"truncated_in_{sec}", (m[sec] + 3) // 8 + 1, m[sec], m[order[order.index(sec) + 1]])
    cut_case("truncated_in_symbols_mid", (m["symbols"] + m["end"]) // 16, m["symbols"], m["end"])
    em = marks["end_magic"]
    assert em == m["end"]
    cut_case("truncated_in_end_magic", (em + 20) // 8, em, em + 48)
    cut_case("truncated_in_combined_crc", len(good) - 2, em + 48, em + 80)

    def variant(**kw):
        b = block_of(data, 3)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    right = crc(data)
    nsel = len(base.selectors)

    def field_case(name, intent, combined=None, **kw):
        """One field of an otherwise valid block set wrong; the trace is the block as it was assembled."""
        b = variant(**kw)
        stored = b.crc if b.crc is not None else right
        tr = {"block": b, "stored_crc": stored, "computed_crc": right,
              "combined": combine([stored]) if combined is None else combined,
              "nblock": len(rle1(data)), "n_tables": len(b.lens)}
        c.append(corrupt(name, stream([b], combined=tr["combined"]), [intent], tr))

    field_case("bad_block_crc", ("the stored block CRC differs, the combined CRC agrees with it",
                                 lambda t: t["stored_crc"] != t["computed_crc"] and t["combined"] == combine([t["stored_crc"]])),
               crc=right ^ 0x10)
    field_case("bad_combined_crc", ("the block CRC is right, the combined one is not",
                                    lambda t: t["stored_crc"] == t["computed_crc"] and t["combined"] != combine([t["stored_crc"]])),
               combined=combine([right]) ^ 1)
    field_case("origptr_equals_nblock", ("origPtr == nblock", lambda t: t["block"].orig == t["nblock"]),
               orig=len(rle1(data)), crc=right)
    field_case("ngroups_1", ("the field says 1", lambda t: t["block"].n_groups_field == 1), n_groups_field=1, crc=right)
    field_case("ngroups_7", ("the field says 7", lambda t: t["block"].n_groups_field == 7), n_groups_field=7, crc=right)
    field_case("nselectors_0", ("the field says 0", lambda t: t["block"].n_sel_field == 0 and t["block"].sel_unary == []),
               n_sel_field=0, sel_unary=[], crc=right)
    field_case("selector_index_past_ngroups", ("a unary value equal to the number of tables",
                                               lambda t: max(t["block"].sel_unary) == t["n_tables"]),
               sel_unary=[0, 3] + [0] * (nsel - 2), crc=right)
    field_case("code_length_0", ("a table's lengths start at 0", lambda t: 0 in t["block"].len_start.values()),
               len_start={1: 0}, crc=right)
    field_case("code_length_21", ("a table's lengths start at 21", lambda t: 21 in t["block"].len_start.values()),
               len_start={1: 21}, crc=right)
    field_case("empty_symbol_map", ("no byte value is in use", lambda t: t["block"].used_map == (0, [])),
               used_map=(0, []), crc=right)
    field_case("randomised_bit", ("the bit is set, all else is valid", lambda t: t["block"].randomised == 1
                                  and t["stored_crc"] == t["computed_crc"]), randomised=1, crc=right)
    noeob = variant(crc=right)
    noeob.symbols = noeob.symbols[:-1]
    c.append(corrupt("missing_end_of_block", stream([noeob]),
                     [("no symbol is the end of block", lambda t: t["eob"] not in t["symbols"])],
                     {"eob": noeob.alpha - 1, "symbols": noeob.symbols}))
    head = ("only the four header bytes differ from the valid stream", lambda t: t["s"][4:] == good[4:] and t["s"][:4] == t["head"] != good[:4])
    for name, h in (("header_digit_0", b"BZh0"), ("wrong_magic", b"BZg9")):
        c.append(corrupt(name, h + good[4:], [head], {"s": h + good[4:], "head": h}))
    c.append(corrupt("empty_input", b"", [("no bytes", lambda t: t["s"] == b"")], {"s": b""}))
    return c


def families():
    return {"tables": tables_family(), "groups": groups_family(), "runs": runs_family(), "mtf": mtf_family(),
            "bwt": bwt_family(), "rle1": rle1_family(), "magic": magic_family(), "corrupt": corrupt_family()}
