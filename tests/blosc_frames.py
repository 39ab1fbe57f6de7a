"""Hand-built c-blosc 1.x frames for the blosc LZ decoders (zarrs_amd/csrc/kernels/blosc.hip): token-level
writers for the LZ4 block, blosclz and raw snappy formats that emit exactly the fields they are told
to, a byte-at-a-time reference executor of each format, a frame assembler (header, bstarts,
{csize, payload} per split; every header field free), numpy shuffle / bitshuffle, and a model of
LzG's accounting (input window, output ring, far copies) for a stream at a given address residue.
Pure Python, no GPU: tests/test_blosc_frames_model.py referees the lz4 and blosclz cases with c-blosc
through the oracle and checks every case's intent against the model; tests/test_gpu_blosc_frames.py
feeds the frames to the kernels.

Every stream case states what it is there for as predicates over the model's trace, so a change of the
kernel's constants cannot quietly move a case off its edge."""
import functools
from dataclasses import dataclass, field

import numpy as np

# The kernels' constants, from this one place: ZG_LZW (input window bytes), ZG_LZ_RING (output ring
# bytes) and ZG_LZM_G (lanes per stream of the narrow path; the wide path uses 64) in blosc.hip.
LZW = 1024
LZR = 4096
G_NARROW = 32
G_WIDE = 64
LZRM = LZR - 1

OK, CORRUPT, LENIENT = "ok", "corrupt", "lenient"
COMP = {"blosclz": 0, "lz4": 1, "snappy": 2}
SIZES = (8192, 16384, 131072)  # the decoded chunk sizes of all cases (a plan has one leaf chunk shape)
TAIL = 16  # final literals of a padded stream


def rnd(n, seed=1):
    """n pseudo-random bytes in 1..250 (never the 0xA5 sentinel's run, never a long repeat)."""
    return bytes(np.random.default_rng(seed).integers(1, 251, n, dtype=np.uint8))


def ext255(v):
    """v as LZ4 / blosclz extension bytes: 255s, then one byte below 255 (so 255 is [255, 0])."""
    return [255] * (v // 255) + [v % 255]


def varint(v, nbytes=None):
    out = bytearray()
    while True:
        b = v & 127
        v >>= 7
        more = v or (nbytes is not None and len(out) + 1 < nbytes)
        out.append(b | (128 if more else 0))
        if not more:
            return bytes(out)


# ---------------------------------------------------------------------------------------------
# token-level writers: every byte is tagged with its field kind
# ---------------------------------------------------------------------------------------------
class _W:
    def __init__(self):
        self.b = bytearray()
        self.kinds = []  # (position, field kind) of every byte
        self.n = 0       # the decoded size of what was written (as the fields state it)

    def put(self, kind, *vals):
        for v in vals:
            self.kinds.append((len(self.b), kind))
            self.b.append(v)

    def data(self, kind, bs):
        for i, v in enumerate(bs):
            k = kind + ("0" if i == 0 else "N" if i == len(bs) - 1 else "")
            self.kinds.append((len(self.b), k))
            self.b.append(v)

    def last(self, kind):
        return max(p for p, k in self.kinds if k == kind)

    def kind_at(self, p):
        return dict(self.kinds).get(p)

    def bytes(self):
        return bytes(self.b)


class Lz4W(_W):
    """LZ4 block: sequences {token, ll extension, literals, offset u16 le, ml extension}."""

    def seq(self, lits, off=None, ml=None, ll_ext=None, ml_ext=None):
        ll = len(lits)
        if ll_ext is None:
            ll_ext = ext255(ll - 15) if ll >= 15 else []
        m = 0
        if off is not None:
            assert ml >= 4
            if ml_ext is None:
                ml_ext = ext255(ml - 19) if ml >= 19 else []
            m = min(ml - 4, 15)
        self.put("token", (min(ll, 15) << 4) | m)
        self.put("ll_ext", *ll_ext)
        self.data("lit", lits)
        self.n += ll + (ml if off is not None else 0)
        if off is not None:
            self.put("off_lo", off & 255)
            self.put("off_hi", off >> 8)
            self.put("ml_ext", *ml_ext)
        return self


class BlzW(_W):
    """blosclz: control bytes; < 32 a literal run of c + 1, else a match (see k_blosclz's comment)."""

    def lit(self, lits, high=0):
        assert 1 <= len(lits) <= 32
        self.put("ctrl", (len(lits) - 1) | (high << 5))  # high bits: only the first control byte may carry them
        self.data("lit", lits)
        self.n += len(lits)
        return self

    def lits(self, lits):
        for i in range(0, len(lits), 32):
            self.lit(lits[i:i + 32])
        return self

    def match(self, dist, ln, far=None, ext=None):
        assert ln >= 3 and dist >= 1
        far = dist > 8191 if far is None else far
        hi = min(ln - 2, 7)
        lo5 = 31 if far else (dist - 1) >> 8
        if ext is None:
            ext = ext255(ln - 9) if hi == 7 else []
        code = 255 if far else (dist - 1) & 255
        assert far or not (lo5 == 31 and code == 255), "8192 is the far form's value 0"
        self.put("ctrl", (hi << 5) | lo5)
        self.put("len_ext", *ext)
        self.n += ln
        self.put("dist", code)
        if far:
            assert 0 <= dist - 8192 <= 65535
            self.put("far_hi", (dist - 8192) >> 8)
            self.put("far_lo", (dist - 8192) & 255)
        return self


class SnW(_W):
    """raw snappy: varint preamble, then literal / copy elements."""

    def preamble(self, n, nbytes=None):
        self.put("pre", *varint(n, nbytes))
        return self

    def literal(self, lits, width=None):
        n = len(lits)
        assert n >= 1
        if width is None:
            width = 0 if n <= 60 else max(1, ((n - 1).bit_length() + 7) // 8)
        if width == 0:
            assert n <= 60
            self.put("tag", (n - 1) << 2)
        else:
            assert n - 1 < 1 << (8 * width)
            self.put("tag", (59 + width) << 2)
            for i, v in enumerate((n - 1).to_bytes(width, "little")):
                self.put(f"len_b{i}", v)
        self.data("lit", lits)
        self.n += n
        return self

    def copy(self, off, ln, form=None):
        self.n += ln
        if form is None:
            form = 1 if (4 <= ln <= 11 and off < 2048) else 2 if off < 65536 else 3
        if form == 1:
            assert 4 <= ln <= 11 and off < 2048
            self.put("tag", 1 | ((ln - 4) << 2) | ((off >> 8) << 5))
            self.put("off1", off & 255)
        else:
            assert 1 <= ln <= 64
            self.put("tag", form | ((ln - 1) << 2))
            for i, v in enumerate(off.to_bytes(2 if form == 2 else 4, "little")):
                self.put(f"off{2 if form == 2 else 4}_{i}", v)
        return self


# ---- the seeded snappy encoder of tests/test_gpu_blosc.py (every element form, by chance) ----
def _snappy_literal(out, lit, rng):
    while lit:
        n = len(lit) if len(lit) <= 200 else int(rng.integers(1, len(lit) + 1))
        if n <= 60 and rng.random() < 0.7:
            out.append((n - 1) << 2)
        else:  # 60..63: the length - 1 in 1..4 little-endian bytes (any width that holds it is valid)
            nb = max(1, ((n - 1).bit_length() + 7) // 8)
            nb = min(4, nb + int(rng.integers(0, 2)))
            out.append((59 + nb) << 2)
            out += (n - 1).to_bytes(nb, "little")
        out += lit[:n]
        lit = lit[n:]


def _snappy_copy(out, off, n, rng):
    while n:
        if 4 <= n <= 11 and off < 2048 and rng.random() < 0.6:
            out.append(1 | ((n - 4) << 2) | ((off >> 8) << 5))
            out.append(off & 255)
            return
        m = min(n, 64)
        if n - m and n - m < 4:  # keep the remainder encodable (a copy of >= 1 byte is fine too)
            m = n - 4 if n > 4 else n
        if off < 65536 and rng.random() < 0.7:
            out.append(2 | ((m - 1) << 2))
            out += off.to_bytes(2, "little")
        else:
            out.append(3 | ((m - 1) << 2))
            out += off.to_bytes(4, "little")
        n -= m


def _snappy_compress(data, rng):
    out = bytearray(varint(len(data)))
    table, i, lit0, n = {}, 0, 0, len(data)
    while i + 4 <= n:
        key = data[i:i + 4]
        j = table.get(key)
        table[key] = i
        if j is not None:
            m = 4
            while i + m < n and data[j + m] == data[i + m] and m < 300:
                m += 1
            _snappy_literal(out, data[lit0:i], rng)
            _snappy_copy(out, i - j, m, rng)
            i += m
            lit0 = i
        else:
            i += 1
    _snappy_literal(out, data[lit0:], rng)
    return bytes(out)


def _blosc_snappy_frame(data, ts, shuffle, blocksize, split, rng):
    nbytes = len(data)
    nblk = -(-nbytes // blocksize)
    left = nbytes % blocksize
    flags = (1 if shuffle else 0) | (0 if split else 0x10) | (2 << 5)
    body, starts = bytearray(), []
    hdr_len = 16 + 4 * nblk
    for b in range(nblk):
        src = data[b * blocksize:(b + 1) * blocksize]
        bsize = len(src)
        if shuffle and ts > 1:  # c-blosc shuffle: byte i of element j -> i * neb + j; the tail as is
            neb = bsize // ts
            a = np.frombuffer(src[:neb * ts], np.uint8).reshape(neb, ts).T.reshape(-1).tobytes()
            src = a + src[neb * ts:]
        nsplit = ts if (split and not (left and b == nblk - 1)) else 1
        ne = bsize // nsplit
        starts.append(hdr_len + len(body))
        for j in range(nsplit):
            part = src[j * ne:(j + 1) * ne]
            z = _snappy_compress(part, rng)
            if len(z) >= ne:
                z = part  # stored
            body += len(z).to_bytes(4, "little") + z
    cbytes = hdr_len + len(body)
    hdr = bytes([2, 1, flags, ts]) + nbytes.to_bytes(4, "little") + blocksize.to_bytes(4, "little") + \
        cbytes.to_bytes(4, "little")
    return hdr + b"".join(s.to_bytes(4, "little") for s in starts) + bytes(body)


# ---- one token list in all three formats: ops = [("lit", bytes) | ("match", off, ml)] ----
def ops_len(ops):
    return sum(len(o[1]) if o[0] == "lit" else o[2] for o in ops)


def ops_decode(ops):
    out = bytearray()
    for o in ops:
        if o[0] == "lit":
            out += o[1]
        else:
            _, off, ml = o
            assert 1 <= off <= len(out)
            for _ in range(ml):
                out.append(out[-off])
    return bytes(out)


def enc_lz4(ops, w=None):
    w = w or Lz4W()
    lits = b""
    for o in ops:
        if o[0] == "lit":
            lits += o[1]
        else:
            w.seq(lits, o[1], o[2])
            lits = b""
    w.seq(lits)
    return w


def enc_blz(ops, w=None):
    w = w or BlzW()
    assert ops[0][0] == "lit"
    for o in ops:
        if o[0] == "lit":
            w.lits(o[1])
        else:
            w.match(o[1], o[2])
    return w


def enc_snappy(ops, w=None, forms=None):
    w = w or SnW().preamble(ops_len(ops))
    for o in ops:
        if o[0] == "lit":
            w.literal(o[1])
        else:
            _, off, ml = o
            while ml:  # copies hold at most 64 bytes; the pieces keep the distance
                m = min(ml, 64)
                w.copy(off, m, 2 if (forms is None and off < 65536) else (forms or 3))
                ml -= m
    return w


ENC = {"lz4": enc_lz4, "blosclz": enc_blz, "snappy": enc_snappy}


def pad_ops(ops, size, seed=99):
    """ops + one offset-1 match up to `size` - TAIL, then TAIL literals (c-blosc's LZ4 wants the last 5
    bytes, and a match's start 12 from the end, as literals; blosclz a literal run at the end)."""
    n = ops_len(ops)
    assert 1 <= n and size - TAIL - n >= 4, (n, size)
    return list(ops) + [("match", 1, size - TAIL - n), ("lit", rnd(TAIL, seed))]


def prefix_ops(n, seed=7):
    """n bytes of output from 251 literals and one match (a prime period: a copy that reads a wrong
    place shows)."""
    assert n >= 251 + 4
    return [("lit", rnd(251, seed)), ("match", 251, n - 251)]


# ---------------------------------------------------------------------------------------------
# reference executors: ("ok", bytes) or ("corrupt", position in the stream)
# ---------------------------------------------------------------------------------------------
class _Bad(Exception):
    pass


def _run(fn, z, cap):
    try:
        return OK, fn(bytes(z), cap)
    except _Bad as e:
        return CORRUPT, e.args[0]


def _copy(out, off, ml, cap, ip):
    if off == 0 or off > len(out) or len(out) + ml > cap:
        raise _Bad(ip)
    for _ in range(ml):
        out.append(out[-off])


def _lz4(z, cap, trace=None):
    """trace (a list): gets ("lit", length, extension bytes) / ("match", length, offset, extension
    bytes) per element, for tests/encoded_inspect.py; the return value is the same with or without."""
    out, ip, n = bytearray(), 0, len(z)
    while True:
        if ip >= n:
            raise _Bad(ip)  # a block ends with a literals-only sequence
        tok = z[ip]
        ip += 1
        ll = tok >> 4
        ip0 = ip
        if ll == 15:
            while True:
                if ip >= n:
                    raise _Bad(ip)
                b = z[ip]
                ip += 1
                ll += b
                if b != 255:
                    break
        if ip + ll > n or len(out) + ll > cap:
            raise _Bad(ip)
        if trace is not None and (ll or ip + ll == n):
            trace.append(("lit", ll, ip - ip0))
        out += z[ip:ip + ll]
        ip += ll
        if ip == n:
            return bytes(out)
        if ip + 2 > n:
            raise _Bad(ip)
        off = z[ip] | (z[ip + 1] << 8)
        ip += 2
        ml = tok & 15
        ip0 = ip
        if ml == 15:
            while True:
                if ip >= n:
                    raise _Bad(ip)
                b = z[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        if trace is not None:
            trace.append(("match", ml + 4, off, ip - ip0))
        _copy(out, off, ml + 4, cap, ip)


def _blosclz(z, cap, trace=None):
    """blosclz_decompress of c-blosc 1.21 restated, but a match at the very end of the stream is
    copied (c-blosc leaves its loop before the copy; only a far match can sit there). trace: as _lz4's,
    the form of a literal run "run", of a match ("near" | "far", length extension bytes)."""
    out, n = bytearray(), len(z)
    if n == 0:
        raise _Bad(0)
    ctrl, ip = z[0] & 31, 1
    while True:
        if ctrl >= 32:
            ln, ofs = (ctrl >> 5) - 1, (ctrl & 31) << 8
            ip0, far = ip, False
            if ln == 6:
                while True:
                    if ip + 1 >= n:
                        raise _Bad(ip)
                    code = z[ip]
                    ip += 1
                    ln += code
                    if code != 255:
                        break
            elif ip + 1 >= n:
                raise _Bad(ip)
            code = z[ip]
            ip += 1
            next_ = ip - ip0 - 1
            ln += 3
            dist = ofs + code + 1
            if code == 255 and ofs == 31 << 8:
                if ip + 1 >= n:
                    raise _Bad(ip)
                dist = (z[ip] << 8) + z[ip + 1] + 8192
                ip += 2
                far = True
            if trace is not None:
                trace.append(("match", ln, dist, ("far" if far else "near", next_)))
            _copy(out, dist, ln, cap, ip)
        else:
            run = ctrl + 1
            if len(out) + run > cap or ip + run > n:
                raise _Bad(ip)
            if trace is not None:
                trace.append(("lit", run, "run"))
            out += z[ip:ip + run]
            ip += run
        if ip >= n:
            return bytes(out)
        ctrl = z[ip]
        ip += 1


def _snappy(z, cap, trace=None):
    """trace: as _lz4's, first ("pre", decoded length, preamble bytes); the form of a literal is its
    length bytes after the tag (0..4), of a copy its tag type (1, 2 or 3)."""
    out, ip, n, want = bytearray(), 0, len(z), 0
    for k in range(6):
        if ip >= n or k == 5:
            raise _Bad(ip)
        b = z[ip]
        ip += 1
        want |= (b & 127) << (7 * k)
        if not b & 128:
            break
    if want > cap or want >= 1 << 32:
        raise _Bad(ip)
    if trace is not None:
        trace.append(("pre", want, ip))
    while ip < n:
        tag = z[ip]
        ip += 1
        if tag & 3 == 0:
            ln = (tag >> 2) + 1
            nb = 0
            if ln > 60:
                nb = ln - 60
                if ip + nb > n:
                    raise _Bad(ip)
                ln = int.from_bytes(z[ip:ip + nb], "little") + 1
                ip += nb
            if ip + ln > n or len(out) + ln > want:
                raise _Bad(ip)
            if trace is not None:
                trace.append(("lit", ln, nb))
            out += z[ip:ip + ln]
            ip += ln
        else:
            form = tag & 3
            nb = {1: 1, 2: 2, 3: 4}[form]
            if ip + nb > n:
                raise _Bad(ip)
            if form == 1:
                ln, off = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | z[ip]
            else:
                ln, off = 1 + (tag >> 2), int.from_bytes(z[ip:ip + nb], "little")
            ip += nb
            if trace is not None:
                trace.append(("match", ln, off, form))
            _copy(out, off, ln, want, ip)
    if len(out) != want:
        raise _Bad(ip)
    return bytes(out)


def execute(fmt, z, cap=1 << 31):
    return _run({"lz4": _lz4, "blosclz": _blosclz, "snappy": _snappy}[fmt], z, cap)


# ---------------------------------------------------------------------------------------------
# model of LzG (blosc.hip): the accounting of one stream at address residue r, G lanes
# ---------------------------------------------------------------------------------------------
@dataclass
class Trace:
    r: int
    G: int
    fills: list = field(default_factory=list)    # {p, kind, wo, partial_first, partial_last}
    lits: list = field(default_factory=list)     # {ip, n, hbm, first_hbm}
    matches: list = field(default_factory=list)  # {op, off, ml, path, fence, overlap, passes, wrap, src_end}
    err: bool = False
    out: bytes = b""

    def refills(self, kind=None, p=None):
        return [f for f in self.fills[1:] if (kind is None or f["kind"] == kind) and (p is None or f["p"] == p)]

    def m(self, **kw):
        return [m for m in self.matches if all(m[k] == v for k, v in kw.items())]


class LzG:
    def __init__(self, z, r, G, cap):
        self.z, self.cs, self.r, self.G, self.cap = bytes(z), len(z), r, G, cap
        self.wo, self.safe, self.out = 0, 0, bytearray()
        self.t = Trace(r, G)

    def fill(self, p, kind):
        a = (self.r + p) & ~15
        self.wo = a - self.r
        end = self.r + self.cs  # the stream's end as an address offset from its 16-B aligned base
        self.t.fills.append({"p": p, "kind": kind, "wo": self.wo, "partial_first": self.wo < 0,
                             "partial_last": end % 16 != 0 and a <= end - end % 16 < a + LZW})

    def rd(self, p, kind):
        assert 0 <= p < self.cs, f"the kernel would read stream byte {p} of {self.cs}"
        if not 0 <= p - self.wo < LZW:
            self.fill(p, kind)
        return self.z[p]

    def lits(self, ip, n):
        assert ip + n <= self.cs
        hbm = [q for q in range(ip, ip + n) if q - self.wo >= LZW]
        self.t.lits.append({"ip": ip, "n": n, "hbm": len(hbm), "first_hbm": hbm[0] if hbm else None})
        self.out += self.z[ip:ip + n]

    def match(self, off, ml):
        op = len(self.out)
        rec = {"op": op, "off": off, "ml": ml, "overlap": off < ml, "passes": -(-ml // self.G),
               "src_end": op - off + min(off, ml), "fence": None}
        if off + ml <= LZR:
            rec["path"] = "ring"
            rec["wrap"] = (op & LZRM) + ml > LZR or ((op - off) & LZRM) + min(off, ml) > LZR
        else:
            rec["path"] = "far"
            rec["wrap"] = (op & LZRM) + ml > LZR
            rec["fence"] = rec["src_end"] > self.safe
            if rec["fence"]:
                self.safe = op
        self.t.matches.append(rec)
        for _ in range(ml):
            self.out.append(self.out[-off])


def _m_lz4(L):
    ip, cs, cap = 0, L.cs, L.cap
    while True:
        tok = L.rd(ip, "token")
        ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                if ip >= cs:
                    return True
                b = L.rd(ip, "ll_ext")
                ip += 1
                ll += b
                if b != 255:
                    break
        if ll > cs - ip or ll > cap - len(L.out):
            return True
        L.lits(ip, ll)
        ip += ll
        if ip == cs:
            return False
        if cs - ip < 2:
            return True
        off = L.rd(ip, "off_lo") | (L.rd(ip + 1, "off_hi") << 8)
        ip += 2
        ml = tok & 15
        if off == 0 or off > len(L.out):
            return True
        if ml == 15:
            while True:
                if ip >= cs:
                    return True
                b = L.rd(ip, "ml_ext")
                ip += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if ml > cap - len(L.out) or ip >= cs:
            return True
        L.match(off, ml)


def _m_blosclz(L):
    cs, cap = L.cs, L.cap
    ctrl, ip = L.rd(0, "ctrl") & 31, 1
    while True:
        if ctrl >= 32:
            ln, ofs = (ctrl >> 5) - 1, (ctrl & 31) << 8
            if ln == 6:
                while True:
                    if cs - ip <= 1:
                        return True
                    code = L.rd(ip, "len_ext")
                    ip += 1
                    ln += code
                    if code != 255:
                        break
            elif cs - ip <= 1:
                return True
            code = L.rd(ip, "dist")
            ip += 1
            ln += 3
            dist = ofs + code + 1
            if code == 255 and ofs == 31 << 8:
                if cs - ip <= 1:
                    return True
                dist = (L.rd(ip, "far_hi") << 8) + L.rd(ip + 1, "far_lo") + 8192
                ip += 2
            if ln > cap - len(L.out) or dist > len(L.out):
                return True
            L.match(dist, ln)
        else:
            run = ctrl + 1
            if run > cap - len(L.out) or run > cs - ip:
                return True
            L.lits(ip, run)
            ip += run
        if ip >= cs:
            return False
        ctrl = L.rd(ip, "ctrl")
        ip += 1


def _m_snappy(L):
    cs, cap, ip, want = L.cs, L.cap, 0, 0
    k = 0
    while True:
        if ip >= cs or k == 5:
            return True
        b = L.rd(ip, "pre")
        ip += 1
        want |= (b & 127) << (7 * k)
        if not b & 128:
            break
        k += 1
    if want > cap:
        return True
    while ip < cs:
        tag = L.rd(ip, "tag")
        ip += 1
        if tag & 3 == 0:
            ln = (tag >> 2) + 1
            if ln > 60:
                nb = ln - 60
                if nb > cs - ip:
                    return True
                ln = sum(L.rd(ip + q, f"len_b{q}") << (8 * q) for q in range(nb)) + 1
                ip += nb
            if ln > cs - ip or ln > want - len(L.out):
                return True
            L.lits(ip, ln)
            ip += ln
        else:
            form = tag & 3
            nb = {1: 1, 2: 2, 3: 4}[form]
            if cs - ip < nb:
                return True
            if form == 1:
                ln, off = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | L.rd(ip, "off1")
            else:
                ln = 1 + (tag >> 2)
                off = sum(L.rd(ip + q, f"off{nb}_{q}") << (8 * q) for q in range(nb))
            ip += nb
            if off == 0 or off > len(L.out) or ln > want - len(L.out):
                return True
            L.match(off, ln)
    return len(L.out) != want


def model(fmt, z, r, G=G_NARROW, cap=1 << 31):
    """The trace of k_lz4m / k_blosclzm / k_snappym<G> on stream z at address residue r."""
    L = LzG(z, r, G, cap)
    if L.cs == 0:
        L.t.err = True
        return L.t
    L.fill(0, "start")
    L.t.err = bool({"lz4": _m_lz4, "blosclz": _m_blosclz, "snappy": _m_snappy}[fmt](L))
    L.t.out = bytes(L.out)
    return L.t


# ---------------------------------------------------------------------------------------------
# shuffle / bitshuffle (c-blosc shuffle.c; format 2: bitshuffle only when elements % 8 == 0)
# ---------------------------------------------------------------------------------------------
def shuffle(block, ts):
    n = len(block) // ts
    a = np.frombuffer(block[:n * ts], np.uint8).reshape(n, ts).T.reshape(-1).tobytes()
    return a + block[n * ts:]


def unshuffle(block, ts):
    n = len(block) // ts
    a = np.frombuffer(block[:n * ts], np.uint8).reshape(ts, n).T.reshape(-1).tobytes()
    return a + block[n * ts:]


def bitshuffle(block, ts):
    n = len(block) // ts
    if n % 8 or len(block) < ts:
        return bytes(block)
    a = np.frombuffer(block[:n * ts], np.uint8).reshape(n, ts)
    bits = np.unpackbits(a, axis=1, bitorder="little")  # [element, 8 * byte + bit]
    return np.packbits(bits.T, axis=1, bitorder="little").tobytes() + block[n * ts:]


def bitunshuffle(block, ts):
    n = len(block) // ts
    if n % 8 or len(block) < ts:
        return bytes(block)
    rows = np.frombuffer(block[:n * ts], np.uint8).reshape(8 * ts, n // 8)
    bits = np.unpackbits(rows, axis=1, bitorder="little")  # [8 * byte + bit, element]
    return np.packbits(bits.T, axis=1, bitorder="little").tobytes() + block[n * ts:]


def filtered(block, ts, mode):
    """The bytes c-blosc compresses for a block: mode 0 none, 1 shuffle, 2 bitshuffle."""
    if mode == 1 and ts > 1:
        return shuffle(block, ts)
    if mode == 2:
        return bitshuffle(block, ts)
    return bytes(block)


def unfiltered(block, ts, mode):
    if mode == 1 and ts > 1:
        return unshuffle(block, ts)
    if mode == 2:
        return bitunshuffle(block, ts)
    return bytes(block)


# ---------------------------------------------------------------------------------------------
# frame assembler
# ---------------------------------------------------------------------------------------------
@dataclass
class S:
    """One split's stream: payload bytes, the split's decoded size, stored or compressed."""
    payload: bytes
    ne: int
    stored: bool = False
    csize: int = None  # the size field, when it is to differ from len(payload)


@dataclass
class Frame:
    data: bytes
    payload_off: list  # [block][split] -> offset of the payload in the frame


def header(version=2, versionlz=1, flags=0, typesize=1, nbytes=0, blocksize=0, cbytes=0):
    return bytes([version, versionlz, flags, typesize]) + b"".join(
        (v & 0xFFFFFFFF).to_bytes(4, "little") for v in (nbytes, blocksize, cbytes))


def assemble(blocks, *, comp, typesize, nbytes, blocksize, mode=0, split=False, memcpy=False, version=2,
             versionlz=1, flags=None, order=None, pads=None, trailing=b"", cbytes=None, bstarts=None,
             nblocks=None):
    """A c-blosc 1.x frame of `blocks` ([block][split] -> S). order: the blocks' physical order;
    pads[b]: bytes of padding before block b's first size field; bstarts: {block: value} overrides;
    trailing: bytes after the frame (counted in cbytes only when cbytes is given so)."""
    if flags is None:
        flags = (1 if mode == 1 else 4 if mode == 2 else 0) | (0 if split else 0x10) | (comp << 5) | (2 if memcpy else 0)
    if memcpy:
        body = b"".join(s.payload for b in blocks for s in b)
        cb = 16 + len(body) if cbytes is None else cbytes
        return Frame(header(version, versionlz, flags, typesize, nbytes, blocksize, cb) + body + trailing, [[16]])
    nb = len(blocks) if nblocks is None else nblocks
    hdr_len = 16 + 4 * nb
    body, starts, offs = bytearray(), {}, {}
    for b in (order if order is not None else range(len(blocks))):
        body += b"\xEE" * ((pads or {}).get(b, 0))
        starts[b] = hdr_len + len(body)
        offs[b] = []
        for s in blocks[b]:
            assert s.stored == (len(s.payload) == s.ne) or s.csize is not None, \
                "csize == ne means stored, to c-blosc and to k_blosc_streams"
            cs = len(s.payload) if s.csize is None else s.csize
            body += (cs & 0xFFFFFFFF).to_bytes(4, "little")
            offs[b].append(hdr_len + len(body))
            body += s.payload
    starts.update(bstarts or {})
    cb = hdr_len + len(body) if cbytes is None else cbytes
    tab = b"".join((starts[b] & 0xFFFFFFFF).to_bytes(4, "little") for b in range(len(blocks)))
    tab = tab[:4 * nb].ljust(4 * nb, b"\0")
    return Frame(header(version, versionlz, flags, typesize, nbytes, blocksize, cb) + tab + bytes(body) + trailing,
                 [offs[b] for b in range(len(blocks))])


def count_streams(frame):
    """The entries a frame takes in the stream table (k_blosc_info's nsub)."""
    flags, ts = frame[2], frame[3]
    nbytes, bs = int.from_bytes(frame[4:8], "little"), int.from_bytes(frame[8:12], "little")
    if flags & 2 or not nbytes:
        return 1 if nbytes else 0
    nfull, lo = divmod(nbytes, bs)
    return nfull * (ts if cblosc_splits(not flags & 0x10, ts, bs) else 1) + (1 if lo else 0)


def one_block(fmt, stream, size, wide=False, pad=0, stored=False):
    """The frame of one unsplit block holding `stream`; wide: the bitshuffle flag (typesize 1), which
    sends the stream to the one-stream-per-wave kernel."""
    return assemble([[S(stream, size, stored)]], comp=COMP[fmt], typesize=1, nbytes=size, blocksize=size,
                    mode=2 if wide else 0, pads={0: pad})


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
@dataclass
class Case:
    id: str
    family: str
    size: int
    status: str = OK
    fmt: str = None
    stream: object = None         # r -> stream bytes (a stream case), else None
    residues: tuple = (0,)
    intent: list = field(default_factory=list)  # (text, predicate over the model's Trace)
    frame_fn: object = None       # a frame case: () -> Frame
    expect_bytes: bytes = None    # a frame case's chunk bytes
    cap: int = None               # the decoders' output bound for this case's stream (default: size)
    ne: int = None                # a stream case whose block is smaller than the chunk (two blocks)
    gpu_accepts: bool = None      # lenient cases: what the GPU does (asserted once known)
    cblosc_unspecified: bool = False  # a lenient case the other way round: c-blosc returns unspecified bytes
    why: str = ""
    same_trace_as: str = None     # a case whose trace equals another's on purpose (the reason beside it)

    @property
    def is_stream(self):
        return self.stream is not None

    def executed(self, r=0):
        return execute(self.fmt, self.stream(r), self.cap or self.size)

    def frame(self, r=0, wide=False):
        """The case's frame; a stream case's payload sits at offset 24 (residue: the caller's base)."""
        if not self.is_stream:
            return self.frame_fn()
        z = self.stream(r)
        if self.ne is None:
            return one_block(self.fmt, z, self.size, wide)
        # two blocks of ne bytes: the case's stream, then a stored block
        assert 2 * self.ne == self.size
        return assemble([[S(z, self.ne)], [S(rnd(self.ne, 5), self.ne, True)]], comp=COMP[self.fmt], typesize=1,
                        nbytes=self.size, blocksize=self.ne, mode=2 if wide else 0)

    def expect(self, r=0, wide=False):
        if not self.is_stream:
            return self.expect_bytes
        st, out = self.executed(r)
        assert st == OK, (self.id, st, out)
        if self.ne is not None:
            out = out + rnd(self.ne, 5)
            return b"".join(unfiltered(out[i:i + self.ne], 1, 2 if wide else 0) for i in (0, self.ne))
        return unfiltered(out, 1, 2 if wide else 0)


PAYLOAD_OFF = 24  # of a one-block frame's stream: header 16, one bstart, one size field


def _stream_case(cid, fam, fmt, size, ops=None, w=None, **kw):
    """A case from a token list (padded to `size`) or from a finished writer."""
    if ops is not None:
        z = ENC[fmt](pad_ops(ops, size)).bytes()
    else:
        z = w.bytes()
    return Case(cid, fam, size, fmt=fmt, stream=lambda r, z=z: z, **kw)


FMTS = ("lz4", "blosclz", "snappy")


def _fits(fmt, ops):
    """Can the format express this token list with the same matches? (blosclz: match >= 3, distance
    <= 8191 + 65536, starts with a literal; lz4: match >= 4, distance <= 65535; snappy splits long copies)."""
    for o in ops:
        if o[0] != "match":
            continue
        _, off, ml = o
        if fmt == "lz4" and (ml < 4 or off > 65535):
            return False
        if fmt == "blosclz" and (ml < 3 or off > 8192 + 65535):
            return False
    return not (fmt == "blosclz" and ops[0][0] != "lit")


# ---- window ---------------------------------------------------------------------------------
def _place(build, kind, P):
    """build(L, v) -> writer whose target sequence follows L filler literals (v: a variant of the
    filler's layout): the writer that puts the last byte of field `kind` at stream position P."""
    lo, hi = 0, P + 1
    while lo < hi:  # the position grows with L
        mid = (lo + hi) // 2
        if build(mid, 0).last(kind) < P:
            lo = mid + 1
        else:
            hi = mid
    for L in range(max(0, lo - 3), lo + 1):
        for v in (0, 1):
            w = build(L, v)
            if w.last(kind) == P:
                return w
    raise AssertionError(f"no filler puts {kind} at {P}")


def _lz4_probe(L, v=0):
    w = Lz4W()
    w.seq(rnd(max(L, 1), 3), 1, 8)
    w.seq(rnd(20, 4), 7, 30)  # token, ll extension, 20 literals, offset, ml extension
    return w


def _blz_probe(L, v=0):
    w = BlzW().lit(b"\x11").match(1, 8400)
    if v:  # one more control byte: the runs of 32 alone skip every 33rd position
        w.lit(b"\x22")
    w.lits(rnd(max(L, 1), 3))
    w.match(8192 + 300, 12)   # control, length extension, distance byte 255, two far bytes
    return w


def _sn_probe(L, v=0, size=8192):
    w = SnW().preamble(size)
    w.literal(rnd(max(L, 1), 3))
    w.literal(rnd(70, 4), width=4)
    w.copy(9, 8, 1).copy(300, 20, 2).copy(77, 30, 3)
    return w


def _finish_stream(fmt, w, size):
    """Pad the writer's stream (it ends on a match, or snappy anywhere) to `size` decoded bytes."""
    n = w.n
    assert size - TAIL - n >= 4, (n, size)
    if fmt == "lz4":
        w.seq(b"", 1, size - TAIL - n)
        w.seq(rnd(TAIL, 99))
    elif fmt == "blosclz":
        w.match(1, size - TAIL - n).lits(rnd(TAIL, 99))
    else:
        enc_snappy([("match", 1, size - TAIL - n), ("lit", rnd(TAIL, 99))], w)
    return w


_PROBES = {
    "lz4": (_lz4_probe, 8192, ["token", "ll_ext", "off_lo", "off_hi", "ml_ext"]),
    "blosclz": (_blz_probe, 16384, ["ctrl", "len_ext", "dist", "far_hi", "far_lo"]),
    "snappy": (_sn_probe, 8192, ["tag", "len_b0", "len_b1", "len_b2", "len_b3", "off1", "off2_0", "off2_1",
                                 "off4_0", "off4_1", "off4_2", "off4_3"]),
}
# a refill by this field straddles a multi-byte field (its earlier bytes came from the window before)
_STRADDLE = {"off_hi", "far_lo", "len_b1", "len_b2", "len_b3", "off2_1", "off4_1", "off4_2", "off4_3"}
ALL_R = tuple(range(16))


def _window_stream(fmt, kind, r, dp=0):
    build, size, _ = _PROBES[fmt]
    if fmt == "snappy":
        build = functools.partial(_sn_probe, size=size)
    return _finish_stream(fmt, _place(build, kind, LZW - r + dp), size).bytes()


def _window():
    out = []
    for fmt, (build, size, kinds) in _PROBES.items():
        for i, kind in enumerate(kinds):
            rs = ALL_R if i in (0, 3) else (0, 1, 15)  # all residues: the first field and one multi-byte field's tail
            out.append(Case(f"window_{fmt}_{kind}", "window", size, fmt=fmt, residues=rs,
                            stream=functools.lru_cache(None)(lambda r, fmt=fmt, kind=kind: _window_stream(fmt, kind, r)),
                            intent=[(f"the read of {kind} at LZW - r is the first refill" +
                                     (", in the middle of its field" if kind in _STRADDLE else ""),
                                     lambda t, kind=kind: t.fills[1]["kind"] == kind and t.fills[1]["p"] == LZW - t.r)]))
    # literals are not read through rd: a literal past the window comes from HBM (the other branch of lits)
    for fmt in ("lz4", "snappy"):
        for name, kind, dp, hbm in (("first_literal", "lit0", 0, 20), ("last_literal", "litN", 0, 1),
                                    ("run_starts_on_last_window_byte", "lit0", -1, 19)):
            n_l = 70 if fmt == "snappy" else 20
            hb = hbm if hbm == 1 else n_l - (20 - hbm)
            out.append(Case(f"window_{fmt}_{name}", "window", 8192, fmt=fmt, residues=(0, 1, 15),
                            stream=functools.lru_cache(None)(lambda r, fmt=fmt, kind=kind, dp=dp: _window_stream(fmt, kind, r, dp)),
                            intent=[(f"{hb} of the run's {n_l} literals come from HBM, the first at LZW - r + {max(dp, 0) if kind == 'lit0' else 0}",
                                     lambda t, hb=hb, n_l=n_l: any(x["n"] == n_l and x["hbm"] == hb for x in t.lits))]))
        for name, n in (("run_over_one_window", LZW + 77), ("run_over_two_windows", 2 * LZW + 77)):
            ops = [("lit", rnd(5, 2)), ("match", 2, 9), ("lit", rnd(n, 6)), ("match", 1000, 40)]
            out.append(_stream_case(f"window_{fmt}_{name}", "window", fmt, 8192, ops, residues=(0, 1, 15),
                                    intent=[(f"a literal run of {n} with at least {n - LZW} bytes from HBM, then a refill",
                                             lambda t, n=n: any(x["n"] >= n - 1200 and x["hbm"] >= n - LZW for x in t.lits) and len(t.fills) >= 2)]))
    out.append(Case("window_blosclz_literal_runs_are_32", "window", 8192, fmt="blosclz", residues=(0,),
                    stream=lambda r: enc_blz(pad_ops([("lit", rnd(32, 1)), ("lit", rnd(1, 2))], 8192)).bytes(),
                    intent=[("runs of 32 and 1 literals (a blosclz run is at most 32: none spans a window)",
                             lambda t: [x["n"] for x in t.lits[:2]] == [32, 1])]))
    return out


# ---- tiny blocks: streams shorter than 16 bytes, every residue, large stream tables ---------
def small_stream(fmt, ne, seed):
    """A stream of 11-13 bytes (ne 16; a few more for larger ne) decoding to ne >= 13 bytes."""
    a, b, ml = rnd(4, seed), rnd(5, seed + 1000), ne - 9
    dec = a + a[-1:] * ml + b
    if fmt == "lz4":
        return Lz4W().seq(a, 1, ml).seq(b).bytes(), dec
    if fmt == "blosclz":
        return BlzW().lit(a).match(1, ml).lit(b).bytes(), dec
    return enc_snappy([("match", 1, ml), ("lit", b)], SnW().preamble(ne).literal(a)).bytes(), dec


def cblosc_splits(split_flag, ts, bs):
    """c-blosc 1.21 blosc_d: a block is split only when the flag allows it and typesize <= 16
    (MAX_SPLITS) and blocksize / typesize >= 128 (MIN_BUFFERSIZE); the leftover block never is."""
    return bool(split_flag) and ts <= 16 and bs // ts >= 128


def grid_frame(fmt, nbytes, bs, ts, split, stored=lambda k: False, mode=0, seed=0):
    """Blocks of bs bytes, every stream small_stream or stored (stored(k), or too small to compress);
    `split` is the header's flag, the layout follows c-blosc's rule. Returns (Frame, chunk bytes,
    number of streams)."""
    ns_full = ts if cblosc_splits(split, ts, bs) else 1
    blocks, chunk, k = [], b"", 0
    nfull, lo = divmod(nbytes, bs)
    for b in range(nfull + (1 if lo else 0)):
        left = b == nfull
        ns = 1 if left else ns_full
        ne = (lo if left else bs) // ns
        bl, dec = [], b""
        for j in range(ns):
            if ne < 13 or stored(k):
                d = rnd(ne, seed * 7919 + k)
                bl.append(S(d, ne, True))
            else:
                z, d = small_stream(fmt, ne, seed * 7919 + k)
                bl.append(S(z, ne))
            dec += d
            k += 1
        blocks.append(bl)
        chunk += unfiltered(dec, ts, mode)
    f = assemble(blocks, comp=COMP[fmt], typesize=ts, nbytes=nbytes, blocksize=bs, mode=mode, split=split)
    return f, chunk, k


def _frame_case(cid, fam, size, fr, expect, status=OK, **kw):
    return Case(cid, fam, size, status=status, frame_fn=lambda fr=fr: fr, expect_bytes=expect, **kw)


def one_match_ops():
    """Two literals, one match, the final literals: the shortest valid stream of 8192 bytes."""
    return [("lit", rnd(2, 8)), ("match", 1, 8192 - 2 - TAIL), ("lit", rnd(TAIL, 3))]


def many_ops():
    """1300 short matches, each followed by a literal, in 8192 bytes."""
    many = [("lit", rnd(3, 8))]
    for i in range(1300):
        many += [("match", 1 + i % 3, 4 + i % 2), ("lit", bytes([1 + i % 200]))]
    return many + [("lit", rnd(8192 - ops_len(many), 9))]


def _pairs():
    out = []
    for fmt in FMTS:
        # 512 streams shorter than 16 bytes; their 15- or 17-byte records walk through every address residue
        f, chunk, k = grid_frame(fmt, 8192, 16, 1, False)
        assert k == 512 and {o[0] % 16 for o in f.payload_off} == set(range(16))
        out.append(_frame_case(f"pairs_{fmt}_tiny_streams_every_residue", "pairs", 8192, f, chunk,
                               why="the partial first and last vector of fill at every residue"))
        # split blocks whose splits alternate stored and compressed
        f, chunk, k = grid_frame(fmt, 8192, 512, 4, True, stored=lambda k: k % 2 == 1, mode=1, seed=1)
        assert k == 64
        out.append(_frame_case(f"pairs_{fmt}_alternating_stored", "pairs", 8192, f, chunk))
        # thousands of tokens in one stream (beside the family's other, short streams)
        many = many_ops()
        out.append(Case(f"pairs_{fmt}_thousands_of_tokens", "pairs", 8192, fmt=fmt, stream=lambda r, z=ENC[fmt](many).bytes(): z,
                        intent=[("over 1000 matches in one stream", lambda t: len(t.matches) > 1000)]))
        out.append(Case(f"pairs_{fmt}_one_match", "pairs", 8192, fmt=fmt, stream=lambda r, z=ENC[fmt](one_match_ops()).bytes(): z,
                        intent=[("one match of 8174 bytes (snappy: its pieces of at most 64, 128 of them)",
                                 lambda t, fmt=fmt: {m["off"] for m in t.matches} == {1} and sum(m["ml"] for m in t.matches) == 8174
                                 and len(t.matches) == (128 if fmt == "snappy" else 1))]))
    return out


def pairs_batches():
    """The `pairs` family's batches for the GPU test: name -> (chunk size, [(frame bytes, chunk bytes)],
    stream-table size). Tables of 1023, 1024, 1025 and 2049 streams with stored streams in between
    (k_lz_list compacts in rounds of 1024; blocks of 16 bytes, unsplit: c-blosc splits no block of
    fewer than 128 elements), and every compressor, filter and width in one call with odd counts."""
    n = 8192
    res = {}
    third = lambda k: k % 3 == 1

    def t(fmt, bs, mode, seed):
        f, c, k = grid_frame(fmt, n, bs, 1, False, third, mode, seed)
        return (f.data, c), k
    a512 = [t(f, 16, m, s) for s, (f, m) in enumerate([("lz4", 0), ("blosclz", 2), ("snappy", 0), ("lz4", 2)])]
    a482 = t("blosclz", 17, 0, 9)  # 481 blocks and a leftover block
    assert a482[1] == 482 and all(k == 512 for _, k in a512)
    ops = pad_ops([("lit", rnd(9, 4))], n)
    one = (one_block("lz4", enc_lz4(ops).bytes(), n, wide=True).data, bitunshuffle(ops_decode(ops), 1))
    res["table_1023"] = (n, [a512[0][0], a482[0]] + [one] * 29, 1023)
    res["table_1024"] = (n, [a512[0][0], a512[1][0]], 1024)
    res["table_1025"] = (n, [a512[1][0], one, a512[2][0]], 1025)
    res["table_2049"] = (n, [x[0] for x in a512] + [one], 2049)
    mix = []
    for i, fmt in enumerate(FMTS):
        ops = pad_ops(prefix_ops(300 + i, seed=i), n)
        z, d = ENC[fmt](ops).bytes(), ops_decode(ops)
        mix.append((one_block(fmt, z, n).data, d))
        mix.append((one_block(fmt, z, n, wide=True).data, bitunshuffle(d, 1)))
        f, c, _ = grid_frame(fmt, n, 1024, 2, True, third, 1, 20 + i)
        mix.append((f.data, c))
        f, c, _ = grid_frame(fmt, n, 1000, 2, False, third, 2, 30 + i)  # 9 streams: an odd count
        mix.append((f.data, c))
    res["mixed_compressors_and_widths"] = (n, mix, None)
    # per compressor three one-stream frames, so each compacted list is [one match, 1300 matches, one match]:
    # the first wave pairs the one-token stream with the long one, the second wave's other half is idle
    un = []
    for fmt in FMTS:
        for ops in (one_match_ops(), many_ops(), one_match_ops()):
            un.append((one_block(fmt, ENC[fmt](ops).bytes(), n).data, ops_decode(ops)))
    res["one_token_beside_thousands_odd_count"] = (n, un, 9)
    return res


# ---- ring -----------------------------------------------------------------------------------
def _ring():
    out = []

    def add(name, size, ops, intent, fmts=FMTS, **kw):
        for fmt in fmts:
            if _fits(fmt, ops):
                out.append(_stream_case(f"ring_{fmt}_{name}", "ring", fmt, size, ops, intent=intent, **kw))

    ML = 40
    for d in (-1, 0, 1):
        off = LZR - ML + d
        add(f"off_plus_ml_LZR{d:+d}", 8192, prefix_ops(4300) + [("match", off, ML), ("lit", rnd(3, 1))],
            [(f"a match of {ML} at distance {off}: the {'ring' if d <= 0 else 'far'} path",
              lambda t, off=off, d=d: t.m(off=off, ml=ML, path="ring" if d <= 0 else "far"))])
    for g in (G_NARROW, G_WIDE):
        for d in (-1, 0, 1):
            ml = g + d
            for oname, off in (("far_apart", 100), ("overlapping", 5)):
                add(f"ml_G{g}{d:+d}_{oname}", 8192, prefix_ops(300) + [("match", off, ml), ("lit", rnd(3, 1))],
                    [(f"a ring match of {ml} bytes: {-(-ml // g)} pass(es) over {g} lanes",
                      lambda t, off=off, ml=ml, g=g: t.m(off=off, ml=ml, path="ring") and
                      (t.G != g or t.m(off=off, ml=ml)[0]["passes"] == (1 if ml <= g else 2)))],
                    fmts=FMTS if ml <= 64 else ("lz4", "blosclz"))
    add("write_wraps_ring", 8192, prefix_ops(LZR - 10) + [("match", 333, ML), ("lit", rnd(3, 1))],
        [("the copy's ring writes wrap the ring index", lambda t: t.m(off=333, ml=ML, path="ring", wrap=True))])
    add("source_wraps_ring", 8192, prefix_ops(LZR + 20) + [("match", ML, ML), ("lit", rnd(3, 1))],
        [("the copy's ring source wraps the ring index", lambda t: t.m(off=ML, ml=ML, path="ring", wrap=True))])
    for oname, off in (("1", 1), ("2", 2), ("3", 3), ("ml-1", ML - 1), ("ml", ML), ("ml+1", ML + 1)):
        add(f"off_{oname}", 8192, prefix_ops(300) + [("match", off, ML), ("lit", rnd(3, 1))],
            [(f"distance {off} against length {ML}: {'overlapping' if off < ML else 'disjoint'}",
              lambda t, off=off: t.m(off=off, ml=ML, overlap=off < ML))])
    add("off_equals_op", 8192, prefix_ops(700) + [("match", 700, ML), ("lit", rnd(3, 1))],
        [("a match from output byte 0", lambda t: t.m(op=700, off=700))])
    add("far_source_ends_at_op", 16384, prefix_ops(300) + [("lit", rnd(90, 4)), ("match", 100, 5000), ("lit", rnd(3, 1))],
        [("a far match whose source ends at op: the fence is taken",
          lambda t: any(m["path"] == "far" and m["fence"] and m["src_end"] == m["op"] and m["off"] == 100 for m in t.matches))],
        fmts=("lz4", "blosclz"))
    # snappy: copies hold 64 bytes, so a far copy (off + 64 > LZR) never overlaps; its source can still end at op - off + 64
    add("far_overlapping", 16384, prefix_ops(2500) + [("match", 2100, 5000), ("lit", rnd(3, 1))],
        [("a far overlapping match (distance 2100, 5000 bytes)", lambda t: t.m(off=2100, ml=5000, path="far", overlap=True))],
        fmts=("lz4", "blosclz"))
    add("far_far_below_safe_then_above", 16384,
        prefix_ops(4500) + [("match", 4050, 100), ("match", 4300, 100), ("match", 150, 4000), ("lit", rnd(3, 1))],
        [("far with fence, far below safe without, far above safe with",
          lambda t: [(m["path"], m["fence"]) for m in t.matches if (m["off"], m["ml"]) in ((4050, 100), (4300, 100), (150, 4000))]
          == [("far", True), ("far", False), ("far", True)])], fmts=("lz4", "blosclz"))
    add("far_far_below_safe_then_above_64", 16384,
        prefix_ops(4500) + [("match", 4050, 64), ("match", 4300, 64), ("match", 251, 4000), ("match", 4033, 64), ("lit", rnd(3, 1))],
        [("far copies of 64: fence, none (below safe), fence again (its source was written after the first)",
          lambda t: [(m["path"], m["fence"]) for m in t.matches if (m["off"], m["ml"]) in ((4050, 64), (4300, 64), (4033, 64))]
          == [("far", True), ("far", False), ("far", True)])], fmts=("snappy",))
    big = 131072
    add("lz4_max_distance", big, prefix_ops(66000) + [("match", 65535, 50), ("lit", rnd(3, 1))],
        [("distance 65535", lambda t: t.m(off=65535, ml=50))], fmts=("lz4", "snappy"))
    for name, dist in (("near_8191", 8191), ("far_value_0", 8192), ("far_max", 8192 + 65535), ("code_255_ordinary", (5 << 8) + 256)):
        add(f"distance_{name}", big, prefix_ops(74000) + [("match", dist, 50), ("lit", rnd(3, 1))],
            [(f"distance {dist}", lambda t, dist=dist: t.m(off=dist, ml=50))], fmts=("blosclz",))
    for name, off, form in (("form1_2047", 2047, 1), ("form2_65535", 65535, 2), ("form3_65536", 65536, 3), ("form3_70001", 70001, 3),
                            ("form3_small_distance", 9, 3)):
        w = enc_snappy(prefix_ops(74000), SnW().preamble(big))
        w.copy(off, 11, form).literal(rnd(3, 1))
        w = enc_snappy([("match", 1, big - TAIL - 74000 - 14), ("lit", rnd(TAIL, 99))], w)
        out.append(_stream_case(f"ring_snappy_{name}", "ring", "snappy", big, w=w,
                                intent=[(f"a form {form} copy at distance {off}", lambda t, off=off: t.m(off=off, ml=11))]))
    return out


# ---- lengths --------------------------------------------------------------------------------
def _lengths():
    out = []

    def lz4(name, seqs, intent):
        w = Lz4W().seq(rnd(40, 2), 3, 6)
        for a in seqs:
            w.seq(*a)
        out.append(_stream_case(f"lengths_lz4_{name}", "lengths", "lz4", 8192, w=_finish_stream("lz4", w, 8192), intent=intent))

    for ll, ext in ((0, []), (14, []), (15, [0]), (15 + 254, [254]), (15 + 255, [255, 0]), (15 + 510, [255, 255, 0])):
        lz4(f"ll_{ll}", [(rnd(ll, ll + 1), 9, 8, ext if ll >= 15 else None)],
            [(f"a literal run of {ll}: extension bytes {ext}", lambda t, ll=ll: any(x["n"] == ll for x in t.lits))])
    for ml in (4, 18, 19, 273, 274):
        lz4(f"ml_{ml}", [(rnd(2, 3), 9, ml)], [(f"a match of {ml}", lambda t, ml=ml: t.m(off=9, ml=ml))])

    def blz(name, fn, intent, high=0, **kw):
        w = BlzW().lit(rnd(32, 2), high=high)
        fn(w)
        out.append(_stream_case(f"lengths_blosclz_{name}", "lengths", "blosclz", 8192, w=_finish_stream("blosclz", w, 8192),
                                intent=intent, **kw))

    for ml in (3, 4, 5, 6, 7, 8):
        blz(f"ml_{ml}", lambda w, ml=ml: w.match(9, ml).lit(rnd(1, 5)), [(f"a match of {ml}", lambda t, ml=ml: t.m(off=9, ml=ml))])
    blz("ml_9_ext_0", lambda w: w.match(9, 9, ext=[0]).lit(rnd(1, 5)), [("a match of 9: extension byte 0", lambda t: t.m(off=9, ml=9))])
    blz("ml_ext_255_0", lambda w: w.match(9, 9 + 255, ext=[255, 0]).lit(rnd(1, 5)),
        [("extension bytes 255, 0", lambda t: t.m(off=9, ml=264))])
    blz("ml_ext_255_255_7", lambda w: w.match(9, 9 + 517).lit(rnd(1, 5)), [("two full extension bytes", lambda t: t.m(off=9, ml=526))])
    blz("runs_1_and_32", lambda w: w.lit(rnd(1, 6)).match(2, 5).lit(rnd(32, 7)).match(2, 5).lit(rnd(1, 8)),
        [("literal runs of 1 and 32", lambda t: {1, 32} <= {x["n"] for x in t.lits})])
    blz("first_ctrl_high_bits", lambda w: w.match(9, 5).lit(rnd(1, 5)), [("the first control byte's high bits are ignored",
                                                                        lambda t: t.lits[0]["n"] == 32)], high=5,
        same_trace_as="lengths_blosclz_ml_5")  # the same tokens: only the ignored bits of the stream's first byte differ

    def sn(name, fn, intent, pre=None):
        w = SnW().preamble(8192, pre).literal(rnd(40, 2))
        fn(w)
        out.append(_stream_case(f"lengths_snappy_{name}", "lengths", "snappy", 8192, w=_finish_stream("snappy", w, 8192), intent=intent))

    for n, width in ((60, 0), (61, 1), (60, 1), (5, 2), (61, 3), (300, 2), (300, 4), (1, 4)):
        sn(f"literal_{n}_width_{width}", lambda w, n=n, width=width: w.literal(rnd(n, n), width=width),
           [(f"a literal of {n} with {width} length byte(s)", lambda t, n=n: any(x["n"] == n for x in t.lits[1:]))])
    for ln in range(4, 12):
        sn(f"copy1_{ln}", lambda w, ln=ln: w.copy(9, ln, 1), [(f"a form 1 copy of {ln}", lambda t, ln=ln: t.m(off=9, ml=ln))])
    for form in (2, 3):
        for ln in (1, 64):
            sn(f"copy{form}_{ln}", lambda w, ln=ln, form=form: w.copy(9, ln, form),
               [(f"a form {form} copy of {ln}", lambda t, ln=ln: t.m(off=9, ml=ln))])
    sn("preamble_5_bytes", lambda w: w.copy(9, 5, 1), [("a preamble padded to 5 bytes", lambda t: not t.err)], pre=5)
    return out


# ---- shared token lists: the executors agree across formats ----------------------------------
def shared_token_lists():
    """Token lists every format can express (matches of 4..64 bytes), for the executors' agreement."""
    res = []
    for seed in range(6):
        g = np.random.default_rng(seed)
        ops, n = [("lit", rnd(int(g.integers(1, 70)), seed))], 0
        for _ in range(200):
            n = ops_len(ops)
            ops.append(("match", int(g.integers(1, min(n, 5000) + 1)), int(g.integers(4, 65))))
            if g.random() < 0.6:
                ops.append(("lit", rnd(int(g.integers(1, 90)), int(g.integers(1 << 30)))))
        ops.append(("lit", rnd(TAIL, seed)))
        res.append(ops)
    return res


# ---- frames ---------------------------------------------------------------------------------
def _std_blocks(fmt, nbytes, bs, ts, split, mode, seed=0):
    """Blocks of a chunk of compressible bytes: every split one short stream (or stored)."""
    g = np.random.default_rng(seed)
    chunk = bytes(np.repeat(g.integers(1, 250, -(-nbytes // 8), dtype=np.uint8), 8)[:nbytes])
    blocks = []
    nfull, lo = divmod(nbytes, bs)
    for b in range(nfull + (1 if lo else 0)):
        raw = chunk[b * bs:(b + 1) * bs]
        left = b == nfull
        f = filtered(raw, ts, mode)
        ns = ts if (cblosc_splits(split, ts, bs) and not left) else 1
        ne = len(f) // ns
        bl = []
        for j in range(ns):
            part = f[j * ne:(j + 1) * ne]
            z = _rle_stream(fmt, part) if ne >= 24 and (b + j) % 3 != 2 else None
            if z is None or len(z) >= ne:
                bl.append(S(part, ne, True))
            else:
                bl.append(S(z, ne))
        blocks.append(bl)
    return blocks, chunk


def _rle_stream(fmt, part):
    """A valid stream of `part`: run-length matches at distance 1, literals elsewhere."""
    ops, i, lit, end = [], 0, bytearray(), len(part) - TAIL
    while i < end:
        j = i
        while j < end and part[j] == part[i]:
            j += 1
        if j - i >= 8:
            ops += [("lit", bytes(lit) + part[i:i + 1]), ("match", 1, j - i - 1)]
            lit = bytearray()
        else:
            lit += part[i:j]
        i = j
    ops.append(("lit", bytes(lit) + part[end:]))
    assert ops_decode(ops) == part
    return ENC[fmt](ops).bytes()


def _frames():
    out = []
    n = 8192

    def add(name, status, fr, expect=None, fam="frames", **kw):
        out.append(_frame_case(f"{fam}_{name}", fam, n, fr, expect if status == OK else None, status, **kw))

    def std(fmt="lz4", bs=2048, ts=4, split=True, mode=1, nbytes=n, seed=0, **kw):
        blocks, chunk = _std_blocks(fmt, nbytes, bs, ts, split, mode, seed)
        return assemble(blocks, comp=COMP[fmt], typesize=ts, nbytes=nbytes, blocksize=bs, mode=mode, split=split, **kw), chunk

    for fmt in ("lz4", "blosclz", "snappy"):
        f, c = std(fmt, bs=3000)
        add(f"{fmt}_leftover_block", OK, f, c)
        f, c = std(fmt, order=[3, 2, 1, 0])
        add(f"{fmt}_bstarts_reversed", OK, f, c)
        f, c = std(fmt, pads={0: 3, 1: 1, 2: 16, 3: 7})
        add(f"{fmt}_gaps_before_streams", OK, f, c)
    raw = rnd(n, 44)
    add("memcpyed", OK, assemble([[S(raw, n, True)]], comp=1, typesize=4, nbytes=n, blocksize=n, memcpy=True, mode=1), raw)
    # a memcpyed frame's compressor and compressor version are not read by c-blosc; its sizes are
    add("memcpyed_versionlz_7", OK, assemble([[S(raw, n, True)]], comp=1, typesize=4, nbytes=n, blocksize=n, memcpy=True, versionlz=7), raw)
    add("memcpyed_compressor_format_7", OK, assemble([[S(raw, n, True)]], comp=7, typesize=4, nbytes=n, blocksize=512, memcpy=True), raw)
    add("memcpyed_cbytes_over_payload", CORRUPT, assemble([[S(raw + b"xy", n + 2, True)]], comp=1, typesize=4, nbytes=n, blocksize=n, memcpy=True))
    add("memcpyed_blocksize_0", CORRUPT, assemble([[S(raw, n, True)]], comp=1, typesize=4, nbytes=n, blocksize=0, memcpy=True))
    add("memcpyed_typesize_0", CORRUPT, assemble([[S(raw, n, True)]], comp=1, typesize=0, nbytes=n, blocksize=n, memcpy=True))
    add("memcpyed_blosclz_bitshuffle_flag", OK, assemble([[S(raw, n, True)]], comp=0, typesize=2, nbytes=n, blocksize=n, memcpy=True, mode=2), raw)
    # typesize against the block, with and without the split flag: c-blosc decides which are valid
    # (c-blosc splits only typesize <= 16 with at least 128 elements a block, whatever the flag says)
    for ts in (3, 16, 17, 255):
        for split in (False, True):
            bs = {3: 3 * 256, 16: 2048, 17: 17 * 128, 255: 255 * 8}[ts]
            f, c = std("lz4", bs=bs, ts=ts, split=split, mode=1, seed=ts)
            add(f"typesize_{ts}_{'splitflag' if split else 'nosplit'}", OK, f, c)
    f, c = std("blosclz", bs=256, ts=4, split=True, mode=1, seed=5)
    add("split_flag_block_under_128_elements", OK, f, c, why="the flag allows a split; c-blosc does not split 64 elements")
    for split in (False, True):
        f, c = std("lz4", bs=64, ts=200, split=split, mode=1)
        add(f"typesize_larger_than_block_{'splitflag' if split else 'nosplit'}", OK, f, c)
    # corrupt layouts
    base = dict(fmt="lz4", bs=2048, ts=4, split=True, mode=1)
    hdr_len = 16 + 4 * 4
    f0, _ = std(**base)
    for name, kw in (("bstart_below_table", dict(bstarts={1: hdr_len - 1})), ("bstart_past_cbytes", dict(bstarts={2: len(f0.data) + 1})),
                     ("bstart_negative", dict(bstarts={3: -8}))):
        add(name, CORRUPT, std(**base, **kw)[0])

    def patched(name, fn, status=CORRUPT, expect=None, **kw):
        d = bytearray(f0.data)
        d = fn(d) or d
        add(name, status, Frame(bytes(d), f0.payload_off), expect, **kw)

    first = f0.payload_off[0][0] - 4
    patched("csize_negative", lambda d: d.__setitem__(slice(first, first + 4), (-5 & 0xFFFFFFFF).to_bytes(4, "little")))
    last = f0.payload_off[3][3] - 4
    patched("csize_past_cbytes", lambda d: d.__setitem__(slice(last, last + 4), (len(f0.data)).to_bytes(4, "little")))
    patched("cbytes_greater_than_buffer", lambda d: d.__setitem__(slice(12, 16), (len(d) + 1).to_bytes(4, "little")))
    patched("buffer_under_16_bytes", lambda d: d[:15])
    patched("typesize_0", lambda d: d.__setitem__(3, 0))
    patched("blocksize_0", lambda d: d.__setitem__(slice(8, 12), bytes(4)))
    blocks, _ = _std_blocks("lz4", n, 2050, 4, True, 0)
    add("blocksize_not_multiple_of_splits", CORRUPT,
        assemble(blocks, comp=1, typesize=4, nbytes=n, blocksize=2050, mode=0, split=True))
    for comp in (5, 6, 7):
        patched(f"compressor_format_{comp}", lambda d, comp=comp: d.__setitem__(2, (d[2] & 0x1F) | (comp << 5)))
    for dn in (1, -1):
        patched(f"nbytes_{'one_above' if dn > 0 else 'one_below'}_chunk", lambda d, dn=dn: d.__setitem__(slice(4, 8), (n + dn).to_bytes(4, "little")))
    patched("nbytes_0", lambda d: d.__setitem__(slice(4, 8), bytes(4)), why="an empty frame against a chunk of 8192 bytes: the sizes differ")
    # both shuffle bits: c-blosc takes the byte shuffle when typesize > 1 (blosc_d tests it first)
    f, c = std(**base)
    d = bytearray(f.data)
    d[2] |= 0x4
    add("both_shuffle_bits", OK, Frame(bytes(d), f.payload_off), c, why="c-blosc decides: byte shuffle wins")
    # the four header cases: c-blosc 1.21 rejects all of them
    patched("version_1", lambda d: d.__setitem__(0, 1))
    patched("version_3", lambda d: d.__setitem__(0, 3))
    patched("versionlz_7", lambda d: d.__setitem__(1, 7))
    return out


# ---- finish ---------------------------------------------------------------------------------
def _finish():
    out = []
    n = 8192
    for mode, mname in ((1, "shuffle"), (2, "bitshuffle")):
        for ts in (1, 2, 3, 4, 8, 16):
            # block sizes: a multiple of 16 * ts; not one (and, ts 1-2, an element count not a multiple
            # of 8); blocks then start at output offsets that are not multiples of 16; a leftover block
            for bname, bs in (("aligned", 16 * ts * 8), ("odd", 16 * ts * 8 + ts * 3 + (1 if ts > 1 else 3))):
                for fmt in (("lz4", "blosclz", "snappy") if (ts, bname) in ((4, "aligned"), (2, "odd")) else ("lz4",)):
                    for split in ((False, True) if ts > 1 and bs % ts == 0 else (False,)):
                        blocks, chunk = _std_blocks(fmt, n, bs, ts, split, mode, seed=ts * 10 + mode)
                        pads = {b: (b * 5 + 1) % 16 for b in range(len(blocks))}  # stored planes at odd addresses
                        f = assemble(blocks, comp=COMP[fmt], typesize=ts, nbytes=n, blocksize=bs, mode=mode, split=split, pads=pads)
                        out.append(_frame_case(f"finish_{mname}_ts{ts}_{bname}_{fmt}_{'split' if split else 'nosplit'}", "finish", n, f, chunk))
    return out


# ---- corrupt --------------------------------------------------------------------------------
def _short_stream(fmt):
    """A short stream with every element kind, decoding to 8192."""
    if fmt == "lz4":
        return _finish_stream("lz4", Lz4W().seq(rnd(20, 1), 9, 30).seq(rnd(3, 2), 2, 7), 8192).bytes()
    if fmt == "blosclz":
        return _finish_stream("blosclz", BlzW().lit(rnd(20, 1)).match(9, 30).lit(rnd(3, 2)).match(2, 7), 8192).bytes()
    return _finish_stream("snappy", SnW().preamble(8192).literal(rnd(20, 1)).copy(9, 8, 1).literal(rnd(70, 2)).copy(2, 7, 2).copy(50, 9, 3), 8192).bytes()


def _corrupt():
    out = []
    n = 8192
    for fmt in FMTS:
        z = _short_stream(fmt)
        for k in range(1, len(z)):
            # a prefix is corrupt when it fails to decode or decodes to another size (the oracle decides for lz4 / blosclz)
            out.append(Case(f"corrupt_{fmt}_cut_after_{k}", "corrupt", n, status=CORRUPT, fmt=fmt, stream=lambda r, z=z[:k]: z))
        def raw(name, w, **kw):
            out.append(Case(f"corrupt_{fmt}_{name}", "corrupt", n, status=CORRUPT, fmt=fmt, stream=lambda r, z=w.bytes(): z, **kw))

        def with_match(off, name):
            if fmt == "lz4":
                w = Lz4W().seq(rnd(30, 1), off, 8)
            elif fmt == "blosclz":
                w = BlzW().lit(rnd(30, 1))
                if off == 0:
                    return  # blosclz stores distance - 1: offset 0 cannot be written
                w.match(off, 8)
            else:
                w = SnW().preamble(n).literal(rnd(30, 1)).copy(off, 8, 2)
            raw(name, _finish_stream(fmt, w, n))

        if fmt != "lz4":  # lz4: lenient_lz4_offset_0
            with_match(0, "offset_0")
        with_match(31, "offset_op_plus_1")
        # output one byte over / under the block: a two-block frame (ne = 4096) beside chunks of one 8192-byte
        # block, so the decoders' bound is the batch's largest and only k_blosc_finish's length check sees it
        for d, name in ((1, "one_byte_over_ne"), (-1, "one_byte_under_ne")):
            ops = pad_ops([("lit", rnd(30, 1))], 4096 + d)
            w = ENC[fmt](ops) if fmt != "snappy" else enc_snappy(ops, SnW().preamble(4096 + d))
            out.append(Case(f"corrupt_{fmt}_{name}", "corrupt", n, status=CORRUPT, fmt=fmt, stream=lambda r, z=w.bytes(): z,
                            ne=4096, cap=n))
    for d, name in ((1, "preamble_one_above_output"), (-1, "preamble_one_below_output")):
        ops = pad_ops([("lit", rnd(30, 1))], n)
        out.append(Case(f"corrupt_snappy_{name}", "corrupt", n, status=CORRUPT, fmt="snappy",
                        stream=lambda r, z=enc_snappy(ops, SnW().preamble(n + d)).bytes(): z, cap=2 * n))
    ops = pad_ops([("lit", rnd(30, 1))], n)
    out.append(Case("corrupt_snappy_preamble_6_bytes", "corrupt", n, status=CORRUPT, fmt="snappy",
                    stream=lambda r, z=enc_snappy(ops, SnW().preamble(n, 6)).bytes(): z))
    return out


# ---- lenient: streams c-blosc rejects and the decoders accept by design ----------------------
def _lenient():
    n = 8192
    out = []
    pre = prefix_ops(n - 100)

    def lz4(name, w, why, **kw):
        out.append(Case(f"lenient_lz4_{name}", "lenient", n, status=LENIENT, fmt="lz4", stream=lambda r, z=w.bytes(): z,
                        why=why, gpu_accepts=True, **kw))

    # LZ4's end-of-block rules (lz4_Block_format.md: the last 5 bytes are literals, the last match starts
    # at least 12 bytes before the end), which LZ4_decompress_safe enforces against the block's size
    lz4("match_ends_4_before_end", enc_lz4(pre + [("match", 7, 96), ("lit", rnd(4, 1))]),
        "a match ending 4 bytes before the end (fewer than 5 final literals)")
    lz4("match_ends_at_end_empty_last_sequence", enc_lz4(pre + [("match", 7, 100), ("lit", b"")]),
        "a match ending at the end, then an empty literals-only sequence (token 0)")
    lz4("match_starts_in_last_12", enc_lz4(pre + [("lit", rnd(90, 2)), ("match", 7, 5), ("lit", rnd(5, 1))]),
        "a match starting 10 bytes before the end")
    out.append(Case("lenient_blosclz_ends_on_far_match", "lenient", 16384, status=LENIENT, fmt="blosclz",
                    stream=lambda r, z=enc_blz([("lit", rnd(251, 7)), ("match", 251, 16384 - 251 - 40), ("match", 8192 + 77, 40)]).bytes(): z,
                    why="a stream whose last bytes are a far match: blosclz_decompress leaves its loop before the copy",
                    gpu_accepts=True))
    # bytes after the frame (header cbytes below the buffer's length): blosc_cbuffer_validate wants them equal.
    # Kept: a plan re-executed over device buffers rewritten in place keeps each buffer's length, whatever
    # frame it holds (tests/test_gpu_blosc.py::test_blosc_plan_cached_layout_and_rerun)
    ops = pad_ops(prefix_ops(300), n)
    fr = one_block("lz4", enc_lz4(ops).bytes(), n)
    out.append(_frame_case("lenient_trailing_bytes", "lenient", n, Frame(fr.data + b"\0\0\0", fr.payload_off), ops_decode(ops),
                           status=LENIENT, gpu_accepts=True, why="bytes after the frame are ignored"))
    # blocksize above nbytes: blosc_cbuffer_validate refuses it. Kept: the frame is then its one leftover block,
    # and frame writers that do not clamp the block size emit it (test_gpu_blosc.py's snappy frames of 1000 bytes)
    d = bytearray(fr.data)
    d[8:12] = (2 * n).to_bytes(4, "little")
    out.append(_frame_case("lenient_blocksize_greater_than_nbytes", "lenient", n, Frame(bytes(d), fr.payload_off), ops_decode(ops),
                           status=LENIENT, gpu_accepts=True, why="decoded as one leftover block"))
    # the other way round: lz4_Block_format.md calls offset 0 invalid and the decoders refuse it, but
    # LZ4_decompress_safe copies from the destination it has not written yet and c-blosc returns those bytes
    out.append(Case("lenient_lz4_offset_0", "lenient", n, status=LENIENT, fmt="lz4", gpu_accepts=False, cblosc_unspecified=True,
                    stream=lambda r, z=_finish_stream("lz4", Lz4W().seq(rnd(30, 1), 0, 8), n).bytes(): z,
                    why="offset 0: refused here, unspecified bytes from c-blosc"))
    return out


FAMILIES = {"window": _window, "ring": _ring, "lengths": _lengths, "pairs": _pairs, "frames": _frames,
            "finish": _finish, "corrupt": _corrupt, "lenient": _lenient}


@functools.lru_cache(None)
def family(name):
    cs = FAMILIES[name]()
    assert all(c.family == name and c.size in SIZES for c in cs), name
    return cs


def all_cases():
    return [c for f in FAMILIES for c in family(f)]
