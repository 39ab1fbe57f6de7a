"""Exact model of the cast_value codec in Python integers and fractions.Fraction, written from the
codec's rules (no numpy casts, no floating point arithmetic):

  element     bits of one of int8..int64, uint8..uint64, float16, bfloat16, float32, float64 -> an exact
              integer, an exact rational (with the sign of a zero), NaN or +-infinity
  scalar map  first: an element whose bits equal a key's bits becomes that entry's value (first entry
              wins; it never fails)
  -> integer  a float rounds to an integer in the rounding mode (NaN, +-inf: not representable); a value
              outside the target's range is not representable (out_of_range absent), the nearer bound
              (clamp) or the value modulo 2^bits in two's complement (wrap)
  -> float    NaN -> the canonical NaN; +-inf pass; a finite value outside [-max, max] of the target
              (tested on the exact value) is not representable (absent), +-inf (clamp), or by the
              rounding mode the bound or +-inf (wrap: towards-zero and the mode pointing back inside give
              the bound); otherwise it rounds once to the format (precision, emin, emax) in the rounding
              mode, subnormals kept, -0.0 kept

bfloat16 is carried as its uint16 bits (numpy has no bfloat16). CastModelChain composes the model with
value_codecs (fixedscaleoffset, bitround) and the CPU oracle for the rest of a chain, as
value_codecs.ModelChain does for those codecs."""
from fractions import Fraction

import numpy as np

import oracle as O
import value_codecs as V

INTS = {"int8": (True, 8), "int16": (True, 16), "int32": (True, 32), "int64": (True, 64),
        "uint8": (False, 8), "uint16": (False, 16), "uint32": (False, 32), "uint64": (False, 64)}
FLOATS = {"float16": (11, 5), "bfloat16": (8, 8), "float32": (24, 8), "float64": (53, 11)}  # (precision, exponent bits)
TYPES = list(INTS) + list(FLOATS)
ROUNDINGS = ["nearest-even", "towards-zero", "towards-positive", "towards-negative", "nearest-away"]
OUT_OF_RANGE = [None, "clamp", "wrap"]
NAME = "cast_value"
MAP_MAX = 32


def size_of(t):
    return (INTS[t][1] if t in INTS else sum(FLOATS[t]) ) // 8


def is_float(t):
    return t in FLOATS


def float_max(t):
    p, eb = FLOATS[t]
    bias = (1 << (eb - 1)) - 1
    return Fraction((1 << p) - 1) * Fraction(2) ** (bias - (p - 1))


def canonical_nan(t):
    p, eb = FLOATS[t]
    return ((1 << (eb + 1)) - 1) << (p - 2)


def inf_bits(t, negative):
    p, eb = FLOATS[t]
    return (int(negative) << (p - 1 + eb)) | (((1 << eb) - 1) << (p - 1))


def decode(bits, t):
    """('int', n) | ('nan',) | ('inf', negative) | ('fin', Fraction, negative)"""
    if t in INTS:
        signed, w = INTS[t]
        return ("int", bits - (1 << w) if signed and bits >> (w - 1) else bits)
    p, eb = FLOATS[t]
    negative = bool(bits >> (p - 1 + eb))
    ef = (bits >> (p - 1)) & ((1 << eb) - 1)
    m = bits & ((1 << (p - 1)) - 1)
    bias = (1 << (eb - 1)) - 1
    if ef == (1 << eb) - 1:
        return ("nan",) if m else ("inf", negative)
    if ef == 0:
        mag = Fraction(m) * Fraction(2) ** (1 - bias - (p - 1))
    else:
        mag = Fraction(m | (1 << (p - 1))) * Fraction(2) ** (ef - bias - (p - 1))
    return ("fin", -mag if negative else mag, negative)


def _round_int(q, negative, rounding):
    """a non-negative rational magnitude -> integer magnitude, in the mode (negative: the value's sign)"""
    k = q.numerator // q.denominator
    rem = q - k
    if rem == 0:
        return k
    half = Fraction(1, 2)
    up = {"nearest-even": rem > half or (rem == half and k & 1),
          "towards-zero": False,
          "towards-positive": not negative,
          "towards-negative": negative,
          "nearest-away": rem >= half}[rounding]
    return k + 1 if up else k


def round_once(x, negative, t, rounding):
    """the rational x (negative: its sign, which a zero keeps), |x| <= float_max(t), -> bits of t"""
    p, eb = FLOATS[t]
    bias = (1 << (eb - 1)) - 1
    sbit = int(negative) << (p - 1 + eb)
    a = abs(x)
    if a == 0:
        return sbit
    e = a.numerator.bit_length() - a.denominator.bit_length()  # floor(log2 a) or one above
    if Fraction(2) ** e > a:
        e -= 1
    et = max(e, 1 - bias)
    kept = _round_int(a / Fraction(2) ** (et - (p - 1)), negative, rounding)
    return sbit | (((et + bias - 1) << (p - 1)) + kept)


def cast(bits, s, t, rounding="nearest-even", out_of_range=None):
    """one element's bits of type s -> bits of type t, or None: not representable"""
    v = decode(bits, s)
    if t in INTS:
        signed, w = INTS[t]
        lo, hi = (-(1 << (w - 1)), (1 << (w - 1)) - 1) if signed else (0, (1 << w) - 1)
        if v[0] in ("nan", "inf"):
            return None
        if v[0] == "int":
            n = v[1]
        else:
            n = _round_int(abs(v[1]), v[2], rounding)
            n = -n if v[2] else n
        if n < lo or n > hi:
            if out_of_range is None:
                return None
            n = min(max(n, lo), hi) if out_of_range == "clamp" else n
        return n & ((1 << w) - 1)
    if v[0] == "nan":
        return canonical_nan(t)
    if v[0] == "inf":
        return inf_bits(t, v[1])
    x, negative = (Fraction(v[1]), v[1] < 0) if v[0] == "int" else (v[1], v[2])
    if abs(x) > float_max(t):
        if out_of_range is None:
            return None
        if out_of_range == "clamp":
            return inf_bits(t, negative)
        inward = "towards-positive" if negative else "towards-negative"
        if rounding in ("towards-zero", inward):
            return round_once(-float_max(t) if negative else float_max(t), negative, t, "towards-zero")
        return inf_bits(t, negative)
    return round_once(x, negative, t, rounding)


def cast_list(elems, s, t, rounding="nearest-even", out_of_range=None, smap=()):
    """elems: bits of s. Returns (bits of t up to the first failure, index of the first failure or None)."""
    out = []
    for i, b in enumerate(elems):
        hit = next((val for key, val in smap if key == b), None)
        y = hit if hit is not None else cast(b, s, t, rounding, out_of_range)
        if y is None:
            return out, i
        out.append(y)
    return out, None


def infallible(s, t, out_of_range):
    """no element of s can fail to cast to t: stated from the types' value sets"""
    if is_float(s) and not is_float(t):
        return False
    if out_of_range is not None:
        return True

    def span(ty):
        if ty in INTS:
            signed, w = INTS[ty]
            return (-(1 << (w - 1)), (1 << (w - 1)) - 1) if signed else (0, (1 << w) - 1)
        return (-float_max(ty), float_max(ty))
    (slo, shi), (tlo, thi) = span(s), span(t)
    return tlo <= slo and shi <= thi


# ---------------------------------------------------------------------------------------------------
# bytes, scalars of the metadata
# ---------------------------------------------------------------------------------------------------
def to_bytes(bits_list, t):
    return b"".join(int(b).to_bytes(size_of(t), "little") for b in bits_list)


def from_bytes(data, t):
    n = size_of(t)
    return [int.from_bytes(data[i:i + n], "little") for i in range(0, len(data), n)]


def scalar_bits(value, t):
    """a scalar_map key or value as the type's fill value metadata is read: integers for the integer
    types; numbers, "NaN", "Infinity", "-Infinity" and "0x..." bit strings for the floats"""
    if t in INTS:
        signed, w = INTS[t]
        if isinstance(value, bool) or not isinstance(value, int):
            raise ValueError(f"{value!r} is no {t}")
        lo, hi = (-(1 << (w - 1)), (1 << (w - 1)) - 1) if signed else (0, (1 << w) - 1)
        if not lo <= value <= hi:
            raise ValueError(f"{value!r} is no {t}")
        return value & ((1 << w) - 1)
    if isinstance(value, str):
        if value == "NaN":
            return canonical_nan(t)
        if value in ("Infinity", "-Infinity"):
            return inf_bits(t, value[0] == "-")
        if value.startswith("0x") and len(value) == 2 + 2 * size_of(t):
            return int(value[2:], 16)
        raise ValueError(f"{value!r} is no {t}")
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise ValueError(f"{value!r} is no {t}")
    f = float(value)  # a JSON number reads as a double, then rounds to nearest even
    b64 = int.from_bytes(np.float64(f).tobytes(), "little")
    return cast(b64, "float64", t, "nearest-even", "clamp")


def scalar_map(cfg, direction, src, dst):
    entries = ((cfg.get("scalar_map") or {}).get(direction)) or []
    return [(scalar_bits(k, src), scalar_bits(v, dst)) for k, v in entries]


def target_of(cfg):
    dt = cfg["data_type"]
    return dt["name"] if isinstance(dt, dict) else dt


def encode_bits(elems, cfg, data_type):
    t = target_of(cfg)
    return cast_list(elems, data_type, t, cfg.get("rounding") or "nearest-even", cfg.get("out_of_range"),
                     scalar_map(cfg, "encode", data_type, t))


def decode_bits(elems, cfg, data_type):
    t = target_of(cfg)
    return cast_list(elems, t, data_type, cfg.get("rounding") or "nearest-even", cfg.get("out_of_range"),
                     scalar_map(cfg, "decode", t, data_type))


# ---------------------------------------------------------------------------------------------------
# test inputs
# ---------------------------------------------------------------------------------------------------
def edge_elements(t):
    """the fixed edge list of a source type, as bits"""
    if t in INTS:
        signed, w = INTS[t]
        lo, hi = (-(1 << (w - 1)), (1 << (w - 1)) - 1) if signed else (0, (1 << w) - 1)
        vals = [lo, lo + 1, -129, -128, -1, 0, 1, 2, 3, 127, 128, 255, 256]
        for k in (15, 16, 24, 31, 32, 53):
            vals += [(1 << k) - 1, (1 << k) + 1]
        vals += [(1 << 63) - 1, 1 << 63, (1 << 63) + (1 << 39) - 1, (1 << 63) + (1 << 39) + 1, (1 << 64) - 1]
        out = []
        for v in vals:
            if lo <= v <= hi and v & ((1 << w) - 1) not in out:
                out.append(v & ((1 << w) - 1))
        return out
    p, eb = FLOATS[t]
    f64 = lambda x: int.from_bytes(np.float64(x).tobytes(), "little")  # noqa: E731
    mags = [0.0, 1.0, 2.0, 3.0, 0.5, 1.5, 2.5, 127.5, 255.5, 65504.0, 65519.0, 65520.0, 2.0 ** 31, 2.0 ** 63, 2.0 ** 64, 2.0 ** 127]
    out = []

    def add(b):
        if b is not None and b not in out:
            out.append(b)
    for m in mags:
        for sgn in (1.0, -1.0):
            # the value itself where the type holds it exactly (towards-zero from the double, exact or dropped)
            b = cast(f64(sgn * m), "float64", t, "towards-zero", None)
            if b is not None and decode(b, t)[0] == "fin" and decode(b, t)[1] == Fraction(sgn * m):
                add(b)
    sign = 1 << (p - 1 + eb)
    maxb = inf_bits(t, False) - 1
    for b in (1, maxb, inf_bits(t, False), ):
        add(b)
        add(b | sign)
    add(canonical_nan(t))
    add(canonical_nan(t) | sign | 1)  # a negative NaN with a payload
    # for every narrower format: a value halfway between two of its neighbours, and the halfway's two
    # neighbours in float64 (which only float64 holds)
    for u in FLOATS:
        pu, _ = FLOATS[u]
        if pu >= p:
            continue
        one = decode(round_once(Fraction(1), False, u, "towards-zero"), u)[1]
        half = one + Fraction(2) ** (-pu)  # between 1 and 1 + 2^(1 - pu) of u
        add(round_once(half, False, t, "towards-zero"))
        add(round_once(-half, True, t, "towards-zero"))
        if t == "float64":
            hb = round_once(half, False, t, "towards-zero")
            for b in (hb - 1, hb + 1):
                add(b)
                add(b | sign)
    return out


def xorshift_elements(t, n=64, seed=0x9E3779B97F4A7C15):
    state = seed
    data = bytearray()
    for _ in range(n * size_of(t)):
        state ^= (state << 13) & 0xFFFFFFFFFFFFFFFF
        state ^= state >> 7
        state ^= (state << 17) & 0xFFFFFFFFFFFFFFFF
        data.append(state & 0xFF)
    return from_bytes(bytes(data), t)


def error_free(elems, s, t, rounding, out_of_range, smap=()):
    return [b for b in elems if cast_list([b], s, t, rounding, out_of_range, smap)[1] is None]


# ---------------------------------------------------------------------------------------------------
# chains: the model around value_codecs and the oracle
# ---------------------------------------------------------------------------------------------------
class NotRepresentable(ValueError):
    def __init__(self, index):
        super().__init__(f"element {index} is not representable")
        self.index = index


def _bits_of(a, t):
    a = np.ascontiguousarray(a)
    return [int(x) for x in a.reshape(-1).view(f"<u{size_of(t)}")]


def _array_of(bits, t, shape):
    return np.array(bits, dtype=object).astype(f"<u{size_of(t)}").view(V.NP[t]).reshape(shape)


def _is_value(c):
    return c["name"] == NAME or V._is_value(c)


def _encode_step(a, c, data_type):
    if c["name"] != NAME:
        return V._apply_encode(a, c, data_type)
    out, bad = encode_bits(_bits_of(a, data_type), c["configuration"], data_type)
    if bad is not None:
        raise NotRepresentable(bad)
    return _array_of(out, target_of(c["configuration"]), a.shape)


def _decode_step(e, c, data_type):
    if c["name"] != NAME:
        return V._apply_decode(e, c)
    out, bad = decode_bits(_bits_of(e, target_of(c["configuration"])), c["configuration"], data_type)
    if bad is not None:
        raise NotRepresentable(bad)
    return _array_of(out, data_type, e.shape)


def _strip(codecs, data_type, fill, steps):
    """as value_codecs._strip with cast_value among the value codecs; fill is a 1-element array"""
    a2a = [c for c in codecs if c["name"] == "transpose" or _is_value(c)]
    rest = [c for c in codecs if not (c["name"] == "transpose" or _is_value(c))]
    out = []
    for c in a2a:
        if c["name"] == "transpose":
            out.append(c)
            continue
        steps.append((c, data_type))
        fill = _encode_step(fill, c, data_type)
        if c["name"] == NAME:
            data_type = target_of(c["configuration"])
        elif c["name"] == V.FSO and c["configuration"].get("astype"):
            data_type = V.v3_name(c["configuration"]["astype"])
    for c in rest:
        if c["name"] == "sharding_indexed":
            cfg = dict(c["configuration"])
            cfg["codecs"], data_type, fill = _strip(cfg["codecs"], data_type, fill, steps)
            out.append({"name": c["name"], "configuration": cfg})
        else:
            out.append(c)
    return out, data_type, fill


class CastModelChain:
    """A chain with cast_value (and fixedscaleoffset / bitround) around the oracle's chain without them."""

    def __init__(self, codecs, data_type, fill=0, ndim=1):
        self.data_type, self.ndim = data_type, ndim
        self.steps = []
        f = _array_of([scalar_bits(fill, data_type)], data_type, (1,))
        self.stripped, self.enc_type, ef = _strip(codecs, data_type, f, self.steps)
        self.enc_fill = ef.tobytes()
        # (the oracle carries the 16-bit floats as their uint16 bits through the same codecs)
        self.otype = "uint16" if self.enc_type in ("bfloat16", "float16") else self.enc_type
        self.oracle = O.OracleChain.from_metadata(self.stripped, self.otype, self.enc_fill, ndim)

    def encode_values(self, a):
        for c, dt in self.steps:
            a = _encode_step(a, c, dt)
        return a

    def decode_values(self, e):
        for c, dt in reversed(self.steps):
            e = _decode_step(e, c, dt)
        return e

    def encode(self, a):
        e = self.encode_values(np.ascontiguousarray(a))
        return self.oracle.encode(e.view(V.NP[self.otype]))

    def decode(self, enc, shape):
        e = self.oracle.decode(enc, [int(s) for s in shape])
        return self.decode_values(e.view(V.NP[self.enc_type]))

    def decoded_fill(self, shape):
        """what a missing chunk decodes to: the decoded form of the encoded fill value"""
        one = np.frombuffer(self.enc_fill, V.NP[self.enc_type])
        return self.decode_values(np.full(shape, one[0], V.NP[self.enc_type]))
