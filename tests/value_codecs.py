"""Plain numpy model of the codecs that change element values or widths: numcodecs.fixedscaleoffset,
bitround and packbits, written from their definitions (not a port of any implementation).

  fixedscaleoffset  encode: round((x as F - offset as F) * scale as F) as T, then (with `astype`) T ->
                    f32 -> astype; decode: (with `astype`) astype -> f32 -> T, then
                    (x as F / scale as F + offset as F) as T. F is f32 for 8/16-bit integers and f32,
                    f64 otherwise; offset and scale are f32. `round` is half away from zero; every
                    float -> integer cast truncates, saturates and maps NaN to 0 (explicitly: numpy's
                    own out-of-range cast is not defined and is never used here).
  bitround          encode on the raw bits x of width W, with m = maxbits - keepbits > 0:
                    sat_add(x, ((x >> m) & 1) + (1 << (m - 1)) - 1) & ~((1 << m) - 1); maxbits is the
                    mantissa width for floats and W - clz(x) for integers. decode: identity.
  packbits          bits first_bit..last_bit of every component, least significant first, back to back
                    into bytes from bit 0 up, zero-padded to a byte; an optional first / last byte holds
                    the number of padding bits. Decode sign-extends signed integers only through the
                    rest of the byte that holds the sign bit.

ModelChain composes them with the CPU oracle for the rest of a chain: the model transforms the array,
the oracle encodes the chain without the value codecs in the encoded data type (packbits: the oracle
encodes the packed bytes as a 1-D uint8 array)."""
import numpy as np

import oracle as O

NP = {"bool": "?", "int8": "i1", "int16": "<i2", "int32": "<i4", "int64": "<i8", "uint8": "u1", "uint16": "<u2",
      "uint32": "<u4", "uint64": "<u8", "float16": "<f2", "float32": "<f4", "float64": "<f8",
      "complex64": "<c8", "complex128": "<c16",
      "bfloat16": "<u2"}  # numpy has no bfloat16: its arrays hold the raw bits here
V3 = {"b1": "bool", "i1": "int8", "i2": "int16", "i4": "int32", "i8": "int64", "u1": "uint8", "u2": "uint16",
      "u4": "uint32", "u8": "uint64", "f2": "float16", "f4": "float32", "f8": "float64"}
MANTISSA = {"float16": 10, "bfloat16": 7, "float32": 23, "float64": 52}
BITROUND_NAMES = ("bitround", "numcodecs.bitround")
FSO = "numcodecs.fixedscaleoffset"


def v3_name(numpy_str):
    return V3[numpy_str.lstrip("<>|=")]


# ---------------------------------------------------------------------------------------------------
# casts
# ---------------------------------------------------------------------------------------------------
def sat_cast(x, to):
    """float array -> integer dtype: truncate toward zero, saturate at the bounds, NaN -> 0."""
    to = np.dtype(to)
    info = np.iinfo(to)
    x = np.asarray(x)
    hi_excl = x.dtype.type(2.0) ** (info.bits - (1 if info.min < 0 else 0))  # a power of two: exact
    lo = x.dtype.type(info.min)
    out = np.zeros(x.shape, to)
    nan = np.isnan(x)
    high = ~nan & (x >= hi_excl)
    low = ~nan & (x <= lo)
    mid = ~(nan | high | low)
    out[high] = info.max
    out[low] = info.min
    out[mid] = np.trunc(x[mid]).astype(to)  # in range: exact
    return out


def cast(x, to):
    """`x as to` of the reference's language for numeric arrays."""
    to = np.dtype(to)
    x = np.asarray(x)
    if to.kind in "iu" and x.dtype.kind == "f":
        return sat_cast(x, to)
    with np.errstate(over="ignore"):
        return x.astype(to)  # integer -> float and float -> float round to nearest even


def round_away(p):
    """round half away from zero; p - trunc(p) is exact in floating point."""
    with np.errstate(invalid="ignore"):
        t = np.trunc(p)
        up = np.abs(p - t) >= p.dtype.type(0.5)
        return np.where(up, t + np.sign(p), t).astype(p.dtype)


def _float_of(dt):
    dt = np.dtype(dt)
    return np.float32 if (dt.kind in "iu" and dt.itemsize <= 2) or dt == np.float32 else np.float64


# ---------------------------------------------------------------------------------------------------
# fixedscaleoffset
# ---------------------------------------------------------------------------------------------------
def fso_encode(a, offset, scale, dtype, astype=None):
    dt = np.dtype(NP[v3_name(dtype)])
    a = np.asarray(a)
    assert a.dtype == dt
    F = _float_of(dt)
    with np.errstate(all="ignore"):
        p = (cast(a, F) - F(np.float32(offset))) * F(np.float32(scale))
        t = cast(round_away(p), dt)
    if astype is None:
        return t
    return cast(cast(t, np.float32), NP[v3_name(astype)])


def fso_decode(e, offset, scale, dtype, astype=None):
    dt = np.dtype(NP[v3_name(dtype)])
    e = np.asarray(e)
    t = e if astype is None else cast(cast(e, np.float32), dt)
    assert t.dtype == dt
    F = _float_of(dt)
    with np.errstate(all="ignore"):
        r = cast(t, F) / F(np.float32(scale)) + F(np.float32(offset))
    return cast(r, dt)


# ---------------------------------------------------------------------------------------------------
# bitround
# ---------------------------------------------------------------------------------------------------
def _round_bits(x, keepbits, maxbits, width):
    if keepbits >= maxbits:
        return x
    m = maxbits - keepbits
    full = (1 << width) - 1
    s = min(x + ((x >> m) & 1) + (1 << (m - 1)) - 1, full)  # the add saturates
    return s & ~((1 << m) - 1) & full


def bitround_bits(raw, keepbits, data_type):
    """bitround encode of an unsigned array holding the raw bits of `data_type` elements."""
    width = raw.dtype.itemsize * 8
    mant = MANTISSA.get(data_type)
    out = [_round_bits(int(x), keepbits, mant if mant else int(x).bit_length(), width) for x in raw.reshape(-1)]
    return np.array(out, dtype=object).astype(raw.dtype).reshape(raw.shape)


def bitround_encode(a, keepbits, data_type):
    a = np.ascontiguousarray(a)
    raw = a.view(f"<u{a.dtype.itemsize}")
    return bitround_bits(raw, keepbits, data_type).view(a.dtype)


# ---------------------------------------------------------------------------------------------------
# packbits
# ---------------------------------------------------------------------------------------------------
def _components(data_type):
    """(bits per component, components per element, unsigned view dtype, sign extension)"""
    if data_type == "bool":
        return 1, 1, np.dtype("u1"), False
    dt = np.dtype(NP[data_type])
    ncomp = 2 if dt.kind == "c" else 1
    size = dt.itemsize // ncomp
    return 8 * size, ncomp, np.dtype(f"<u{size}"), dt.kind == "i"


def packbits_geometry(data_type, first_bit=None, last_bit=None):
    bits, ncomp, udt, signed = _components(data_type)
    first = 0 if first_bit is None else first_bit
    last = bits - 1 if last_bit is None else last_bit
    assert first <= last < bits
    return first, last, bits, ncomp, udt, signed


def packbits_is_bytes(data_type, first_bit=None, last_bit=None):
    first, last, bits, _, _, _ = packbits_geometry(data_type, first_bit, last_bit)
    return bits % 8 == 0 and first == 0 and last == bits - 1


def packbits_size(n, data_type, first_bit=None, last_bit=None, padding="none"):
    first, last, _, ncomp, _, _ = packbits_geometry(data_type, first_bit, last_bit)
    return (n * (last - first + 1) * ncomp + 7) // 8 + (0 if padding == "none" else 1)


def packbits_encode(a, data_type, first_bit=None, last_bit=None, padding="none"):
    first, last, _, _, udt, _ = packbits_geometry(data_type, first_bit, last_bit)
    comps = np.ascontiguousarray(a).reshape(-1).view(udt).astype(np.uint64)
    ext = last - first + 1
    bits = ((comps[:, None] >> np.arange(first, last + 1, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
    body = np.packbits(bits.reshape(-1), bitorder="little").tobytes()
    pad = bytes([(-(comps.size * ext)) % 8])
    return {"none": body, "first_byte": pad + body, "last_byte": body + pad}[padding]


class PackBitsError(ValueError):
    pass


def packbits_decode(enc, n, data_type, first_bit=None, last_bit=None, padding="none"):
    first, last, _, ncomp, udt, signed = packbits_geometry(data_type, first_bit, last_bit)
    ext = last - first + 1
    if len(enc) != packbits_size(n, data_type, first_bit, last_bit, padding):
        raise PackBitsError("length")
    pad = (-(n * ncomp * ext)) % 8
    if padding == "first_byte":
        if enc[0] != pad:
            raise PackBitsError("padding byte")
        enc = enc[1:]
    elif padding == "last_byte":
        if enc[-1] != pad:
            raise PackBitsError("padding byte")
        enc = enc[:-1]
    bits = np.unpackbits(np.frombuffer(enc, np.uint8), bitorder="little")[:n * ncomp * ext].reshape(n * ncomp, ext)
    comps = np.zeros(n * ncomp, np.uint64)
    for k in range(ext):
        comps |= bits[:, k].astype(np.uint64) << np.uint64(first + k)
    if signed:
        # the rest of the byte that holds the sign bit, not the rest of the component
        fill = np.uint64(((0xFF << (last % 8 + 1)) & 0xFF) << (8 * (last // 8)))
        comps = np.where(bits[:, ext - 1] == 1, comps | fill, comps)
    out = comps.astype(udt)
    return out.view("?" if data_type == "bool" else NP[data_type])


# ---------------------------------------------------------------------------------------------------
# chains: the model around the oracle
# ---------------------------------------------------------------------------------------------------
def _is_value(c):
    return c["name"] == FSO or c["name"] in BITROUND_NAMES


def _strip(codecs, data_type, fill, steps):
    """codecs without the value codecs (recursively through sharding_indexed); steps gets (codec,
    decoded data type) in encode order; returns (stripped codecs, encoded data type, encoded fill)."""
    a2a = [c for c in codecs if c["name"] == "transpose" or _is_value(c)]
    rest = [c for c in codecs if not (c["name"] == "transpose" or _is_value(c))]
    out = []
    for c in a2a:
        if c["name"] == "transpose":
            out.append(c)
            continue
        steps.append((c, data_type))
        f = np.array([fill], NP[data_type])
        f = _apply_encode(f, c, data_type)
        if c["name"] == FSO and c["configuration"].get("astype"):
            data_type = v3_name(c["configuration"]["astype"])
        fill = f[0].item()
    for c in rest:
        if c["name"] == "sharding_indexed":
            cfg = dict(c["configuration"])
            cfg["codecs"], data_type, fill = _strip(cfg["codecs"], data_type, fill, steps)
            out.append({"name": c["name"], "configuration": cfg})
        else:
            out.append(c)
    return out, data_type, fill


def _apply_encode(a, c, data_type):
    cfg = c["configuration"]
    if c["name"] == FSO:
        return fso_encode(a, cfg["offset"], cfg["scale"], cfg["dtype"], cfg.get("astype"))
    return bitround_encode(a, cfg["keepbits"], data_type)


def _apply_decode(e, c):
    cfg = c["configuration"]
    if c["name"] == FSO:
        return fso_decode(e, cfg["offset"], cfg["scale"], cfg["dtype"], cfg.get("astype"))
    return e


class ModelChain:
    """A chain with value codecs and / or packbits (unsharded) as the array->bytes codec."""

    def __init__(self, codecs, data_type, fill=0, ndim=1):
        self.data_type, self.ndim = data_type, ndim
        self.steps = []
        self.stripped, self.enc_type, self.enc_fill = _strip(codecs, data_type, fill, self.steps)
        self.pack = next((c for c in self.stripped if c["name"] == "packbits"), None)
        if self.pack is not None:
            cfg = self.pack.get("configuration", {})
            self.pb = dict(first_bit=cfg.get("first_bit"), last_bit=cfg.get("last_bit"),
                           padding=cfg.get("padding_encoding") or "none")
            self.orders = [c["configuration"]["order"] for c in self.stripped if c["name"] == "transpose"]
            b2b = self.stripped[self.stripped.index(self.pack) + 1:]
            if packbits_is_bytes(self.enc_type, self.pb["first_bit"], self.pb["last_bit"]):
                # the whole component of a byte-sized type is `bytes` little-endian, without a padding byte
                self.pack = None
                self.stripped = [c if c["name"] != "packbits" else
                                 {"name": "bytes", "configuration": {"endian": "little"}} for c in self.stripped]
            else:
                self.oracle = O.OracleChain.from_metadata(
                    [{"name": "bytes", "configuration": {"endian": "little"}}] + b2b, "uint8", 0, 1)
        if self.pack is None:
            # (the oracle has no bfloat16; uint16 carries its raw bits through the same codecs)
            otype = "uint16" if self.enc_type == "bfloat16" else self.enc_type
            self.oracle = O.OracleChain.from_metadata(self.stripped, otype, self.enc_fill, ndim)

    def encode_values(self, a):
        for c, dt in self.steps:
            a = _apply_encode(a, c, dt)
        return a

    def decode_values(self, e):
        for c, _ in reversed(self.steps):
            e = _apply_decode(e, c)
        return e

    def encode(self, a):
        e = self.encode_values(np.ascontiguousarray(a))
        if self.pack is None:
            return self.oracle.encode(e)
        for order in self.orders:
            e = np.ascontiguousarray(e.transpose(order))
        packed = packbits_encode(e, self.enc_type, **self.pb)
        return self.oracle.encode(np.frombuffer(packed, np.uint8))

    def decode(self, enc, shape):
        shape = [int(s) for s in shape]
        if self.pack is None:
            return self.decode_values(self.oracle.decode(enc, shape))
        n = int(np.prod(shape))
        packed = self.oracle.decode(enc, [packbits_size(n, self.enc_type, **self.pb)]).tobytes()
        e = packbits_decode(packed, n, self.enc_type, **self.pb)
        axes = list(range(len(shape)))  # encoded axis a <-> decoded axis axes[a]
        for order in self.orders:
            axes = [axes[o] for o in order]
        e = e.reshape([shape[a] for a in axes]).transpose(np.argsort(axes))
        return self.decode_values(np.ascontiguousarray(e))

    def decoded_fill(self, shape):
        """what a missing chunk decodes to: the decoded form of the encoded fill value"""
        return self.decode_values(np.full(shape, self.enc_fill, NP[self.enc_type]))
