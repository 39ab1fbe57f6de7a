"""GPU decode, encode and store of cast_value chains (k_cast in kernels/value.hip, value_general and the
write path) against the exact model (tests/cast_value_model.py) composed with value_codecs and the CPU
oracle: bit for bit, every (source, target) pair x rounding mode x out_of_range, the composed paths, and
the elements that cannot be cast."""
import ctypes as C

import numpy as np
import pytest

import cast_value_model as M
import oracle as O
import value_codecs as V

pytestmark = pytest.mark.gpu

BYTES = {"name": "bytes", "configuration": {"endian": "little"}}
IDX = [BYTES, {"name": "crc32c"}]
ZSTD = {"name": "zstd", "configuration": {"level": 3, "checksum": True}}
GZIP = {"name": "gzip", "configuration": {"level": 1}}
CRC = {"name": "crc32c"}
CHUNK = [8, 16, 16]
SELS = (([0, 0, 0], CHUNK), ([1, 5, 7], [6, 9, 8]), ([5, 9, 1], [1, 1, 1]))
NOT_REPRESENTABLE = 13


def cv(data_type, **cfg):
    return {"name": M.NAME, "configuration": {"data_type": data_type, **cfg}}


def sh(cs, inner):
    return {"name": "sharding_indexed", "configuration": {"chunk_shape": cs, "codecs": inner, "index_codecs": IDX}}


def tr(order):
    return {"name": "transpose", "configuration": {"order": order}}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    return Context(0)


def test_the_status_is_named(ctx):
    from zarrs_amd import _lib as L
    assert L.CAST_NOT_REPRESENTABLE == NOT_REPRESENTABLE
    assert L.load().zgpu_status_name(NOT_REPRESENTABLE) == b"CAST_NOT_REPRESENTABLE"


# ---------------------------------------------------------------------------------------------------
# the kernel against the model
# ---------------------------------------------------------------------------------------------------
def chain(ctx, codec, data_type):
    from zarrs_amd import CodecChain
    return CodecChain.from_metadata([codec, BYTES], data_type, bytes(M.size_of(data_type)), ctx)


def tensor_of(torch, data, t, lead=0):
    """a device tensor of the element size of t holding `data`, its base `lead` elements past an allocation"""
    size = M.size_of(t)
    a = np.frombuffer(bytes(lead * size) + data, {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[size])
    return torch.from_numpy(a.copy()).cuda()[lead:]


def gpu_encode(ch, torch, data, t, shape=None, lead=0):
    """(encoded bytes, None) or (None, (status, message))"""
    from zarrs_amd import ZgpuError
    x = tensor_of(torch, data, t, lead)
    shape = shape or [x.numel()]
    try:
        parts = ch.encode_chunks(x.reshape(shape), shape, [[0] * len(shape)])
    except ZgpuError as e:
        return None, (e.status, str(e))
    return bytes(parts[0].cpu().numpy()), None


def gpu_decode(ch, data, enc_t, t, shape=None):
    """(decoded bytes, status) of one whole chunk of elements of the encoded type enc_t, decoded to t"""
    from zarrs_amd import _lib as L
    from zarrs_amd import make_desc
    n = len(data) // M.size_of(enc_t)
    shape = shape or [n]
    out = np.zeros(n * M.size_of(t), np.uint8)
    desc = make_desc(data, shape)  # (keeps the encoded bytes alive through the call)
    arr = (L.ChunkDesc * 1)(desc)
    st = (C.c_int32 * 1)()
    rc = L.load().zgpu_decode_batch(ch._h, len(shape), arr, 1, out.ctypes.data, L.u64s(shape), 0, st, None)
    assert rc == st[0]
    return out.tobytes(), st[0]


def configurations(encoded_type):
    for r in M.ROUNDINGS:
        for oor in (None, "clamp") + (() if M.is_float(encoded_type) else ("wrap",)):
            yield r, oor


@pytest.mark.parametrize("s", M.TYPES)
def test_encode_every_target_against_the_model(ctx, torch_cuda, s):
    """k_cast<s, t> as the encode of a [cast_value(t), bytes] chain on an array of type s"""
    edges = M.edge_elements(s)
    for t in M.TYPES:
        for r, oor in configurations(t):
            codec = cv(t, rounding=r, **({"out_of_range": oor} if oor else {}))
            ch = chain(ctx, codec, s)
            clean = M.error_free(edges, s, t, r, oor)
            assert len(clean) >= 4
            for elems in (edges, clean):
                want, bad = M.cast_list(elems, s, t, r, oor)
                got, err = gpu_encode(ch, torch_cuda, M.to_bytes(elems, s), s)
                if bad is None:
                    assert err is None and got == M.to_bytes(want, t), (s, t, r, oor)
                else:
                    assert got is None and err[0] == NOT_REPRESENTABLE and f"element {bad} " in err[1], (s, t, r, oor, err)


@pytest.mark.parametrize("s", M.TYPES)
def test_decode_every_target_against_the_model(ctx, torch_cuda, s):
    """k_cast<s, t> as the decode of a [cast_value(s), bytes] chain on an array of type t: the same
    rounding and out_of_range, source and target swapped (wrap: only where the encoded type s is an
    integer, which is where a float target meets it)"""
    edges = M.edge_elements(s)
    for t in M.TYPES:
        for r, oor in configurations(s):
            codec = cv(s, rounding=r, **({"out_of_range": oor} if oor else {}))
            ch = chain(ctx, codec, t)
            clean = M.error_free(edges, s, t, r, oor)
            assert len(clean) >= 4
            for elems in (edges, clean):
                want, bad = M.cast_list(elems, s, t, r, oor)
                got, st = gpu_decode(ch, M.to_bytes(elems, s), s, t)
                if bad is None:
                    assert st == 0 and got == M.to_bytes(want, t), (s, t, r, oor)
                else:
                    assert st == NOT_REPRESENTABLE, (s, t, r, oor)


COUNTS = [1, 15, 16, 17, 4097]


@pytest.mark.parametrize("s", M.TYPES)
def test_counts_alignment_and_rank(ctx, torch_cuda, s):
    """1, 15, 16, 17 and 4097 elements (a tail; an odd count of the wider type), a [5, 7, 3] chunk, and a
    device input that starts one element past a 16-byte boundary: the vector path and the element path"""
    base = M.edge_elements(s)
    for k, t in enumerate(M.TYPES):
        r = M.ROUNDINGS[k % 5]
        codec = cv(t, rounding=r, out_of_range="clamp")
        ch = chain(ctx, codec, s)
        clean = M.error_free(base, s, t, r, "clamp")
        want1 = M.cast_list(clean, s, t, r, "clamp")[0]
        back = M.error_free(want1, t, s, r, "clamp")
        back_want = M.cast_list(back, t, s, r, "clamp")[0]
        for n, shape in [(c, None) for c in COUNTS] + [(105, [5, 7, 3])]:
            reps = -(-n // len(clean))
            elems, want = (clean * reps)[:n], (want1 * reps)[:n]
            for lead in (0, 1):
                got, err = gpu_encode(ch, torch_cuda, M.to_bytes(elems, s), s, shape, lead)
                assert err is None and got == M.to_bytes(want, t), (s, t, n, lead)
            reps = -(-n // len(back))
            got, st = gpu_decode(ch, M.to_bytes((back * reps)[:n], t), t, s, shape)
            assert st == 0 and got == M.to_bytes((back_want * reps)[:n], s), (s, t, n)


def test_a_failure_far_into_a_large_array_names_the_first_index(ctx, torch_cuda):
    """many blocks, failures in several of them: the smallest index wins"""
    n = 300001
    a = np.arange(n, dtype="<f8") % 1000
    a[[123457, 123456, 299999]] = np.nan
    ch = chain(ctx, cv("int16"), "float64")
    got, err = gpu_encode(ch, torch_cuda, a.tobytes(), "float64")
    assert got is None and err[0] == NOT_REPRESENTABLE and "element 123456 " in err[1]


# ---------------------------------------------------------------------------------------------------
# paths
# ---------------------------------------------------------------------------------------------------
F32_U8 = cv("uint8", out_of_range="clamp", scalar_map={"encode": [["NaN", 0]], "decode": [[0, "NaN"]]})
F64_I16 = cv("int16", rounding="nearest-away")
PAIRS = {"f32_u8": ("float32", F32_U8, "NaN"), "f64_i16": ("float64", F64_I16, 0.0)}
FSO = {"name": V.FSO, "configuration": {"offset": 100, "scale": 10, "dtype": "f4"}}
BITROUND = {"name": "bitround", "configuration": {"keepbits": 5}}
PLACES = {
    "bytes_zstd": lambda c: [c, BYTES, ZSTD],
    "before_shard": lambda c: [c, sh([4, 8, 8], [BYTES, GZIP])],
    "inside_shard": lambda c: [sh([4, 8, 8], [c, BYTES, ZSTD])],
    "between_transposes": lambda c: [tr([2, 0, 1]), c, tr([1, 0, 2]), sh([4, 8, 8], [BYTES, CRC])],
}


def _array(pair, seed):
    data_type, _, fill = PAIRS[pair]
    rng = np.random.default_rng(seed)
    if pair == "f32_u8":
        a = (rng.standard_normal(CHUNK) * 90 + 120).astype("<f4")  # some below 0 and above 255: clamped
        flat = a.reshape(-1)
        flat[rng.choice(flat.size, 60, replace=False)] = np.tile(np.array([np.nan, 0.5, 1.5, 2.5, 254.5, 1e30], "<f4"), 10)
    else:
        a = (rng.standard_normal(CHUNK) * 9000).astype("<f8").clip(-32768, 32767)
        flat = a.reshape(-1)
        flat[rng.choice(flat.size, 60, replace=False)] = np.tile(np.array([0.5, -0.5, 2.5, -2.5, 32767.49, -32768.49]), 10)
    a[4:8, 8:16, 0:8] = np.array([float(fill)], a.dtype)[0]  # a whole inner chunk at the fill value: omitted
    return a


def _src(enc, torch, hbm):
    return torch.frombuffer(bytearray(enc), dtype=torch.uint8).cuda() if hbm else enc


def check_decode(ch, torch, enc, exp, tag):
    from zarrs_amd import make_desc
    for hbm in (True, False):
        src = _src(enc, torch, hbm)
        for start, sub in SELS:
            out = np.zeros(sub, exp.dtype)
            assert ch.decode_batch([make_desc(src, CHUNK, start, sub)], out, sub, enc_device=hbm) == [0]
            want = np.ascontiguousarray(exp[tuple(slice(s, s + n) for s, n in zip(start, sub))])
            assert out.tobytes() == want.tobytes(), (tag, hbm, start, sub)


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_decode_paths(ctx, torch_cuda, pair, place):
    from zarrs_amd import CodecChain, make_desc
    data_type, codec, fill = PAIRS[pair]
    codecs = PLACES[place](codec)
    a = _array(pair, 3)
    mc = M.CastModelChain(codecs, data_type, fill, 3)
    enc = mc.encode(a)
    exp = mc.decode(enc, CHUNK)
    assert exp.dtype == a.dtype and exp.tobytes() != a.tobytes()
    ch = CodecChain.from_metadata(codecs, data_type, fill, ctx)
    check_decode(ch, torch_cuda, enc, exp, (pair, place))
    # a missing chunk (and, in a shard, the omitted inner chunk) decodes to the decoded encoded fill value
    gone = mc.decoded_fill([1])
    if "shard" in place:
        assert exp[5, 9, 3].tobytes() == gone.tobytes()
    for hbm in (True, False):
        out = np.zeros([16, 16, 16], a.dtype)
        descs = [make_desc(_src(enc, torch_cuda, hbm), CHUNK, out_start=[0, 0, 0]),
                 make_desc(None, CHUNK, [1, 0, 0], [6, 16, 16], [8, 0, 0])]
        assert ch.decode_batch(descs, out, [16, 16, 16], enc_device=hbm) == [0, 0]
        assert out[:8].tobytes() == exp.tobytes()
        assert out[8:14].tobytes() == mc.decoded_fill([6, 16, 16]).tobytes()
        assert not out[14:].any()


# (the write path takes no transpose before sharding_indexed, with or without a value codec: the
# transposes stand around the cast over a plain bytes codec instead)
ENCODE_PLACES = {k: v for k, v in PLACES.items() if k != "between_transposes"}
ENCODE_PLACES["between_transposes_bytes"] = lambda c: [tr([2, 0, 1]), c, tr([1, 0, 2]), BYTES, CRC]


@pytest.mark.parametrize("place", sorted(ENCODE_PLACES))
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_encode_paths(ctx, torch_cuda, pair, place):
    from zarrs_amd import CodecChain
    data_type, codec, fill = PAIRS[pair]
    codecs = ENCODE_PLACES[place](codec)
    a = _array(pair, 4)
    mc = M.CastModelChain(codecs, data_type, fill, 3)
    ch = CodecChain.from_metadata(codecs, data_type, fill, ctx)
    parts = ch.encode_chunks(torch_cuda.from_numpy(a.copy()).cuda(), CHUNK, [[0, 0, 0]])
    got = bytes(parts[0].cpu().numpy())
    want = mc.encode_values(a)
    assert mc.oracle.decode(got, CHUNK).tobytes() == want.view(V.NP[mc.otype]).tobytes(), (pair, place)


@pytest.mark.parametrize("first", ["fso", "bitround"])
def test_other_value_codecs_compose(ctx, torch_cuda, first):
    from zarrs_amd import CodecChain
    codecs = [FSO if first == "fso" else BITROUND, cv("int16", rounding="towards-negative", out_of_range="clamp"),
              sh([4, 8, 8], [BYTES, ZSTD])]
    rng = np.random.default_rng(8)
    a = (rng.standard_normal(CHUNK) * 400 + 100).astype("<f4")
    a[0:4, 0:8, 8:16] = 100.0
    mc = M.CastModelChain(codecs, "float32", 100.0, 3)
    assert mc.enc_type == "int16" and len(mc.steps) == 2
    enc = mc.encode(a)
    exp = mc.decode(enc, CHUNK)
    ch = CodecChain.from_metadata(codecs, "float32", 100.0, ctx)
    check_decode(ch, torch_cuda, enc, exp, first)
    parts = ch.encode_chunks(torch_cuda.from_numpy(a.copy()).cuda(), CHUNK, [[0, 0, 0]])
    assert mc.oracle.decode(bytes(parts[0].cpu().numpy()), CHUNK).tobytes() == mc.encode_values(a).tobytes()


# ---------------------------------------------------------------------------------------------------
# elements that cannot be cast
# ---------------------------------------------------------------------------------------------------
def _statuses(ch, descs, out, shape, hbm):
    from zarrs_amd import _lib as L
    arr = (L.ChunkDesc * len(descs))(*descs)
    st = (C.c_int32 * len(descs))()
    flags = (L.ENC_DEVICE if hbm else 0)
    rc = L.load().zgpu_decode_batch(ch._h, len(shape), arr, len(descs), out.ctypes.data, L.u64s(shape), flags, st, None)
    return rc, list(st)


@pytest.mark.parametrize("place", ["bytes_zstd", "inside_shard"])
def test_decode_failure_is_its_descriptors_alone(ctx, torch_cuda, place):
    """int8 data stored as uint8 (no out_of_range: encoding produces 0..127 only). A stored chunk with 200
    in it cannot come from encoding and cannot be decoded; with out_of_range = wrap it decodes to -56."""
    from zarrs_amd import CodecChain, make_desc
    from zarrs_amd import _lib as L
    codecs = PLACES[place](cv("uint8"))
    stored = O.OracleChain.from_metadata([BYTES, ZSTD] if place == "bytes_zstd" else [sh([4, 8, 8], [BYTES, ZSTD])],
                                         "uint8", 0, 3)
    rng = np.random.default_rng(5)
    good = [rng.integers(0, 128, CHUNK).astype(np.uint8) for _ in range(2)]
    bad = rng.integers(0, 128, CHUNK).astype(np.uint8)
    bad[5, 9, 3] = 200
    e_good, e_bad = [stored.encode(g) for g in good], stored.encode(bad)
    corrupt = bytearray(stored.encode(good[0]))
    pos = 0 if place == "bytes_zstd" else bytes(corrupt).index(b"\x28\xb5\x2f\xfd")
    corrupt[pos] ^= 0xFF  # the first zstd frame's magic number
    ch = CodecChain.from_metadata(codecs, "int8", 0, ctx)
    for hbm in (True, False):
        out = np.full([40, 16, 16], 77, np.int8)
        descs = [make_desc(_src(e_good[0], torch_cuda, hbm), CHUNK, out_start=[0, 0, 0]),
                 make_desc(_src(e_bad, torch_cuda, hbm), CHUNK, out_start=[8, 0, 0]),
                 make_desc(_src(e_good[1], torch_cuda, hbm), CHUNK, out_start=[16, 0, 0]),
                 make_desc(_src(bytes(corrupt), torch_cuda, hbm), CHUNK, out_start=[24, 0, 0]),
                 make_desc(_src(e_bad, torch_cuda, hbm), CHUNK, [0, 0, 4], [8, 16, 12], [32, 0, 0])]  # avoids [5, 9, 3]
        rc, st = _statuses(ch, descs, out, [40, 16, 16], hbm)
        assert st == [0, NOT_REPRESENTABLE, 0, L.CORRUPT_STREAM, 0] and rc == NOT_REPRESENTABLE, (place, hbm)
        assert out[0:8].tobytes() == good[0].astype(np.int8).tobytes()
        assert out[16:24].tobytes() == good[1].astype(np.int8).tobytes()
        assert out[32:40, :, :12].tobytes() == np.ascontiguousarray(bad[:, :, 4:]).astype(np.int8).tobytes()
        assert (out[32:40, :, 12:] == 77).all()
        # the one bad voxel alone, and its neighbour alone
        one = np.zeros([1, 1, 2], np.int8)
        rc, st = _statuses(ch, [make_desc(_src(e_bad, torch_cuda, hbm), CHUNK, [5, 9, 3], [1, 1, 1]),
                                make_desc(_src(e_bad, torch_cuda, hbm), CHUNK, [5, 9, 4], [1, 1, 1], [0, 0, 1])],
                           one, [1, 1, 2], hbm)
        assert st == [NOT_REPRESENTABLE, 0] and one[0, 0, 1] == bad[5, 9, 4]
    wrapping = CodecChain.from_metadata(PLACES[place](cv("uint8", out_of_range="wrap")), "int8", 0, ctx)
    out = np.zeros(CHUNK, np.int8)
    assert wrapping.decode_batch([make_desc(e_bad, CHUNK)], out, CHUNK, enc_device=False) == [0]
    assert out[5, 9, 3] == -56 and out.tobytes() == bad.view(np.int8).tobytes()


def test_encode_failure_fails_the_call(ctx, torch_cuda):
    from zarrs_amd import CodecChain, ZgpuError
    a = (np.arange(int(np.prod(CHUNK)), dtype="<f4") % 300).reshape(CHUNK)
    a[3, 7, 11] = np.nan
    index = (3 * 16 + 7) * 16 + 11
    x = torch_cuda.from_numpy(a).cuda()
    for codecs in ([cv("int16"), BYTES, ZSTD], [cv("int16"), sh([4, 8, 8], [BYTES, ZSTD])]):
        ch = CodecChain.from_metadata(codecs, "float32", 0.0, ctx)
        with pytest.raises(ZgpuError) as ei:
            ch.encode_chunks(x, CHUNK, [[0, 0, 0]])
        assert ei.value.status == NOT_REPRESENTABLE and f"element {index} " in str(ei.value)
        mapped = [cv("int16", scalar_map={"encode": [["NaN", -1]]})] + codecs[1:]
        mc = M.CastModelChain(mapped, "float32", 0.0, 3)
        ch = CodecChain.from_metadata(mapped, "float32", 0.0, ctx)
        parts = ch.encode_chunks(x, CHUNK, [[0, 0, 0]])
        got = mc.oracle.decode(bytes(parts[0].cpu().numpy()), CHUNK)
        assert got[3, 7, 11] == -1 and got.tobytes() == mc.encode_values(a).tobytes()


# ---------------------------------------------------------------------------------------------------
# surfaces
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codecs", [[cv("int16"), BYTES], [sh([4, 8, 8], [cv("int16"), BYTES])]], ids=["plain", "sharded"])
def test_plans_refuse_cast_value_chains(ctx, torch_cuda, codecs):
    from zarrs_amd import CodecChain, make_desc
    from zarrs_amd import _lib as L
    ch = CodecChain.from_metadata(codecs, "float32", 0, ctx)
    src = torch_cuda.zeros(1 << 16, dtype=torch_cuda.uint8, device="cuda")
    descs = (L.ChunkDesc * 1)(make_desc(src, CHUNK))
    plan = C.c_void_p()
    rc = L.load().zgpu_plan_create(ch._h, 3, descs, 1, L.u64s(CHUNK), L.ENC_DEVICE | L.OUT_DEVICE, C.byref(plan))
    assert rc == L.UNSUPPORTED and not plan.value
    assert "fused plan" in L.last_error()


# the geometry of tests/test_gpu_store.py at half the extent (the exact model runs element by element):
# whole array, one covered chunk, a straddling box, a slab, one voxel in the last (partial) chunk, a thin slab
A3, C3 = [10, 17, 20], [4, 8, 8]
SUBSETS3 = [([0, 0, 0], [10, 17, 20]), ([4, 8, 8], [4, 8, 8]), ([1, 2, 3], [6, 10, 11]), ([0, 0, 0], [10, 17, 9]),
            ([9, 16, 19], [1, 1, 1]), ([0, 0, 1], [10, 17, 2])]


@pytest.mark.parametrize("device", [False, True], ids=["host", "hbm"])
def test_store_array_subset_unsharded(ctx, torch_cuda, device):
    """as tests/test_gpu_store.py::test_unsharded_subsets holds its fso_zstd case: the model's actions,
    keys, counters and every written chunk, decoded here through the cast_value model"""
    import store_model as SM
    from test_gpu_store import Rig, random_data

    class CastRig(Rig):
        def __init__(self, codecs, data_type, fill, seeded):
            from zarrs_amd import Array, DeviceStore, MemoryStore, fill_value_bytes
            self.torch, self.device, self.nd = torch_cuda, device, 3
            self.meta = {"shape": A3, "data_type": data_type, "fill_value": fill, "codecs": codecs,
                         "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": C3}}}
            fb = fill_value_bytes(data_type, fill)
            self.mc = M.CastModelChain(codecs, data_type, fill, 3)
            self.dtype = np.dtype(V.NP[data_type])
            rt = lambda a: self.mc.decode(self.mc.encode(a), list(a.shape))  # noqa: E731
            self.model = SM.StoreModel(A3, C3, self.dtype, fb, None, rt, self.mc.decoded_fill([1])[0])
            self.store = DeviceStore() if device else MemoryStore()
            self.arr = Array(self.store, self.meta, ctx)
            if seeded:
                raw = random_data(self.dtype, self.model.padded.shape, 1)
                self.model.fill_from(raw)
                for idx in self.model.chunks():
                    if idx in self.model.keys():
                        self.put(idx, self.mc.encode(raw[self.model.chunk_box(idx)]))

    codecs = [cv("int16"), BYTES, {"name": "zstd", "configuration": {"level": 3}}]
    for seeded in (False, True):
        rig = CastRig(codecs, "float32", 0.0, seeded)
        for k, (start, shape) in enumerate(SUBSETS3):
            r, _, _ = rig.apply(start, random_data(rig.dtype, shape, 100 + k))
            assert r["actions"]
        rig.read_back()
    # an element that cannot be cast fails the store, and nothing is written
    from zarrs_amd import ZgpuError
    rig = CastRig(codecs, "float32", 0.0, False)
    data = random_data(rig.dtype, C3, 9)
    data[1, 2, 3] = np.inf
    with pytest.raises(ZgpuError) as ei:
        rig.arr.store_array_subset(C3, rig.give(data))
    assert ei.value.status == NOT_REPRESENTABLE and not rig.snapshot()


def test_store_inside_sharding_is_unsupported(ctx, torch_cuda):
    from zarrs_amd import Array, MemoryStore, ZgpuError
    from zarrs_amd import _lib as L
    meta = {"shape": [20, 33, 40], "data_type": "float32", "fill_value": 0.0,
            "codecs": [sh([4, 8, 8], [cv("int16"), BYTES])],
            "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": CHUNK}}}
    arr = Array(MemoryStore(), meta, ctx)
    with pytest.raises(ZgpuError) as e:
        arr.store_array_subset([0, 0, 0], np.ones([20, 33, 40], np.float32))
    assert e.value.status == L.UNSUPPORTED and not arr.store
