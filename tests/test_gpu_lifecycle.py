"""Object lifetimes across the C ABI: a context outlives the chains, plans and caches made on it, in
whatever order a garbage-collected binding (Python here, Rust's Drop in rust/zarrs_gpu) destroys them
(zgpu_ctx_refcount, include/zgpu.h). The round-4 bench died with SIGSEGV in __cxa_finalize after its
line was printed when contexts were closed while their chains and plans were still alive; the
subprocess cases below end the interpreter in exactly those states and require a clean exit."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODECS = [{"name": "transpose", "configuration": {"order": [2, 1, 0]}},
          {"name": "bytes", "configuration": {"endian": "big"}}]


def _chunk():
    a = np.random.default_rng(3).standard_normal((16, 16, 16)).astype(np.float32)
    return a, O.OracleChain.from_metadata(CODECS, "float32", 0.0, 3).encode(a)


def test_context_closed_before_chain_and_plan():
    import torch
    from zarrs_amd import CodecChain, Context, make_desc
    from zarrs_amd import _lib as L
    lib = L.load()
    a, enc = _chunk()
    ctx = Context(0)
    assert ctx.refcount() == 1
    chain = CodecChain.from_metadata(CODECS, "float32", 0.0, ctx)
    assert ctx.refcount() == 2
    d = torch.frombuffer(bytearray(enc), dtype=torch.uint8).cuda()
    descs = (L.ChunkDesc * 1)(make_desc(d, [16, 16, 16]))
    plan = C.c_void_p()
    L.check(lib.zgpu_plan_create(chain._h, 3, descs, 1, L.u64s([16, 16, 16]), L.ENC_DEVICE | L.OUT_DEVICE,
                                 C.byref(plan)))
    assert ctx.refcount() == 3
    raw = ctx._h
    ctx.close()  # the caller's reference only: the chain and the plan keep the context alive
    assert lib.zgpu_ctx_refcount(raw) == 2
    out = torch.empty((16, 16, 16), dtype=torch.float32, device="cuda")
    st = (C.c_int32 * 1)()
    L.check(lib.zgpu_plan_execute(plan, out.data_ptr(), st, None))
    assert st[0] == 0 and np.array_equal(out.cpu().numpy(), a)
    out.zero_()
    assert chain.decode_batch([make_desc(d, [16, 16, 16])], out, [16, 16, 16], enc_device=True) == [0]
    assert np.array_equal(out.cpu().numpy(), a)
    h = np.empty((16, 16, 16), np.float32)  # host in / host out, coalesced, on the closed handle's context
    assert chain.decode_batch_into([make_desc(np.frombuffer(enc, np.uint8), [16, 16, 16])], h, [0, 0, 0],
                                   [16, 16, 16], enc_device=False, coalesce=True) == [0]
    assert np.array_equal(h, a)
    lib.zgpu_plan_destroy(plan)
    assert lib.zgpu_ctx_refcount(raw) == 1
    del chain  # the last reference: the context is freed here


def test_cache_holds_its_context():
    from zarrs_amd import Context
    from zarrs_amd import _lib as L
    lib = L.load()
    ctx = Context(0)
    cache = C.c_void_p()
    L.check(lib.zgpu_cache_create(ctx._h, 1 << 20, C.byref(cache)))
    raw = ctx._h
    assert ctx.refcount() == 2
    ctx.close()
    assert lib.zgpu_ctx_refcount(raw) == 1
    lib.zgpu_cache_destroy(cache)


EXIT_CASES = {
    # contexts never closed, chains / plans alive at interpreter exit
    "leak_all": "pass",
    # context closed first, chain and plan dropped by the interpreter's teardown
    "ctx_first": "ctx.close()",
    # everything closed explicitly in the worst order
    "ordered_worst": "ctx.close(); lib.zgpu_plan_destroy(plan); del chain",
}


@pytest.mark.parametrize("case", sorted(EXIT_CASES))
def test_clean_interpreter_exit(case, tmp_path):
    a, enc = _chunk()
    np.save(tmp_path / "a.npy", a)
    (tmp_path / "enc.bin").write_bytes(enc)
    src = textwrap.dedent(f"""
        import ctypes as C, sys
        import numpy as np, torch
        sys.path.insert(0, {ROOT!r})
        from zarrs_amd import CodecChain, Context, make_desc
        from zarrs_amd import _lib as L
        from concurrent.futures import ThreadPoolExecutor
        lib = L.load()
        a = np.load({str(tmp_path / "a.npy")!r})
        enc = open({str(tmp_path / "enc.bin")!r}, "rb").read()
        ctx = Context(0)
        chain = CodecChain.from_metadata({CODECS!r}, "float32", 0.0, ctx)
        d = torch.frombuffer(bytearray(enc), dtype=torch.uint8).cuda()
        descs = (L.ChunkDesc * 1)(make_desc(d, [16, 16, 16]))
        plan = C.c_void_p()
        L.check(lib.zgpu_plan_create(chain._h, 3, descs, 1, L.u64s([16, 16, 16]), L.ENC_DEVICE | L.OUT_DEVICE,
                                     C.byref(plan)))
        out = torch.empty((16, 16, 16), dtype=torch.float32, device="cuda")
        L.check(lib.zgpu_plan_execute(plan, out.data_ptr(), None, None))
        def call(_):
            h = np.empty((16, 16, 16), np.float32)
            chain.decode_batch_into([make_desc(np.frombuffer(enc, np.uint8), [16, 16, 16])], h, [0, 0, 0],
                                    [16, 16, 16], enc_device=False, coalesce=True)
            return bool(np.array_equal(h, a))
        with ThreadPoolExecutor(8) as ex:
            assert all(ex.map(call, range(32)))
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), a)
        {EXIT_CASES[case]}
        print("done", flush=True)
    """)
    p = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, f"rc={p.returncode}\n{p.stderr[-2000:]}"
    assert p.stdout.strip().endswith("done")


C5_CODECS = [{"name": "bytes", "configuration": {"endian": "little"}},
             {"name": "numcodecs.shuffle", "configuration": {"elementsize": 2}},
             {"name": "zstd", "configuration": {"level": 3, "checksum": False}}]


def test_pinned_calls_keep_pools_bounded(monkeypatch):
    """200 zgpu_decode_pinned calls of varying batch and chunk sizes (the per-codec plugin's pattern that
    exhausted device memory in the round-5 C5 drop-in leg): every result bit-exact, the device and pinned
    pools' free blocks within their caps (ZGPU_POOL_CAP_MB / ZGPU_PINNED_CAP_MB, read at context
    creation), and the blocks in use back to the same level after every call (zgpu_ctx_pool_stats)."""
    from zarrs_amd import CodecChain, Context, make_desc
    monkeypatch.setenv("ZGPU_POOL_CAP_MB", "256")
    monkeypatch.setenv("ZGPU_PINNED_CAP_MB", "128")
    ctx = Context(0)
    chain = CodecChain.from_metadata(C5_CODECS, "uint16", 0, ctx)
    co = O.OracleChain.from_metadata(C5_CODECS, "uint16", 0, 3)
    rng = np.random.default_rng(11)
    lives, frees, hfrees, hlives = [], [], [], []
    for i in range(200):
        n, rows = 1 + (i * 7) % 8, 1 + (i * 13) % 48
        base = rng.integers(0, 64, size=(1, 64, 64), dtype=np.uint16)
        chunks = [(base + rng.integers(0, 3, size=(rows, 64, 64), dtype=np.uint16) * (k + 1)).astype(np.uint16)
                  for k in range(n)]
        encs = [co.encode(c) for c in chunks]
        descs = [make_desc(np.frombuffer(e, np.uint8), [rows, 64, 64], out_start=[k * rows, 0, 0])
                 for k, e in enumerate(encs)]
        out = np.empty((n * rows, 64, 64), np.uint16)
        st = chain.decode_pinned_into(descs, out, [0, 0, 0], [n * rows, 64, 64], coalesce=(i % 2 == 0))
        assert st == [0] * n, (i, st)
        assert np.array_equal(out, np.concatenate(chunks)), i
        s = ctx.pool_stats()
        lives.append(s["dev_live"])
        frees.append(s["dev_free"])
        hlives.append(s["host_live"])
        hfrees.append(s["host_free"])
    assert max(frees) <= 256 << 20, max(frees)
    assert max(hfrees) <= 128 << 20, max(hfrees)
    # nothing accumulates in use: the second half of the calls holds no more than the first half did
    assert max(lives[100:]) <= max(lives[:100]), (max(lives[:100]), max(lives[100:]))
    assert max(hlives[100:]) <= max(hlives[:100]), (max(hlives[:100]), max(hlives[100:]))
    ctx.release_cached()
    s = ctx.pool_stats()
    assert s["dev_free"] == 0 and s["host_free"] == 0, s
    del chain
    ctx.close()


# ---------------------------------------------------------------------------------------------------
# Call-scoped memory: the composed ("general") decode paths and the write path take their temporaries
# from the context's pools through one scoped owner (csrc/ctx.hpp Scratch), so a call leaves the pools'
# in-use level where it found it, whether it succeeds or a descriptor fails.
# ---------------------------------------------------------------------------------------------------
import value_codecs as V  # noqa: E402  (the numpy model of packbits / fixedscaleoffset, a helper module)

# The chains, the [16, 32, 32] array and the sub-selection are those of tests/test_gpu_general_chains.py
# (shard_crc_zstd, deep3, transpose_nested_zstd) and tests/test_gpu_value_codecs.py (fixedscaleoffset
# f32 -> u8 before a shard, packbits of bool), restated here so that the test files stay independent.
SHAPE = [16, 32, 32]
PARTIAL = ([3, 5, 7], [11, 20, 22])
WHOLE = ([0, 0, 0], SHAPE)
BYTES = {"name": "bytes", "configuration": {"endian": "little"}}
GZIP = {"name": "gzip", "configuration": {"level": 1}}
ZSTD = {"name": "zstd", "configuration": {"level": 3, "checksum": True}}
CRC = {"name": "crc32c"}


def sh(cs, inner, loc="end"):
    return {"name": "sharding_indexed",
            "configuration": {"chunk_shape": cs, "codecs": inner, "index_codecs": [BYTES, CRC], "index_location": loc}}


def packbits(first=None, last=None, padding="none"):
    cfg = {"padding_encoding": padding}
    if first is not None:
        cfg["first_bit"], cfg["last_bit"] = first, last
    return {"name": "packbits", "configuration": cfg}


FSO = {"name": V.FSO, "configuration": {"offset": 1000, "scale": 10, "dtype": "f4", "astype": "u1"}}
CHAINS = {
    "shard_crc_zstd": [sh([4, 8, 8], [BYTES, GZIP]), CRC, ZSTD],
    "deep3": [sh([8, 16, 16], [sh([4, 8, 8], [sh([2, 4, 4], [BYTES, GZIP])])])],
    "transpose_nested_zstd": [{"name": "transpose", "configuration": {"order": [2, 1, 0]}},
                              sh([8, 16, 8], [sh([4, 8, 4], [BYTES, GZIP])]),
                              {"name": "zstd", "configuration": {"level": 3, "checksum": False}}],
}
FSO_CODECS = [FSO, sh([4, 8, 8], [BYTES, GZIP])]
PACKBITS_CODECS = [packbits(padding="last_byte")]


def _general_array(seed, fill):
    """as tests/test_gpu_general_chains.py: rounded normals with two all-fill regions (omitted inner chunks)"""
    a = np.round(np.random.default_rng(seed).standard_normal(SHAPE) * 20 + (fill if fill > 100 else 0)).astype(np.float32)
    a[8:16, 0:16, 16:32] = fill
    a[0:2, 0:4, 0:4] = fill
    return a


def _tensor(torch, a):
    """a device tensor holding a's bytes (torch has no unsigned 16-bit element type)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view("<i2") if a.dtype == np.uint16 else a).copy()).cuda()


# name -> (codecs, data type, fill, selections, byte to flip, xor mask, status of the flipped stream)
# The flipped byte is one every read of the chunk goes through, whatever its selection: the zstd frame's
# content checksum, the outer shard index's crc32c, the zstd magic number, the packbits padding byte.
DECODE_CASES = {
    "shard_crc_zstd": (CHAINS["shard_crc_zstd"], "float32", 3, [PARTIAL], -1, 0xFF, "CORRUPT_STREAM"),
    "deep3": (CHAINS["deep3"], "float32", 3, [PARTIAL], -1, 0xFF, "INVALID_CHECKSUM"),
    "transpose_nested_zstd": (CHAINS["transpose_nested_zstd"], "float32", 3, [PARTIAL], 0, 0xFF, "CORRUPT_STREAM"),
    # value_general: descriptors that tile the output, then a partial selection (the stacked boxes)
    "fixedscaleoffset": (FSO_CODECS, "float32", 1001.23, [WHOLE, PARTIAL], -1, 0xFF, "INVALID_CHECKSUM"),
    "packbits_bool": (PACKBITS_CODECS, "bool", 0, [PARTIAL], -1, 0x02, "CORRUPT_STREAM"),
}


def _decode_case(name):
    """(array, encoded, expected decode, flipped stream): the models run once per case"""
    codecs, dt, fill, _, pos, mask, _ = DECODE_CASES[name]
    if name == "packbits_bool":
        a = np.random.default_rng(17).integers(0, 2, SHAPE, dtype=np.uint8).view(np.bool_)
    else:
        a = _general_array(sorted(DECODE_CASES).index(name), fill)
    mc = V.ModelChain(codecs, dt, fill, 3) if name in ("packbits_bool", "fixedscaleoffset") else \
        O.OracleChain.from_metadata(codecs, dt, fill, 3)
    enc = mc.encode(a)
    exp = mc.decode(enc, SHAPE)
    bad = bytearray(enc)
    bad[pos] ^= mask
    with pytest.raises((O.OracleError, V.PackBitsError)) as oe:  # the reference rejects the flipped stream too
        mc.decode(bytes(bad), SHAPE)
    return exp, enc, bytes(bad), getattr(oe.value, "status", None)


def _levels(ctx):
    s = ctx.pool_stats()
    return s["dev_live"], s["host_live"]


@pytest.fixture(scope="module")
def decode_cases():
    return {name: _decode_case(name) for name in DECODE_CASES}


@pytest.mark.parametrize("out_device", [True, False], ids=["dev_out", "host_out"])
@pytest.mark.parametrize("name", sorted(DECODE_CASES))
def test_general_decode_returns_its_scratch(decode_cases, name, out_device):
    import torch
    from zarrs_amd import CodecChain, Context, ZgpuError, make_desc
    from zarrs_amd import _lib as L
    codecs, dt, fill, sels, _, _, want_status = DECODE_CASES[name]
    exp, enc, bad, oracle_status = decode_cases[name]
    if oracle_status is not None:
        assert oracle_status == getattr(L, want_status)
    ctx = Context(0)
    ch = CodecChain.from_metadata(codecs, dt, fill, ctx)
    good_d = torch.frombuffer(bytearray(enc), dtype=torch.uint8).cuda()  # torch memory, not the pools'
    bad_d = torch.frombuffer(bytearray(bad), dtype=torch.uint8).cuda()
    for start, sub in sels:
        def output():
            h = np.zeros(sub, exp.dtype)
            return (torch.from_numpy(h.view(np.uint8)).cuda(), h.dtype) if out_device else (h, h.dtype)
        out, odt = output()
        before = _levels(ctx)
        st = ch.decode_batch([make_desc(good_d, SHAPE, start, sub)], out, sub, enc_device=True)
        assert _levels(ctx) == before, (name, start, "ok")
        got = out.cpu().numpy().view(odt) if out_device else out
        want = np.ascontiguousarray(exp[tuple(slice(s, s + n) for s, n in zip(start, sub))])
        assert st == [0] and got.tobytes() == want.tobytes(), (name, start)
        out, _ = output()
        before = _levels(ctx)
        with pytest.raises(ZgpuError) as ei:
            ch.decode_batch([make_desc(bad_d, SHAPE, start, sub)], out, sub, enc_device=True)
        assert _levels(ctx) == before, (name, start, "failed")
        assert ei.value.status == getattr(L, want_status), (name, start)
    del ch
    ctx.close()


ENC_SHAPE = [8, 16, 16]
ENCODE_CASES = {
    "fixed": (CODECS, "float32"),
    "gzip": ([BYTES, GZIP], "float32"),
    "shard_fixed": ([sh([4, 8, 8], [BYTES, CRC])], "float32"),
    "shard_gzip": ([sh([4, 8, 8], [BYTES, GZIP])], "float32"),
    "packbits": ([packbits(3, 12, "first_byte")], "uint16"),
    "fixedscaleoffset": ([FSO, BYTES, ZSTD], "float32"),
}


def _encode_array(dt):
    rng = np.random.default_rng(23)
    if dt == "uint16":
        return rng.integers(0, 1 << 16, ENC_SHAPE).astype(np.uint16)
    a = np.round(1000 + rng.standard_normal(ENC_SHAPE) * 5).astype(np.float32)
    a[0:4, 0:8, 0:8] = 0  # one all-fill inner chunk: omitted from a shard
    return a


@pytest.mark.parametrize("name", sorted(ENCODE_CASES))
def test_encode_returns_its_scratch(name):
    import torch
    from zarrs_amd import CodecChain, Context
    codecs, dt = ENCODE_CASES[name]
    a = _encode_array(dt)
    mc = V.ModelChain(codecs, dt, 0, 3)
    ctx = Context(0)
    ch = CodecChain.from_metadata(codecs, dt, 0, ctx)
    d = _tensor(torch, a)
    before = _levels(ctx)
    parts = ch.encode_chunks(d, ENC_SHAPE, [[0, 0, 0]])
    assert _levels(ctx) == before, name
    got = bytes(parts[0].cpu().numpy())
    # A compressor's or a shard's bytes need not equal the reference's (other matches, other layout of
    # equal content), so every case is held to what the reference decodes the GPU's bytes to: its own
    # decode of its own encoding, bit for bit; a fixed-size unsharded chain is also held bytewise.
    assert mc.decode(got, ENC_SHAPE).tobytes() == mc.decode(mc.encode(a), ENC_SHAPE).tobytes(), name
    if ch.encoded_size(ENC_SHAPE) >= 0 and "shard" not in name:
        assert got == mc.encode(a), name  # a fixed-size chain: bytewise
    del ch
    ctx.close()


def test_encode_pinned_returns_its_scratch():
    from zarrs_amd import CodecChain, Context
    from zarrs_amd import _lib as L
    lib = L.load()
    codecs = [sh([4, 8, 8], [BYTES, GZIP])]
    a = _encode_array("float32")
    oc = O.OracleChain.from_metadata(codecs, "float32", 0, 3)
    ctx = Context(0)
    ch = CodecChain.from_metadata(codecs, "float32", 0, ctx)
    before = _levels(ctx)
    p, n, r = C.c_void_p(), C.c_uint64(), C.c_void_p()
    L.check(lib.zgpu_encode_pinned(ch._h, 3, L.u64s(ENC_SHAPE), a.ctypes.data, C.byref(p), C.byref(n), C.byref(r)))
    try:
        enc = bytes((C.c_uint8 * n.value).from_address(p.value))
    finally:
        lib.zgpu_result_release(r)
    assert _levels(ctx) == before  # the result's pinned block went back with it
    assert oc.decode(enc, ENC_SHAPE).tobytes() == a.tobytes()
    del ch
    ctx.close()
