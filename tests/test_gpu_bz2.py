"""numcodecs.bz2 on the GPU (kernels/bz2.hip): the reference fixtures, streams libbz2 wrote, the
hand-built streams of bz2_streams.py (test_bz2_streams_model.py holds them to libbz2), size mismatches,
chains, the scratch budget's rounds, and the codec's boundary. Every comparison is bit-exact; the
checker is Python's bz2 module. All of it fails without the codec: chain creation is then UNSUPPORTED."""
import bz2
import ctypes as C
import os
import struct

import numpy as np
import pytest

import bz2_streams as S
import fixtures as F
import oracle as O
from test_gpu_checksum_zlib import _shard, _sharding, run_batch

pytestmark = pytest.mark.gpu

BYTES_LE = {"name": "bytes", "configuration": {"endian": "little"}}
STATUS = {S.OK: 0, S.CORRUPT: 4, S.SIZE: 2}


def BZ2(level=9, name="numcodecs.bz2"):
    return {"name": name, "configuration": {"level": level}}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def u8(ctx):
    from zarrs_amd import CodecChain
    return CodecChain.from_metadata([BYTES_LE, BZ2()], "uint8", 0, ctx)


@pytest.fixture(scope="module")
def families():
    return S.families()


def blocks_counter():
    from zarrs_amd import _lib as L
    return L.last_counters()["bz2_blocks"]


def rounds_counter():
    """Rounds of the bz2 stage in this thread's last call (a whole-shard stage: summed over its regrown runs)."""
    from zarrs_amd import _lib as L
    return L.last_counters()["bz2_rounds"]


# ---- reference fixtures ------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["host", "hbm"])
def test_v3_reference_fixture(ctx, torch_cuda, store):
    from zarrs_amd import Array, DeviceStore, MemoryStore
    meta, chunks = F.load_array("v3_zarr_python/array_bz2.zarr")
    full = {"shape": meta["shape"], "data_type": meta["data_type"], "fill_value": meta["fill_value"],
            "codecs": meta["codecs"], "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": meta["chunk_shape"]}}}
    ms = MemoryStore({"c/" + "/".join(map(str, k)): v for k, v in chunks.items()})
    arr = Array(DeviceStore.from_store(ms) if store == "hbm" else ms, full, ctx)
    got = arr.retrieve_array_subset()
    exp = np.zeros((10, 10), np.float32)
    for (i, j), enc in chunks.items():
        exp[5 * i:5 * i + 5, 5 * j:5 * j + 5] = np.frombuffer(bz2.decompress(enc), "<f4").reshape(5, 5)
    assert len(chunks) == 4 and np.array_equal(got, exp)
    m, none = F.load_array("v3_zarr_python/array_none.zarr")
    nm = {"shape": m["shape"], "data_type": m["data_type"], "fill_value": m["fill_value"], "codecs": m["codecs"],
          "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": m["chunk_shape"]}}}
    plain = Array(MemoryStore({"c/" + "/".join(map(str, k)): v for k, v in none.items()}), nm, ctx)
    assert np.array_equal(got, plain.retrieve_array_subset())
    assert np.array_equal(arr.retrieve_array_subset([1, 2], [6, 5]), exp[1:7, 2:7])


def test_v2_reference_fixture(ctx, torch_cuda):
    from zarrs_amd import CodecChain
    base = os.path.join(F.REF, "v2", "array_bz2_C.zarr")
    ch = CodecChain.from_metadata([BYTES_LE, BZ2(9)], "float32", 0, ctx)
    whole = np.zeros((10, 10), np.float32)
    for i in range(2):
        for j in range(2):
            enc = open(os.path.join(base, f"{i}.{j}"), "rb").read()
            exp = np.frombuffer(bz2.decompress(enc), "<f4").reshape(5, 5)
            assert np.array_equal(ch.decode(enc, [5, 5]), exp)
            whole[5 * i:5 * i + 5, 5 * j:5 * j + 5] = exp
    assert np.array_equal(whole, np.arange(100, dtype=np.float32).reshape(10, 10))


# ---- streams made by libbz2 --------------------------------------------------------------------
def content(kind, n, seed=0):
    rng = np.random.default_rng(seed + n)
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "zeros":
        return bytes(n)
    if kind == "ff":
        return b"\xff" * n
    if kind == "shuffled_u16":  # a u16 ramp image with noise, byte-shuffled: the low plane, then the high plane
        m = (n + 1) // 2
        img = (np.arange(m) // 7 + rng.integers(0, 9, m)).astype("<u2")
        return np.frombuffer(img.tobytes(), np.uint8).reshape(m, 2).T.tobytes()[:n]
    return bytes(rng.choice(np.frombuffer(b"acgt \n", np.uint8), n, p=[.3, .25, .2, .15, .07, .03]))


KINDS = ["random", "zeros", "ff", "shuffled_u16", "text"]
# 99,981 is the first size that does not fit level 1's block (100,000 - 19 symbols)
SMALL = [0, 1, 3, 4, 5, 259, 260, 4096, 99980, 99981, 99982]


@pytest.mark.parametrize("level", [1, 9])
@pytest.mark.parametrize("kind", KINDS)
def test_libbz2_streams(u8, torch_cuda, kind, level):
    for n in SMALL:
        d = content(kind, n)
        enc = bz2.compress(d, level)
        rc, st, got = run_batch(torch_cuda, u8, [enc, enc + b"\x00junk", enc], [n])
        assert rc == 0 and st == [0, 0, 0], (n, st)
        assert got.tobytes() == d * 3, n


@pytest.mark.parametrize("kind", KINDS)
def test_three_blocks_not_byte_aligned(u8, torch_cuda, kind):
    n = 250000
    d = content(kind, n)
    enc = bz2.compress(d, 1)
    rc, st, got = run_batch(torch_cuda, u8, [enc] * 2, [n])
    assert rc == 0 and st == [0, 0] and got.tobytes() == d * 2
    if kind in ("random", "text"):  # 250,000 symbols (and a few RLE1 counts) in blocks of 99,981
        assert blocks_counter() == 6
    rc, st, got = run_batch(torch_cuda, u8, [enc], [n])  # a lone item
    assert rc == 0 and st == [0] and got.tobytes() == d


def test_one_mib_random_level9_has_a_full_block(u8, torch_cuda):
    n = 1 << 20
    d = content("random", n)
    enc = bz2.compress(d, 9)
    rc, st, got = run_batch(torch_cuda, u8, [enc], [n])
    assert rc == 0 and st == [0] and got.tobytes() == d
    assert blocks_counter() == 2  # 900,000 - 19 symbols, then the rest


def test_one_mib_of_zeros(u8, torch_cuda):
    n = 1 << 20
    enc = bz2.compress(bytes(n), 9)
    assert len(enc) < 64
    rc, st, got = run_batch(torch_cuda, u8, [enc, enc], [n])
    assert rc == 0 and st == [0, 0] and not got.any() and got.size == 2 * n
    assert blocks_counter() == 2


# ---- hand-built families -----------------------------------------------------------------------
def run_family(torch, u8, cases, beside):
    """Every valid case, one batched call per decoded size, with the `beside` (corrupt) cases between them."""
    sizes = sorted({len(c.expect) for c in cases if c.status == S.OK})
    for size in sizes or [S.PAD]:
        batch = []
        for c in cases:
            if c.status != S.OK or len(c.expect) == size:
                batch.append(c)
        mixed = []
        for k, c in enumerate(batch):
            mixed.append(c)
            if beside:
                mixed.append(beside[k % len(beside)])
        rc, st, got = run_batch(torch, u8, [c.stream for c in mixed], [size])
        want = [STATUS[c.status] for c in mixed]
        assert st == want, [(c.name, s) for c, s, w in zip(mixed, st, want) if s != w]
        assert rc == next((w for w in want if w), 0)
        for k, c in enumerate(mixed):
            if c.status == S.OK:
                assert got[k * size:(k + 1) * size].tobytes() == c.expect, c.name


@pytest.mark.parametrize("family", ["tables", "groups", "runs", "mtf", "bwt", "rle1", "magic"])
def test_hand_built_family(u8, torch_cuda, families, family):
    corrupt = families["corrupt"]
    beside = [corrupt[k] for k in range(0, len(corrupt), 5)]
    run_family(torch_cuda, u8, families[family], beside)


def test_hand_built_corrupt_family(u8, torch_cuda, families):
    good = [c for c in families["tables"] if c.status == S.OK and len(c.expect) == S.PAD][:3]
    cases = families["corrupt"]
    assert len(cases) >= 25 and all(c.status == S.CORRUPT for c in cases)
    run_family(torch_cuda, u8, good + cases + good, [])


@pytest.mark.parametrize("family", ["tables", "rle1", "magic"])
def test_hand_built_lone_items(u8, torch_cuda, families, family):
    for c in families[family]:
        size = len(c.expect) if c.status == S.OK else S.PAD
        rc, st, got = run_batch(torch_cuda, u8, [c.stream], [size])
        assert st == [STATUS[c.status]] and rc == st[0], c.name
        if c.status == S.OK:
            assert got.tobytes() == c.expect, c.name


def test_block_magic_in_payload_is_not_a_block(u8, torch_cuda, families):
    (c,) = [c for c in families["magic"] if c.name == "block_magic_inside_the_payload"]
    rc, st, got = run_batch(torch_cuda, u8, [c.stream], [len(c.expect)])
    assert rc == 0 and got.tobytes() == c.expect
    assert blocks_counter() == c.n_blocks  # the candidate inside the payload is dropped


# ---- sizes -------------------------------------------------------------------------------------
def test_decoded_size_mismatch(u8, torch_cuda):
    from zarrs_amd import ZgpuError, _lib as L
    enc = bz2.compress(content("text", 1000), 9)
    for shape in (1001, 999):
        with pytest.raises(ZgpuError) as ei:
            u8.decode(enc, [shape])
        assert ei.value.status == L.DECODED_SIZE_MISMATCH
        assert L.last_size_mismatch() == (0, 1000, shape)
    with pytest.raises(ZgpuError) as ei:  # far past the slot: the length is only known to be larger
        u8.decode(bz2.compress(bytes(1 << 20)), [99])
    assert ei.value.status == L.DECODED_SIZE_MISMATCH and L.last_size_mismatch() == (0, None, 99)
    # the documented deviation: block records are sized with the slot (32 + slot / 32768), so a hand-made
    # stream of more one-byte blocks than that is reported as outgrowing its slot, never as unsupported
    few, many = S.stream([S.block_of(b"x")] * 30), S.stream([S.block_of(b"x")] * 40)
    assert bz2.decompress(few) == b"x" * 30 and bz2.decompress(many) == b"x" * 40
    assert bytes(u8.decode(few, [30])) == b"x" * 30 and blocks_counter() == 30
    with pytest.raises(ZgpuError) as ei:
        u8.decode(many, [40])
    assert ei.value.status == L.DECODED_SIZE_MISMATCH and L.last_size_mismatch() == (0, None, 40)
    good = bz2.compress(content("text", 999), 9)
    rc, st, got = run_batch(torch_cuda, u8, [good, enc, good], [999])
    assert rc == L.DECODED_SIZE_MISMATCH and st == [0, L.DECODED_SIZE_MISMATCH, 0]
    assert got[:999].tobytes() == content("text", 999) == got[1998:].tobytes()


# ---- chains ------------------------------------------------------------------------------------
def test_chain_bytes_bz2(ctx, torch_cuda):
    from zarrs_amd import CodecChain
    a = (np.random.default_rng(1).standard_normal((32, 32, 32)) * 20).astype(np.int16)
    enc = bz2.compress(a.astype("<i2").tobytes(), 5)
    ch = CodecChain.from_metadata([BYTES_LE, BZ2(5)], "int16", 0, ctx)
    assert np.array_equal(ch.decode(enc, [32, 32, 32]), a)
    sub = ch.partial_decode(enc, [32, 32, 32], [3, 0, 30], [7, 32, 2])  # decodes the chunk, scatters the part
    assert np.array_equal(sub, a[3:10, :, 30:32])
    alias = CodecChain.from_metadata([BYTES_LE, BZ2(5, "https://codec.zarrs.dev/bytes_to_bytes/bz2")], "int16", 0, ctx)
    assert np.array_equal(alias.decode(enc, [32, 32, 32]), a)


@pytest.mark.parametrize("shape,dt", [([5, 7, 3], "uint16"), ([31, 17], "float64")])
def test_chain_transpose_big_shuffle_bz2_crc32c(ctx, torch_cuda, shape, dt):
    from zarrs_amd import CodecChain, _lib as L
    es = np.dtype(dt).itemsize
    head = [{"name": "transpose", "configuration": {"order": list(range(len(shape)))[::-1]}},
            {"name": "bytes", "configuration": {"endian": "big"}},
            {"name": "numcodecs.shuffle", "configuration": {"elementsize": es}}]
    a = (np.random.default_rng(es).standard_normal(shape) * 300).astype(dt)
    inner = O.OracleChain.from_metadata(head, dt, 0, len(shape)).encode(a)
    z = bz2.compress(inner, 9)
    enc = z + struct.pack("<I", O.crc32c(z))
    ch = CodecChain.from_metadata(head + [BZ2(9), {"name": "crc32c"}], dt, 0, ctx)
    assert np.array_equal(ch.decode(enc, shape), a)
    bad = bytearray(enc)
    bad[-1] ^= 1
    rc, st, got = run_batch(torch_cuda, ch, [enc, bytes(bad), enc], shape, dtype=dt)
    assert rc == L.INVALID_CHECKSUM and st == [0, L.INVALID_CHECKSUM, 0]
    assert np.array_equal(got[:shape[0]], a) and np.array_equal(got[2 * shape[0]:], a)
    sub = ch.partial_decode(enc, shape, [1] * len(shape), [2] * len(shape))
    assert np.array_equal(sub, a[tuple(slice(1, 3) for _ in shape)])


def test_sharding_with_bz2_inner_chunks(ctx, torch_cuda):
    from zarrs_amd import CodecChain, _lib as L
    a = np.random.default_rng(11).integers(0, 500, (16, 16)).astype(np.uint16)
    a[8:, :8] = 7  # inner chunk 2 is left out of the shard: the fill value
    origins = [(0, 0), (0, 8), (8, 0), (8, 8)]
    inner = {k: bz2.compress(a[i:i + 8, j:j + 8].tobytes(), 9) for k, (i, j) in enumerate(origins) if k != 2}
    shard = _shard(inner, 4)
    ch = CodecChain.from_metadata([_sharding([8, 8], [BYTES_LE, BZ2(9)])], "uint16", 7, ctx)
    assert np.array_equal(ch.decode(shard, [16, 16]), a)
    assert np.array_equal(ch.partial_decode(shard, [16, 16], [2, 1], [13, 14]), a[2:15, 1:15])
    assert np.array_equal(ch.partial_decode(shard, [16, 16], [9, 9], [1, 1]), a[9:10, 9:10])
    broken = dict(inner)
    c = bytearray(broken[3])
    c[len(c) // 2] ^= 0x20
    broken[3] = bytes(c)
    rc, st, got = run_batch(torch_cuda, ch, [shard, _shard(broken, 4), shard], [16, 16], dtype=np.uint16)
    assert rc == L.CORRUPT_STREAM and st == [0, L.CORRUPT_STREAM, 0]
    assert np.array_equal(got[:16], a) and np.array_equal(got[32:], a)
    # the corrupt inner chunk fails only the reads that touch it
    rc, st, got = run_batch(torch_cuda, ch, [_shard(broken, 4)], [16, 16], dtype=np.uint16, sel=([0, 0], [8, 16]))
    assert rc == 0 and st == [0] and np.array_equal(got, a[:8])
    nested = CodecChain.from_metadata([_sharding([8, 8], [_sharding([4, 4], [BYTES_LE, BZ2(1)])])], "uint16", 0, ctx)
    mids = {}
    for k, (i, j) in enumerate(origins):
        leaves = {q: bz2.compress(a[i + di:i + di + 4, j + dj:j + dj + 4].tobytes(), 1)
                  for q, (di, dj) in enumerate([(0, 0), (0, 4), (4, 0), (4, 4)])}
        mids[k] = _shard(leaves, 4)
    assert np.array_equal(nested.decode(_shard(mids, 4), [16, 16]), a)


def test_bz2_after_sharding_regrows_its_slots(ctx, torch_cuda):
    """bz2 over a whole shard: the stream carries no size, so the slots start at 4x the encoded shard and
    grow 8x per DECODED_SIZE_MISMATCH; the second shard is far better than 4:1."""
    from zarrs_amd import CodecChain
    rng = np.random.default_rng(3)
    noisy = rng.integers(0, 60000, (32, 32)).astype(np.uint16)
    flat = np.zeros((32, 32), np.uint16)
    flat[:16, :16] = (np.arange(256) % 5).reshape(16, 16)
    ch = CodecChain.from_metadata([_sharding([16, 16], [BYTES_LE]), BZ2(9)], "uint16", 0, ctx)
    for a in (noisy, flat):
        inner = {k: a[i:i + 16, j:j + 16].tobytes() for k, (i, j) in enumerate([(0, 0), (0, 16), (16, 0), (16, 16)])}
        shard = _shard(inner, 4)
        enc = bz2.compress(shard, 9)
        assert (len(shard) > 4 * len(enc) + 256) == (a is flat)
        assert np.array_equal(ch.decode(enc, [32, 32]), a)
        # one run of the stage when the first slots (4x) hold the shard, one more per 8x regrow
        runs, cap = 1, max(4 * len(enc), 256)
        while (cap + 255) // 256 * 256 < len(shard):
            runs, cap = runs + 1, cap * 8
        assert rounds_counter() == runs and (runs > 1) == (a is flat)
        assert np.array_equal(ch.partial_decode(enc, [32, 32], [14, 14], [4, 4]), a[14:18, 14:18])


def test_whole_shard_of_many_small_blocks(ctx, torch_cuda):
    """A well-compressing level-1 shard: 42 blocks in under 4 KiB, so the first slot (4x the encoded bytes)
    has records for 32 magics only. That is a size mismatch like any other outgrown slot, and the
    regrowing goes on to a slot that holds both the records and the bytes."""
    from zarrs_amd import CodecChain
    a = (np.arange(1024 * 2048) % 5).astype(np.uint16).reshape(1024, 2048)
    a[::7, ::3] += 1
    inner = {k: a[i:i + 512, j:j + 1024].tobytes() for k, (i, j) in enumerate([(0, 0), (0, 1024), (512, 0), (512, 1024)])}
    shard = _shard(inner, 4)
    enc = bz2.compress(shard, 1)
    magics = S._bit_count(enc, S.BLOCK_MAGIC)
    assert magics > 33 and 32 + 4 * len(enc) // 32768 < magics  # more than the first slot's records
    ch = CodecChain.from_metadata([_sharding([512, 1024], [BYTES_LE]), BZ2(1)], "uint16", 0, ctx)
    assert np.array_equal(ch.decode(enc, [1024, 2048]), a)
    assert blocks_counter() == magics and rounds_counter() >= 3
    assert np.array_equal(ch.partial_decode(enc, [1024, 2048], [510, 1020], [4, 8]), a[510:514, 1020:1028])


def test_scratch_budget_rounds(ctx, torch_cuda, monkeypatch):
    """8 items of 1 MiB slots need 6.25 MiB of scratch each: a budget of 16 MiB holds two per round."""
    from zarrs_amd import CodecChain, _lib as L
    n = 1 << 20
    data = [content("shuffled_u16", n, seed=k) for k in range(8)]
    encs = [bz2.compress(d, 1) for d in data]
    bad = bytearray(encs[5])
    bad[11] ^= 4  # the first block's stored CRC (bits 80..111)
    monkeypatch.setenv("ZGPU_BZ2_SCRATCH_MB", "16")
    ch = CodecChain.from_metadata([BYTES_LE, BZ2(1)], "uint8", 0, ctx)
    rc, st, got = run_batch(torch_cuda, ch, encs[:5] + [bytes(bad)] + encs[6:], [n])
    assert rc == L.CORRUPT_STREAM and st == [0] * 5 + [L.CORRUPT_STREAM] + [0, 0]
    assert rounds_counter() == 4  # two items of 6.25 MiB (and their records) per 16 MiB
    for k in range(8):
        if k != 5:
            assert got[k * n:(k + 1) * n].tobytes() == data[k], k
    monkeypatch.delenv("ZGPU_BZ2_SCRATCH_MB")
    rc, st, got = run_batch(torch_cuda, ch, encs, [n])
    assert rc == 0 and st == [0] * 8 and got.tobytes() == b"".join(data)
    assert rounds_counter() == 1


def test_plan_executed_twice(u8, torch_cuda):
    from zarrs_amd import _lib as L, make_desc
    lib = L.load()
    n, k = 30000, 3
    data = [content("text", n, seed=s) for s in range(k)]
    encs = [bz2.compress(d, 1) for d in data]
    pitch = max(map(len, encs)) + 7
    blob = torch_cuda.frombuffer(bytearray(b"".join(e.ljust(pitch, b"\0") for e in encs)), dtype=torch_cuda.uint8).cuda()
    descs = [make_desc((blob.data_ptr() + i * pitch, len(encs[i])), [n], out_start=[i * n]) for i in range(k)]
    arr = (L.ChunkDesc * k)(*descs)
    plan = C.c_void_p()
    L.check(lib.zgpu_plan_create(u8._h, 1, arr, k, L.u64s([k * n]), L.ENC_DEVICE | L.OUT_DEVICE, C.byref(plan)))
    try:
        out = torch_cuda.zeros(k * n, dtype=torch_cuda.uint8, device="cuda")
        st = (C.c_int32 * k)()
        ctr = (C.c_uint64 * L.N_COUNTERS)()
        for _ in range(2):
            out.zero_()
            assert lib.zgpu_plan_execute(plan, out.data_ptr(), st, None) == 0 and list(st) == [0] * k
            assert out.cpu().numpy().tobytes() == b"".join(data)
            lib.zgpu_plan_counters(plan, ctr, L.N_COUNTERS)
            assert ctr[L.CTR_BZ2_BLOCKS] == k
        blob[pitch + 40] ^= 1  # item 1 corrupt in place; the plan's third execution reports it alone
        assert lib.zgpu_plan_execute(plan, out.data_ptr(), st, None) == L.CORRUPT_STREAM
        assert list(st) == [0, L.CORRUPT_STREAM, 0]
    finally:
        lib.zgpu_plan_destroy(plan)


def test_decode_files_and_host_input(u8, torch_cuda, tmp_path):
    from zarrs_amd import _lib as L, make_desc
    lib = L.load()
    n = 5000
    data = [content("text", n, seed=s) for s in range(3)]
    paths = []
    for k, d in enumerate(data):
        p = tmp_path / f"c{k}"
        p.write_bytes(b"pad" * k + bz2.compress(d, 9))
        paths.append(str(p).encode())
    descs = (L.ChunkDesc * 3)(*[make_desc((None, 0), [n], out_start=[k * n]) for k in range(3)])
    ranges = (L.FileRange * 3)(*[L.FileRange(paths[k], 3 * k, L.WHOLE) for k in range(3)])
    out = torch_cuda.zeros(3 * n, dtype=torch_cuda.uint8, device="cuda")
    st = (C.c_int32 * 3)()
    rc = lib.zgpu_decode_files(u8._h, 1, descs, ranges, 3, out.data_ptr(), L.u64s([3 * n]), L.OUT_DEVICE, st, None)
    assert rc == 0 and list(st) == [0, 0, 0] and out.cpu().numpy().tobytes() == b"".join(data)
    assert bytes(u8.decode(bz2.compress(data[0], 9), [n])) == data[0]  # host bytes in, host array out


def test_coalesced_calls(ctx, torch_cuda):
    """16 threads, one chunk each through ZGPU_COALESCE: the calls share batches (and the stage's scratch and
    rounds); one corrupt caller fails alone."""
    import threading
    from concurrent.futures import ThreadPoolExecutor
    from zarrs_amd import CodecChain, ZgpuError, make_desc, _lib as L
    n, k = 20000, 16
    data = [content("text", n, seed=s) for s in range(k)]
    encs = [bz2.compress(d, 1 + s % 9) for s, d in enumerate(data)]
    bad = bytearray(encs[7])
    bad[11] ^= 1  # the stored block CRC
    encs[7] = bytes(bad)
    ch = CodecChain.from_metadata([BYTES_LE, BZ2(9)], "uint8", 0, ctx)
    out = np.zeros((k, n), np.uint8)
    barrier = threading.Barrier(k)

    def one(i):
        barrier.wait()
        try:
            return ch.decode_batch_into([make_desc(encs[i], [1, n])], out, [i, 0], [1, n], enc_device=False,
                                        coalesce=True)
        except ZgpuError as e:
            return e.status
    ctx.set_coalescing(window_us=50000, max_calls=16)
    try:
        before = ctx.coalescing_stats()
        with ThreadPoolExecutor(k) as ex:
            res = list(ex.map(one, range(k)))
        after = ctx.coalescing_stats()
    finally:
        ctx.set_coalescing(window_us=200, max_calls=8)
    assert res == [[0]] * 7 + [L.CORRUPT_STREAM] + [[0]] * 8, res
    assert after["calls"] - before["calls"] == k and after["batches"] - before["batches"] < k
    for i in range(k):
        if i != 7:
            assert out[i].tobytes() == data[i], i


def test_plan_group(ctx, torch_cuda):
    """Two parts of different chunk shapes in one zgpu_group, executed twice; one corrupt chunk in part 1."""
    from zarrs_amd import CodecChain, PlanGroup, ZgpuError, make_desc
    ch = CodecChain.from_metadata([BYTES_LE, BZ2(9)], "uint16", 0, ctx)
    rng = np.random.default_rng(8)
    arrays = [rng.integers(0, 700, (4 * 16, 64)).astype(np.uint16), rng.integers(0, 9, (6 * 8, 32)).astype(np.uint16)]
    shapes = [[16, 64], [8, 32]]
    for corrupt in (None, (1, 4)):
        keep, parts, outs = [], [], []
        for p, (a, cs) in enumerate(zip(arrays, shapes)):
            descs = []
            for c in range(a.shape[0] // cs[0]):
                b = bytearray(bz2.compress(a[c * cs[0]:(c + 1) * cs[0]].tobytes(), 1 + c))
                if corrupt == (p, c):
                    b[11] ^= 2
                t = torch_cuda.frombuffer(b, dtype=torch_cuda.uint8).cuda()
                keep.append(t)
                descs.append(make_desc(t, cs, out_start=[c * cs[0], 0]))
            parts.append((ch, descs, list(a.shape)))
            outs.append(torch_cuda.zeros(a.shape, dtype=torch_cuda.int16, device="cuda"))
        g = PlanGroup(parts)
        try:
            if corrupt is None:
                for _ in range(2):
                    for o in outs:
                        o.zero_()
                    assert g.execute(outs) == [0] * 10
                    for a, o in zip(arrays, outs):
                        assert np.array_equal(o.cpu().numpy().view(np.uint16), a)
                assert g.counters()[7] == 10
            else:
                with pytest.raises(ZgpuError) as ei:
                    g.execute(outs)
                assert ei.value.status == 4
                st = list(g.status[:10])
                assert st == [0] * 8 + [4, 0]
                assert np.array_equal(outs[0].cpu().numpy().view(np.uint16), arrays[0])
        finally:
            g.close()


# ---- boundary ----------------------------------------------------------------------------------
def test_configuration(ctx, torch_cuda):
    from zarrs_amd import CodecChain, ZgpuError, _lib as L
    for cfg in ({}, {"level": 10}, {"level": "9"}, {"level": 9, "extra": 1}, {"level": -1}, {"level": 1.5}):
        with pytest.raises(ZgpuError) as ei:
            CodecChain.from_metadata([BYTES_LE, {"name": "numcodecs.bz2", "configuration": cfg}], "uint8", 0, ctx)
        assert ei.value.status == L.INVALID_ARGUMENT, cfg
    with pytest.raises(ZgpuError) as ei:
        CodecChain.from_metadata([BYTES_LE, "numcodecs.bz2"], "uint8", 0, ctx)
    assert ei.value.status == L.INVALID_ARGUMENT
    skipped = CodecChain.from_metadata([BYTES_LE, {"name": "numcodecs.bz2", "configuration": {"level": 10},
                                                   "must_understand": False}], "uint8", 0, ctx)
    assert bytes(skipped.decode(b"plain", [5])) == b"plain"
    level0 = CodecChain.from_metadata([BYTES_LE, BZ2(0)], "uint8", 0, ctx)  # decode ignores the level
    assert bytes(level0.decode(bz2.compress(b"abc", 3), [3])) == b"abc"


def test_encoded_bound_and_no_encoder(ctx, torch_cuda):
    from zarrs_amd import CodecChain, ZgpuError, _lib as L
    ch = CodecChain.from_metadata([BYTES_LE, BZ2(9)], "uint16", 0, ctx)
    for shape in ([1], [1000], [32, 32, 32]):
        n = 2 * int(np.prod(shape))
        assert ch.encoded_bound(shape) == n + n // 8 + 1024 and ch.encoded_size(shape) == -1
    crc = CodecChain.from_metadata([BYTES_LE, BZ2(9), {"name": "crc32c"}], "uint16", 0, ctx)
    assert crc.encoded_bound([1000]) == 2000 + 250 + 1024 + 4
    dev = torch_cuda.zeros(1000, dtype=torch_cuda.uint16, device="cuda")
    with pytest.raises(ZgpuError) as ei:
        ch.encode_chunks(dev, [1000], [[0]])
    assert ei.value.status == L.UNSUPPORTED
