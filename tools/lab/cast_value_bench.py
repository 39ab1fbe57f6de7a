"""Cost of cast_value beside fixedscaleoffset on the array of value_fso_bench.py: [256,256,256] f32
stored as u8 + sharded zstd, encoded bytes in HBM, output in HBM; HIP events, median of REPS after 3
warm-ups, the two sides of every comparison interleaved inside one run:
  * k_cast<u8, f32> (the decode of cast_value(uint8, out_of_range clamp)) against k_fso_decode<u8, f32>,
    each launched alone through the library's own launchers on the same 16 MiB in / 64 MiB out;
  * the full read of the cast_value chain against the full read of the fixedscaleoffset chain;
  * one fallible pair, the encode k_cast<f64, i16> (128 MiB in, 32 MiB out, with its failure word).
The yardstick for k_cast<u8, f32> is the fso kernel of the same run and its own min..max spread. Prints
one JSON line (and writes it to the file named by the first argument, if any)."""
import ctypes as C
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.abspath(__file__))
while not os.path.isdir(os.path.join(ROOT, "zarrs_amd")):
    ROOT = os.path.dirname(ROOT)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
from zarrs_amd import CodecChain, Context, make_desc
from zarrs_amd import _lib as L

REPS = 15
ctx = Context(0)
BYTES = {"name": "bytes", "configuration": {"endian": "little"}}
IDX = [BYTES, {"name": "crc32c"}]
FSO = {"name": "numcodecs.fixedscaleoffset", "configuration": {"offset": 1000, "scale": 10, "dtype": "<f4", "astype": "|u1"}}
CAST = {"name": "cast_value", "configuration": {"data_type": "uint8", "out_of_range": "clamp"}}
SH = {"name": "sharding_indexed", "configuration": {"chunk_shape": [32, 32, 32], "index_codecs": IDX,
      "codecs": [BYTES, {"name": "zstd", "configuration": {"level": 3, "checksum": False}}]}}
N, S = 256, 128
g = torch.Generator(device="cuda").manual_seed(1)
z = torch.linspace(0, 6.28, N, device="cuda")
a = (1012 + 8 * torch.sin(z)[:, None, None] * torch.cos(z)[None, :, None] + 3 * torch.sin(3 * z)[None, None, :]
     + 0.3 * torch.randn(N, N, N, device="cuda", generator=g)).float().contiguous()
b = ((a - 1000) * 10).contiguous()  # what cast_value stores as u8 is what fixedscaleoffset stores, up to ties
fso = CodecChain.from_metadata([FSO, SH], "float32", 1000.0, ctx)
cast = CodecChain.from_metadata([CAST, SH], "float32", 0.0, ctx)
starts = [[i, j, k] for i in range(0, N, S) for j in range(0, N, S) for k in range(0, N, S)]
parts = {"fso": fso.encode_chunks(a, [S, S, S], starts), "cast": cast.encode_chunks(b, [S, S, S], starts)}
descs = {k: [make_desc(p, [S, S, S], out_start=st) for p, st in zip(v, starts)] for k, v in parts.items()}
out = torch.empty((N, N, N), dtype=torch.float32, device="cuda")


def launcher(name):
    """a C++ launcher of kernels/launch.hpp by its mangled name in the library's dynamic symbol table"""
    lib = L.load()
    syms = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout.split()
    f = getattr(lib, next(s for s in syms if s.startswith(f"_ZN4zgpu{len(name)}{name}E")))
    f.restype = C.c_int
    return f


class CastMap(C.Structure):  # kernels/cast.hpp
    _fields_ = [("n", C.c_uint32), ("pad", C.c_uint32), ("key", C.c_uint64 * 32), ("val", C.c_uint64 * 32)]


VT = {"int16": 1, "uint8": 4, "float32": 8, "float64": 9}  # ZgValueType
launch_cast, launch_fso_decode = launcher("launch_cast"), launcher("launch_fso_decode")
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
nomap = CastMap()
u8 = torch.randint(0, 256, (N * N * N,), dtype=torch.uint8, device="cuda", generator=g)
f64 = (torch.randn(N * N * N, device="cuda", generator=g, dtype=torch.float64) * 9000).clamp(-32768, 32767)
i16 = torch.empty(N * N * N, dtype=torch.int16, device="cuda")
fail = torch.full((1,), -1, dtype=torch.int64, device="cuda")
n = C.c_uint64(N * N * N)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def k_fso():
    assert launch_fso_decode(VT["uint8"], VT["float32"], p(u8), p(out), n, C.c_float(1000), C.c_float(10), 1, stream) == 0


def k_cast_u8_f32():
    assert launch_cast(VT["uint8"], VT["float32"], p(u8), p(out), n, 0, 1, C.byref(nomap), p(fail), stream) == 0


def k_cast_f64_i16():
    assert launch_cast(VT["float64"], VT["int16"], p(f64), p(i16), n, 4, 0, C.byref(nomap), p(fail), stream) == 0


def timed(fns):
    """every function once per round, in turn (A B A B ...): {name: median / min / max in ms}"""
    ts = {k: [] for k in fns}
    for r in range(REPS + 3):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= 3:
                ts[k].append(e0.elapsed_time(e1))
    return {k: {"median_ms": round(sorted(v)[len(v) // 2], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in ts.items()}


res = {"array": [N, N, N], "shard": [S, S, S], "inner": [32, 32, 32], "reps": REPS,
       "encoded_bytes": {k: sum(int(q.numel()) for q in v) for k, v in parts.items()}}
res["kernels"] = timed({"k_fso_decode_u8_f32": k_fso, "k_cast_u8_f32_decode_clamp": k_cast_u8_f32,
                        "k_cast_f64_i16_encode_nearest_away": k_cast_f64_i16})
k = res["kernels"]
res["k_cast_over_k_fso_decode"] = round(k["k_cast_u8_f32_decode_clamp"]["median_ms"] / k["k_fso_decode_u8_f32"]["median_ms"], 3)
res["k_cast_f64_i16_failed_elements"] = int(fail.item() != -1)
res["reads"] = timed({"full_read_fso_u8_sharded_zstd": lambda: fso.decode_batch(descs["fso"], out, [N, N, N], enc_device=True),
                      "full_read_cast_u8_sharded_zstd": lambda: cast.decode_batch(descs["cast"], out, [N, N, N], enc_device=True)})
# the result is right: the exact model on part of a row (the cast chain's read is the last one into `out`)
import cast_value_model as M
row = b[37, 11, :64].cpu().numpy()
enc, bad = M.encode_bits([int(x) for x in row.view("<u4")], CAST["configuration"], "float32")
dec, _ = M.decode_bits(enc, CAST["configuration"], "float32")
res["sample_bit_exact"] = bool(bad is None and out[37, 11, :64].cpu().numpy().tobytes() == M.to_bytes(dec, "float32"))
res["device"] = torch.cuda.get_device_name(0)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
print(json.dumps(res))
