"""Cost of the composed value-codec path: [256,256,256] f32 stored as fixedscaleoffset(astype u8) +
sharded zstd, encoded bytes in HBM, output in HBM. Times (HIP events, median of REPS): the full read,
the same read of the chain without the value codec (u8 output), a device-to-device copy of the
output bytes. Prints one JSON line (and writes it to the file named by the first argument, if any).
Run it under `rocprofv3 --kernel-trace --stats` for k_fso_decode's own duration
(profiles/value_fso_256cube_*)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
from zarrs_amd import CodecChain, Context, make_desc

REPS = 15
ctx = Context(0)
BYTES = {"name": "bytes", "configuration": {"endian": "little"}}
IDX = [BYTES, {"name": "crc32c"}]
FSO = {"name": "numcodecs.fixedscaleoffset", "configuration": {"offset": 1000, "scale": 10, "dtype": "<f4", "astype": "|u1"}}
SH = {"name": "sharding_indexed", "configuration": {"chunk_shape": [32, 32, 32], "index_codecs": IDX,
      "codecs": [BYTES, {"name": "zstd", "configuration": {"level": 3, "checksum": False}}]}}
N, S = 256, 128
g = torch.Generator(device="cuda").manual_seed(1)
z = torch.linspace(0, 6.28, N, device="cuda")
a = (1012 + 8 * torch.sin(z)[:, None, None] * torch.cos(z)[None, :, None] + 3 * torch.sin(3 * z)[None, None, :]
     + 0.3 * torch.randn(N, N, N, device="cuda", generator=g)).float().contiguous()
full = CodecChain.from_metadata([FSO, SH], "float32", 1000.0, ctx)
bare = CodecChain.from_metadata([SH], "uint8", 0, ctx)
starts = [[i, j, k] for i in range(0, N, S) for j in range(0, N, S) for k in range(0, N, S)]
parts = full.encode_chunks(a, [S, S, S], starts)
enc_bytes = sum(int(p.numel()) for p in parts)
descs = [make_desc(p, [S, S, S], out_start=st) for p, st in zip(parts, starts)]
out = torch.empty((N, N, N), dtype=torch.float32, device="cuda")
out8 = torch.empty((N, N, N), dtype=torch.uint8, device="cuda")
out2 = torch.empty_like(out)

def timed(fn):
    ts = []
    for r in range(REPS + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            ts.append(e0.elapsed_time(e1))
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}

res = {"array": [N, N, N], "shard": [S, S, S], "inner": [32, 32, 32], "encoded_bytes": enc_bytes,
       "output_bytes": out.numel() * 4, "reps": REPS}
res["full_read_fso_u8_sharded_zstd"] = timed(lambda: full.decode_batch(descs, out, [N, N, N], enc_device=True))
res["read_without_value_codec_u8"] = timed(lambda: bare.decode_batch(descs, out8, [N, N, N], enc_device=True))
res["d2d_copy_of_output_bytes"] = timed(lambda: out2.copy_(out))
# the result is right: the model on a sample plane
import value_codecs as V
samp = a[37].cpu().numpy()
want = V.fso_decode(V.fso_encode(samp, 1000, 10, "f4", "u1"), 1000, 10, "f4", "u1")
res["sample_plane_bit_exact"] = bool(out[37].cpu().numpy().tobytes() == want.tobytes())
res["device"] = torch.cuda.get_device_name(0)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
print(json.dumps(res))
