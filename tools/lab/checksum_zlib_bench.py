"""Hand measurement of the adler32 / fletcher32 strip kernels beside k_crc32c_strip, and of the
numcodecs.zlib stage beside gzip (DESIGN "Checksum and zlib stages: measurements").

    python tools/lab/checksum_zlib_bench.py [--runs 5] [--steps 10] > out.json

Every figure is a plan execution timed with HIP events (torch.cuda.Event) on an MI355X: WARM untimed
executions, then `steps` timed ones per run, `runs` runs per variant, the variants taken in turn inside
each run. A checksum kernel's own time is the difference between the validating plan and the same plan
with ZGPU_NO_VALIDATE (which strips without summing): both run the same memset, item copy and scatter
on one stream. GiB/s = checksummed bytes / that difference. With few large items the difference is
not the kernel's time (the checksum leaves the items in the cache for the scatter, so the validating
plan can even be the faster one); there the kernels' own times come from a profiler run of one case,

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/lab/checksum_zlib_bench.py --only few --runs 1

gzip_one_wave is bytes + gzip with ZGPU_GZIP_DIRECT=0: the one-wave kernel into slots plus the scatter,
which is what the zlib stage runs (gzip itself writes whole chunks straight into the output rows).
"""
import argparse
import ctypes as C
import json
import statistics
import struct
import sys
import zlib
import os

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from zarrs_amd import CodecChain, Context, make_desc  # noqa: E402
from zarrs_amd import _lib as L  # noqa: E402

WARM = 3
BYTES_LE = {"name": "bytes", "configuration": {"endian": "little"}}


class Plan:
    def __init__(self, chain, descs, out_shape, flags=0):
        self.lib = L.load()
        self.n = len(descs)
        self.arr = (L.ChunkDesc * self.n)(*descs)
        self.h = C.c_void_p()
        self.chain = chain
        L.check(self.lib.zgpu_plan_create(chain._h, len(out_shape), self.arr, self.n, L.u64s(out_shape),
                                          flags | L.ENC_DEVICE | L.OUT_DEVICE, C.byref(self.h)))
        self.st = (C.c_int32 * self.n)()

    def execute(self, out):
        L.check(self.lib.zgpu_plan_execute(self.h, out.data_ptr(), None, None))

    def check(self):
        L.check(self.lib.zgpu_plan_status(self.h, self.st, None))
        assert list(self.st) == [0] * self.n

    def close(self):
        self.lib.zgpu_plan_destroy(self.h)


def time_plans(plans, out, runs, steps):
    """ms per execution: {name: [one mean per run]}; the plans alternate inside a run."""
    res = {k: [] for k in plans}
    for p in plans.values():
        for _ in range(WARM):
            p.execute(out)
        p.check()
    for _ in range(runs):
        for name, p in plans.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                p.execute(out)
            p.check()  # orders the default stream after the plan's
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / steps)
    return res


def checksum_case(ctx, n_items, item_bytes, runs, steps):
    """bytes + {crc32c, adler32(end), fletcher32} over n_items chunks of item_bytes; the stored values are
    computed by the write path (tests/test_gpu_checksum_zlib.py holds it to the CPU checkers)."""
    data = torch.randint(0, 256, (n_items * item_bytes,), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(data)
    result = {}
    for name, codec in (("crc32c", {"name": "crc32c"}),
                        ("adler32", {"name": "numcodecs.adler32", "configuration": {"location": "end"}}),
                        ("fletcher32", {"name": "numcodecs.fletcher32"})):
        ch = CodecChain.from_metadata([BYTES_LE, codec], "uint8", 0, ctx)
        encs = ch.encode_chunks(data, [item_bytes], [[i * item_bytes] for i in range(n_items)])
        descs = [make_desc((e.data_ptr(), e.numel()), [item_bytes], out_start=[i * item_bytes])
                 for i, e in enumerate(encs)]
        plans = {"validate": Plan(ch, descs, [n_items * item_bytes]),
                 "strip_only": Plan(ch, descs, [n_items * item_bytes], L.NO_VALIDATE)}
        ms = time_plans(plans, out, runs, steps)
        assert torch.equal(out, data)
        diff = [v - s for v, s in zip(ms["validate"], ms["strip_only"])]
        gib = n_items * item_bytes / 2 ** 30
        result[name] = {"validate_ms": ms["validate"], "strip_only_ms": ms["strip_only"], "checksum_ms": diff,
                        "checksum_GiBps_median": gib / (statistics.median(diff) / 1e3)}
        for p in plans.values():
            p.close()
        del encs
    return result


def zlib_case(ctx, n_items, runs, steps):
    """bytes + numcodecs.zlib beside bytes + gzip on the same DEFLATE bodies: 32^3 u16 chunks of a
    quantised smooth field (C3's inner chunks), level 5."""
    n = 32 ** 3
    rng = np.random.default_rng(0)
    bodies, chunks = [], []
    for i in range(64):  # 64 different chunks, repeated
        x = np.arange(n, dtype=np.float32) + i * 1000
        f = (np.sin(0.01 * x) + np.cos(0.0007 * x)) * 2000 + rng.integers(0, 8, n)
        a = f.astype(np.uint16)
        c = zlib.compressobj(5, zlib.DEFLATED, -15)
        chunks.append(a)
        bodies.append(c.compress(a.tobytes()) + c.flush())
    result = {"n_items": n_items, "encoded_bytes_mean": float(np.mean([len(b) for b in bodies]))}
    exp = torch.from_numpy(np.concatenate([chunks[i % 64] for i in range(n_items)]).view(np.int16)).cuda()
    out = torch.empty_like(exp)
    plans, keep = {}, []
    for name in ("gzip", "gzip_one_wave", "zlib"):
        encs = []
        for b, a in zip(bodies, chunks):
            raw = a.tobytes()
            if name != "zlib":
                encs.append(b"\x1f\x8b\x08\0\0\0\0\0\0\xff" + b + struct.pack("<II", zlib.crc32(raw), len(raw)))
            else:
                encs.append(b"\x78\x5e" + b + struct.pack(">I", zlib.adler32(raw)))
                assert zlib.decompress(encs[-1]) == raw
        blob = b"".join(encs[i % 64] for i in range(n_items))
        dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
        keep.append(dev)
        descs, off = [], 0
        for i in range(n_items):
            ln = len(encs[i % 64])
            descs.append(make_desc((dev.data_ptr() + off, ln), [n], out_start=[i * n]))
            off += ln
        codec = {"name": "gzip", "configuration": {"level": 5}} if name != "zlib" else \
            {"name": "numcodecs.zlib", "configuration": {"level": 5}}
        ch = CodecChain.from_metadata([BYTES_LE, codec], "uint16", 0, ctx)
        if name == "gzip_one_wave":
            os.environ["ZGPU_GZIP_DIRECT"] = "0"  # read when the plan is built
        plans[name] = Plan(ch, descs, [n_items * n])
        os.environ.pop("ZGPU_GZIP_DIRECT", None)
    ms = time_plans(plans, out, runs, steps)
    for name, p in plans.items():
        out.zero_()
        p.execute(out)
        p.check()
        assert torch.equal(out, exp), name
        p.close()
    result.update({f"{k}_ms": v for k, v in ms.items()})
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal, not a measurement)")
    ap.add_argument("--only", choices=["many", "few", "zlib"], help="one case (profiler runs)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ctx = Context(0)
    many = (64, 1 << 16) if a.small else (4096, 1 << 20)
    few = (4, 1 << 20) if a.small else (4, 64 << 20)
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "steps": a.steps}
    if a.only in (None, "many"):
        res["checksum_many_items"] = {"items": many[0], "item_bytes": many[1],
                                      **checksum_case(ctx, many[0], many[1], a.runs, a.steps)}
    if a.only in (None, "few"):
        res["checksum_few_items"] = {"items": few[0], "item_bytes": few[1],
                                     **checksum_case(ctx, few[0], few[1], a.runs, a.steps)}
    if a.only in (None, "zlib"):
        res["zlib_vs_gzip"] = zlib_case(ctx, 512 if a.small else 15625, a.runs, a.steps)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
