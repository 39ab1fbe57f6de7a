"""numcodecs.bz2 decode throughput on the GPU beside libbz2 on a 16-thread pool (not a gate).

  python tools/lab/bz2_bench.py [--chunks 256] [--runs 7] [--only NAME]

Workloads: `--chunks` chunks of 1 MiB of a byte-shuffled u16 ramp image and of random bytes, each at
levels 1 and 9, and a lone 16 MiB chunk at level 9, once of random bytes (19 blocks) and once of the
image (10 blocks: RLE1 shortens its high-byte plane before the blocks are cut). Device in, device out:
a plan is created once and executed `--runs` times after two warm-up executions on a stream of its own,
timed with HIP events. The CPU figure is bz2.decompress of the same chunks on a 16-thread pool (the
module releases the GIL), `--runs` times. Both figures are medians. GiB/s are decoded bytes per second.
Prints one JSON line per workload.

The per-kernel split comes from a run of its own:
  rocprofv3 --kernel-trace --stats -- python tools/lab/bz2_bench.py --only random-l9 --chunks 64 --runs 3
"""
import argparse
import bz2
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def image(n, seed):
    rng = np.random.default_rng(seed)
    m = n // 2
    img = (np.arange(m) // 7 + rng.integers(0, 9, m)).astype("<u2")
    return np.frombuffer(img.tobytes(), np.uint8).reshape(m, 2).T.tobytes()


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def bench(name, chunks, level, n, runs):
    import torch
    from zarrs_amd import CodecChain, Context, make_desc
    from zarrs_amd import _lib as L
    lib = L.load()
    with ThreadPoolExecutor(16) as pool:
        encs = list(pool.map(lambda c: bz2.compress(c, level), chunks))
    k = len(encs)
    ch = CodecChain.from_metadata([{"name": "bytes", "configuration": {"endian": "little"}},
                                   {"name": "numcodecs.bz2", "configuration": {"level": level}}], "uint8", 0,
                                  Context.default())
    offs = np.cumsum([0] + [len(e) for e in encs])
    blob = torch.frombuffer(bytearray(b"".join(encs)), dtype=torch.uint8).cuda()
    descs = (L.ChunkDesc * k)(*[make_desc((blob.data_ptr() + int(offs[i]), len(encs[i])), [n], out_start=[i * n])
                                for i in range(k)])
    plan = C.c_void_p()
    L.check(lib.zgpu_plan_create(ch._h, 1, descs, k, L.u64s([k * n]), L.ENC_DEVICE | L.OUT_DEVICE, C.byref(plan)))
    out = torch.zeros(k * n, dtype=torch.uint8, device="cuda")
    st = (C.c_int32 * k)()
    stream = torch.cuda.Stream()  # a stream of its own: with the default stream the library runs on its lane
    torch.cuda.synchronize()
    ms = []
    try:
        for it in range(runs + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            rc = lib.zgpu_plan_execute(plan, out.data_ptr(), None, C.c_void_p(stream.cuda_stream))
            b.record(stream)
            b.synchronize()
            assert rc == 0 and lib.zgpu_plan_status(plan, st, C.c_void_p(stream.cuda_stream)) == 0
            if it >= 2:
                ms.append(a.elapsed_time(b))
        ctr = (C.c_uint64 * L.N_COUNTERS)()
        lib.zgpu_plan_counters(plan, ctr, L.N_COUNTERS)
        assert out[:n].cpu().numpy().tobytes() == chunks[0] and out[-n:].cpu().numpy().tobytes() == chunks[-1]
    finally:
        lib.zgpu_plan_destroy(plan)
    with ThreadPoolExecutor(16) as pool:
        cpu = []
        for _ in range(runs):
            t = time.perf_counter()
            list(pool.map(bz2.decompress, encs))
            cpu.append(time.perf_counter() - t)
    gib = k * n / 2 ** 30
    gpu_ms, cpu_s = statistics.median(ms), statistics.median(cpu)
    print(json.dumps({"workload": name, "chunks": k, "chunk_bytes": n, "level": level, "blocks": int(ctr[L.CTR_BZ2_BLOCKS]),
                      "ratio": round(k * n / sum(map(len, encs)), 2), "gpu_ms": round(gpu_ms, 3),
                      "gpu_GiBps": round(gib / (gpu_ms / 1e3), 3), "cpu16_ms": round(cpu_s * 1e3, 1),
                      "cpu16_GiBps": round(gib / cpu_s, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    assert a.runs >= 5 or a.only
    mib = 1 << 20
    work = []
    for level in (1, 9):
        work.append((f"image-l{level}", [image(mib, s) for s in range(a.chunks)], level, mib))
        work.append((f"random-l{level}", [noise(mib, s) for s in range(a.chunks)], level, mib))
    work.append(("lone-16MiB-random-l9", [noise(16 * mib, 99)], 9, 16 * mib))
    work.append(("lone-16MiB-image-l9", [image(16 * mib, 99)], 9, 16 * mib))
    for name, chunks, level, n in work:
        if a.only in (None, name):
            bench(name, chunks, level, n, a.runs)


if __name__ == "__main__":
    main()
