#!/usr/bin/env python3
"""Read by coordinates on C3's array (bench.py's C3: sharded [2048]^3 f32, 256^3 shards of 32^3 inner chunks,
[bytes, gzip 1, crc32c] + [bytes, crc32c] index; the 64 shards that hold the subset [200:968, 300:1068,
1000:1768] are resident): N uniformly random points of that subset through

  new     zgpu_retrieve_elements (device chunks, device indices, device output; and host indices + output)
  stacked the method that exists without it: one descriptor per touched inner chunk (built on the host
          from host indices, outside the timed region), the inner chunks decoded stacked along axis 0 by
          one zgpu_decode_batch, the stack indexed with torch on the device; for a host output
          decode_pinned_into of the stack plus the numpy gather.

Both are checked against the synthetic values. One process, the legs interleaved round by round, warm-up
rounds first; median, min and max of the rounds are reported, with the bytes each leg moves over PCIe by
construction (descriptor and plan tables inside the decode are not counted; both legs have them).

    python tools/points_bench.py [--points 4096,1048576] [--rounds 7] [--warmup 2] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from zarrs_amd import CodecChain, Context, make_desc  # noqa: E402
from zarrs_amd import _lib as L  # noqa: E402

S, I = bench.C3.SHARD, bench.C3.INNER
ARRAY, START, SHAPE = bench.C3.ARRAY, bench.C3.SUB_START, bench.C3.SUB_SHAPE


def u64(v):
    return (C.c_uint64 * len(v))(*[int(x) for x in v])


def build_shards(dev):
    """the resident shards as bench.py's C3 writes them: {(si, sj, sk): (device tensor, host array)}"""
    syn, nt = bench._synth(), bench._threads()
    lo = [s // S for s in START]
    hi = [(s + n - 1) // S + 1 for s, n in zip(START, SHAPE)]
    dec = np.empty([S] * 3, np.float32)
    shards = {}
    for si in range(lo[0], hi[0]):
        for sj in range(lo[1], hi[1]):
            for sk in range(lo[2], hi[2]):
                syn.synth_c3_values(u64([si * S, sj * S, sk * S]), u64([S] * 3), dec.ctypes.data, nt)
                p, n = C.c_void_p(), C.c_uint64()
                if syn.synth_gzip_crc_shard(dec.ctypes.data, 4, u64([S] * 3), u64([I] * 3), 1, nt, C.byref(p), C.byref(n)):
                    raise RuntimeError("shard encode failed")
                host = np.ctypeslib.as_array((C.c_uint8 * n.value).from_address(p.value)).copy()
                syn.synth_free(p)
                shards[(si, sj, sk)] = (torch.from_numpy(host).to(dev), host)
                print(f"shard {len(shards)} encoded", file=sys.stderr, flush=True)
    return shards


def expected(pts):
    """the synthetic values at the points (one element boxes would be slow: whole subset once)"""
    syn = bench._synth()
    exp = np.empty(SHAPE, np.float32)
    syn.synth_c3_values(u64(START), u64(SHAPE), exp.ctypes.data, bench._threads())
    rel = pts - np.asarray(START)
    return exp[rel[:, 0], rel[:, 1], rel[:, 2]]


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
            "rounds_ms": [round(v, 3) for v in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096,1048576")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-rounds", type=int, default=3, help="rounds of the host-output legs")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = Context(0)
    chain = CodecChain.from_metadata(bench.C3.CODECS, "float32", 0.0, ctx)
    t0 = time.perf_counter()
    shards = build_shards(dev)
    grid = [a // S for a in ARRAY]
    n_grid = int(np.prod(grid))
    tabs = {}
    for where in ("dev", "host"):
        ptrs, lens = (C.c_void_p * n_grid)(), (C.c_uint64 * n_grid)()
        for idx, (t, h) in shards.items():
            lin = int(np.ravel_multi_index(idx, grid))
            ptrs[lin] = t.data_ptr() if where == "dev" else h.ctypes.data
            lens[lin] = len(h)
        tabs[where] = (ptrs, lens)
    lib = L.load()
    record = {"workload": "C3 array of bench.py: points uniform in the subset " + str(START) + " + " + str(SHAPE),
              "device": torch.cuda.get_device_name(0), "resident_shards": len(shards),
              "encoded_bytes_resident": int(sum(len(h) for _, h in shards.values())),
              "setup_s": round(time.perf_counter() - t0, 1), "warmup": args.warmup, "legs": []}
    rng = np.random.default_rng(17)
    for n in [int(v) for v in args.points.split(",")]:
        pts = np.stack([rng.integers(s, s + e, size=n) for s, e in zip(START, SHAPE)], axis=1).astype(np.int64)
        exp = expected(pts)
        d_pts = torch.from_numpy(pts).to(dev)
        # the stacked method's host preparation: the touched inner chunks, a descriptor each, each point's
        # place in the stack
        tp = time.perf_counter()
        leaf = pts // I
        keys, inv = np.unique(leaf, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        rel = pts % I
        flat = (inv * I ** 3 + (rel[:, 0] * I + rel[:, 1]) * I + rel[:, 2]).astype(np.int64)
        descs = {"dev": [], "host": []}
        for k, ci in enumerate(keys):
            org = ci * I
            sh = tuple(int(v) for v in org // S)
            for where in ("dev", "host"):
                t, h = shards[sh]
                enc = (t.data_ptr(), len(h)) if where == "dev" else (h.ctypes.data, len(h))
                descs[where].append(make_desc(enc, [S] * 3, sel_start=[int(v) for v in org % S], sel_shape=[I] * 3,
                                              out_start=[k * I, 0, 0]))
        prep_ms = (time.perf_counter() - tp) * 1e3
        n_leaf = len(keys)
        d_flat = torch.from_numpy(flat).to(dev)
        stack = torch.empty([n_leaf * I, I, I], dtype=torch.float32, device=dev)
        out_new = torch.empty(n, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        def new_dev():
            L.check(lib.zgpu_retrieve_elements(chain._h, 3, u64(ARRAY), u64([S] * 3), *tabs["dev"], d_pts.data_ptr(), n,
                                               out_new.data_ptr(), L.ENC_DEVICE | L.OUT_DEVICE | L.IDX_DEVICE, None))
            return out_new

        def stacked_dev():
            chain.decode_batch(descs["dev"], stack, list(stack.shape), enc_device=True)
            return stack.reshape(-1)[d_flat]

        h_out = np.empty(n, np.float32)
        h_stack = np.empty([n_leaf * I, I, I], np.float32)

        def new_host():
            L.check(lib.zgpu_retrieve_elements(chain._h, 3, u64(ARRAY), u64([S] * 3), *tabs["host"], pts.ctypes.data, n,
                                               h_out.ctypes.data, 0, None))
            return h_out

        def stacked_host():
            chain.decode_pinned_into(descs["host"], h_stack, [0, 0, 0], list(h_stack.shape))
            return h_stack.reshape(-1)[flat]

        legs = {"new_device": new_dev, "stacked_device": stacked_dev}
        if args.host_rounds:
            legs.update({"new_host": new_host, "stacked_host": stacked_host})
        times = {k: [] for k in legs}
        ctrs = {}
        for r in range(args.warmup + args.rounds):
            for name, fn in legs.items():
                if name.endswith("host") and r >= args.warmup + args.host_rounds:
                    continue
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                got = fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t1) * 1e3
                if r == 0:
                    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
                    assert np.array_equal(g, exp), name
                    ctrs[name] = L.last_counters()
                    buf = (C.c_uint64 * L.N_COUNTERS)()
                    lib.zgpu_last_counters(buf, L.N_COUNTERS)
                    ctrs[name]["items"] = int(buf[L.CTR_ITEMS])
                if r >= args.warmup:
                    times[name].append(dt)
        words = (int(np.prod([a // I for a in ARRAY])) + 31) // 32
        rounds = ctrs["new_device"]["point_rounds"]
        mark = 8 + 2 * words * 4  # the bitmap and out-of-bounds word back, the prefix counts up
        pcie = {"new_device": mark + rounds * n_leaf * 8,
                "stacked_device": 0,
                "new_host": mark + rounds * n_leaf * 8 + n * 24 + n * 4 + int(sum(len(h) for _, h in shards.values())),
                "stacked_host": n_leaf * I ** 3 * 4 + int(sum(len(h) for _, h in shards.values()))}
        for name in legs:
            record["legs"].append({"points": n, "leg": name, "touched_inner_chunks": n_leaf, **stats(times[name]),
                                   "pcie_bytes_by_construction": pcie[name], "counters": ctrs[name],
                                   "host_prep_ms_outside_timing": round(prep_ms, 1) if name.startswith("stacked") else 0})
            print(json.dumps(record["legs"][-1]), flush=True)
        del stack, h_stack, descs
    line = json.dumps(record)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
