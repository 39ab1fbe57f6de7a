#!/usr/bin/env python3
"""Store by coordinates on C3's array (bench.py's C3 as tools/points_bench.py sets it up: sharded [2048]^3
f32, 256^3 shards of 32^3 inner chunks, [bytes, gzip 1, crc32c] + [bytes, crc32c] index; the 64 shards that
hold the subset [200:968, 300:1068, 1000:1768] are resident): N uniformly random points of that subset,
random non-fill values, through

  new     zgpu_store_elements (device chunks, indices and data; and host chunks, indices and data)
  stacked the best a caller can do without it: one zgpu_decode_batch of every touched shard whole, stacked
          along axis 0; index_put_ with torch on the device; one zgpu_encode_chunks of those shards. The last
          point on a coordinate wins in both legs; the stacked leg gets that deterministically by dropping
          all but the last point of every coordinate on the host, outside the timed region (index_put_ with
          duplicates has no defined order). For the host leg the shards, indices and data are uploaded and
          the encoded shards copied back inside the timed region.

Both are checked once against the model: the synthetic values with the points applied in order. The new
call's shards are read back at every point and at as many untouched coordinates with
zgpu_retrieve_elements; the stacked leg's encoded shards are decoded whole again. One process, the legs
interleaved round by round, warm-up rounds first; median, min and max of the rounds are reported.

    python tools/store_points_bench.py [--points 4096,1048576] [--rounds 7] [--warmup 2] [--legs new_device,...]
                                       [--out FILE.json]

The share of the winner table (its memset, k_points_claim, k_points_scatter) in the new call comes from a
second run of the new_device leg alone under a kernel trace (rocprofv3 --kernel-trace --stats), never from
the timed run.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import points_bench as PB  # noqa: E402
from zarrs_amd import CodecChain, Context, make_desc  # noqa: E402
from zarrs_amd import _lib as L  # noqa: E402

S, I = PB.S, PB.I
ARRAY, START, SHAPE = PB.ARRAY, PB.START, PB.SHAPE
u64 = PB.u64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096,1048576")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="new_device,stacked_device,new_host,stacked_host")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = Context(0)
    chain = CodecChain.from_metadata(bench.C3.CODECS, "float32", 0.0, ctx)
    t0 = time.perf_counter()
    shards = PB.build_shards(dev)
    grid = [a // S for a in ARRAY]
    n_grid = int(np.prod(grid))
    order = sorted(shards)  # chunk-grid order: the order of the new call's entries
    lin_of = {idx: int(np.ravel_multi_index(idx, grid)) for idx in order}
    tabs = {}
    for where in ("dev", "host"):
        ptrs, lens = (C.c_void_p * n_grid)(), (C.c_uint64 * n_grid)()
        for idx, (t, h) in shards.items():
            ptrs[lin_of[idx]] = t.data_ptr() if where == "dev" else h.ctypes.data
            lens[lin_of[idx]] = len(h)
        tabs[where] = (ptrs, lens)
    lib = L.load()
    enc_total = int(sum(len(h) for _, h in shards.values()))
    record = {"workload": "C3 array of bench.py: points uniform in the subset " + str(START) + " + " + str(SHAPE),
              "device": torch.cuda.get_device_name(0), "resident_shards": len(shards), "encoded_bytes_resident": enc_total,
              "setup_s": round(time.perf_counter() - t0, 1), "warmup": args.warmup, "rounds": args.rounds, "legs": []}
    syn = bench._synth()
    base = np.empty(SHAPE, np.float32)  # the subset's old values
    syn.synth_c3_values(u64(START), u64(SHAPE), base.ctypes.data, bench._threads())
    rng = np.random.default_rng(23)
    for n in [int(v) for v in args.points.split(",")]:
        pts = np.stack([rng.integers(s, s + e, size=n) for s, e in zip(START, SHAPE)], axis=1).astype(np.int64)
        data = (rng.random(n, dtype=np.float32) + 1.0).astype(np.float32)  # never the fill value
        upts = np.ascontiguousarray(pts.astype(np.uint64))
        d_pts, d_data = torch.from_numpy(pts).to(dev), torch.from_numpy(data).to(dev)
        # the model: the points applied in order; per coordinate its last point
        flat_arr = np.ravel_multi_index(tuple(pts.T), ARRAY)
        _, first_rev = np.unique(flat_arr[::-1], return_index=True)
        last = np.sort(n - 1 - first_rev)  # the indices of the winning points
        model = base.copy()
        rel = pts[last] - np.asarray(START)
        model[rel[:, 0], rel[:, 1], rel[:, 2]] = data[last]
        leaves = len(np.unique(pts // I, axis=0))
        touched = sorted({tuple(int(v) for v in p) for p in np.unique(pts // S, axis=0)})
        # the stacked leg's host preparation (outside the timed region): winners only, their place in the stack
        tp = time.perf_counter()
        wp = pts[last]
        k_of = {idx: k for k, idx in enumerate(touched)}
        sh_k = np.asarray([k_of[tuple(int(v) for v in p)] for p in wp // S], np.int64)
        r3 = wp % S
        flat = ((sh_k * S + r3[:, 0]) * S + r3[:, 1]) * S + r3[:, 2]
        prep_ms = (time.perf_counter() - tp) * 1e3
        d_flat, d_wdata = torch.from_numpy(flat).to(dev), torch.from_numpy(data[last]).to(dev)
        descs = {w: [make_desc((shards[idx][0].data_ptr(), len(shards[idx][1])) if w == "dev" else
                               (shards[idx][1].ctypes.data, len(shards[idx][1])), [S] * 3, out_start=[k * S, 0, 0])
                     for k, idx in enumerate(touched)] for w in ("dev", "host")}
        stack = torch.empty([len(touched) * S, S, S], dtype=torch.float32, device=dev)
        starts = [[k * S, 0, 0] for k in range(len(touched))]
        torch.cuda.synchronize()

        def new(where, ip, dp, flags):
            ents, ne, res = C.POINTER(L.StoreEntry)(), C.c_uint64(), C.c_void_p()
            L.check(lib.zgpu_store_elements(chain._h, 3, u64(ARRAY), u64([S] * 3), *tabs[where], ip, n, dp, flags,
                                            C.byref(ents), C.byref(ne), C.byref(res), None))
            return ents, ne.value, res

        def new_dev():
            return new("dev", d_pts.data_ptr(), d_data.data_ptr(), L.ENC_DEVICE | L.OUT_DEVICE | L.IDX_DEVICE)

        def new_host():
            return new("host", upts.ctypes.data, data.ctypes.data, 0)

        def stacked(where):
            if where == "host":
                f, w = torch.from_numpy(flat).to(dev), torch.from_numpy(data[last]).to(dev)
            else:
                f, w = d_flat, d_wdata
            chain.decode_batch(descs[where], stack, list(stack.shape), enc_device=where == "dev")
            stack.reshape(-1).index_put_((f,), w)
            enc = chain.encode_chunks(stack, [S] * 3, starts)
            return [e.cpu().numpy() for e in enc] if where == "host" else enc

        legs = {"new_device": new_dev, "stacked_device": lambda: stacked("dev"),
                "new_host": new_host, "stacked_host": lambda: stacked("host")}
        legs = {k: v for k, v in legs.items() if k in args.legs.split(",")}
        times = {k: [] for k in legs}
        ctrs = {}
        # what the checks read: every point and as many other coordinates of the subset
        other = np.stack([rng.integers(s, s + e, size=n) for s, e in zip(START, SHAPE)], axis=1).astype(np.int64)
        chk = np.concatenate([pts, other])
        crel = chk - np.asarray(START)
        want = model[crel[:, 0], crel[:, 1], crel[:, 2]]
        for r in range(args.warmup + args.rounds):
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                got = fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t1) * 1e3
                if name.startswith("new"):
                    ents, ne, res = got
                    if r == 0:
                        ctrs[name] = L.last_counters()
                        assert [ents[i].chunk for i in range(ne)] == [lin_of[idx] for idx in touched]
                        assert all(ents[i].action == L.STORE_SET and ents[i].status == 0 for i in range(ne))
                        host = name.endswith("host")
                        ptrs, lens = (C.c_void_p * n_grid)(), (C.c_uint64 * n_grid)()
                        for i in range(ne):
                            ptrs[ents[i].chunk], lens[ents[i].chunk] = ents[i].enc, ents[i].enc_len
                        out = np.empty(len(chk), np.float32)
                        cu = np.ascontiguousarray(chk.astype(np.uint64))
                        L.check(lib.zgpu_retrieve_elements(chain._h, 3, u64(ARRAY), u64([S] * 3), ptrs, lens, cu.ctypes.data,
                                                           len(cu), out.ctypes.data, 0 if host else L.ENC_DEVICE, None))
                        assert np.array_equal(out, want), name
                        ctrs[name]["new_encoded_bytes"] = int(sum(ents[i].enc_len for i in range(ne)))
                    lib.zgpu_result_release(res)
                elif r == 0:
                    ctrs[name] = {}
                    again = torch.empty_like(stack)
                    d2 = [make_desc((e.data_ptr(), e.numel()) if isinstance(e, torch.Tensor) else (e.ctypes.data, len(e)),
                                    [S] * 3, out_start=[k * S, 0, 0]) for k, e in enumerate(got)]
                    chain.decode_batch(d2, again, list(again.shape), enc_device=isinstance(got[0], torch.Tensor))
                    for k, idx in enumerate(touched):
                        lo = [max(i * S, s) for i, s in zip(idx, START)]
                        hi = [min((i + 1) * S, s + e) for i, s, e in zip(idx, START, SHAPE)]
                        a = again[k * S:(k + 1) * S][tuple(slice(a - i * S, b - i * S) for a, b, i in zip(lo, hi, idx))]
                        m = model[tuple(slice(a - s, b - s) for a, b, s in zip(lo, hi, START))]
                        assert np.array_equal(a.cpu().numpy(), m), (name, idx)
                    ctrs[name]["new_encoded_bytes"] = int(sum(len(e) for e in got))
                    del again
                del got
                if r >= args.warmup:
                    times[name].append(dt)
        for name in legs:
            record["legs"].append({"points": n, "distinct_coordinates": int(len(last)), "leg": name,
                                   "touched_inner_chunks": leaves, "touched_shards": len(touched), **PB.stats(times[name]),
                                   "staged_bytes": leaves * I ** 3 * 4 if name.startswith("new") else len(touched) * S ** 3 * 4,
                                   "winner_table_bytes": leaves * I ** 3 * 4 if name.startswith("new") else 0,
                                   "counters": ctrs[name],
                                   "host_prep_ms_outside_timing": round(prep_ms, 1) if name.startswith("stacked") else 0})
            print(json.dumps(record["legs"][-1]), flush=True)
        del stack, descs
    line = json.dumps(record)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
