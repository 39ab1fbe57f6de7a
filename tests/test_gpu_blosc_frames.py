"""The blosc kernels (k_blosc_info, k_blosc_layout, k_blosc_streams, k_lz_list, k_lz4m, k_blosclzm,
k_snappym, k_blosc_finish) on hand-built frames (tests/blosc_frames.py): fields across the input window's
refills at every stream-address residue, matches on both sides of the output ring's edge and of the
far path's fence, every length encoding's boundary, streams paired unevenly in a wave and stream tables
across k_lz_list's rounds, frame layouts c-blosc accepts and refuses, unshuffles of hand-placed streams,
and corrupt and lenient streams, each beside a valid stream of its format in the same wave. Bit-exact against the reference executors, which c-blosc
referees for lz4 and blosclz on the CPU (tests/test_blosc_frames_model.py; snappy rests on its
executor alone). One plan per family, path and decoded size, executed twice (the second execution
lays the stream table out with k_blosc_layout); the output is prefilled with a sentinel.

Paths: narrow (two streams per wave), wide (the bitshuffle flag: one stream per wave), host input,
and the slot path (ZGPU_BLOSC_NO_DIRECT; the others write the output rows directly).

Cases per family (items with their residues in brackets): window 33 (175), ring 88, lengths 43,
pairs 12 (+ 6 batches), frames 47, finish 46, corrupt 675, lenient 7. The lenient family holds what the
decoders and c-blosc 1.21 decide differently, by design; what the GPU does with each is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest

import blosc_frames as B

pytestmark = pytest.mark.gpu

CODECS = [{"name": "bytes", "configuration": {"endian": "little"}},
          {"name": "blosc", "configuration": {"cname": "lz4", "clevel": 5, "shuffle": "noshuffle", "typesize": 1,
                                              "blocksize": 0}}]
SENTINEL = 0xA5
TAIL = 4096   # sentinel bytes after the last row
GUARD = 4096  # and before the first (a multiple of 16: the rows stay aligned)
PATHS = ("narrow", "wide", "host", "no_direct")


class Item:
    """One chunk of a call: its frame, the residue its stream's address is to have (or None), the
    verdict (OK / CORRUPT / LENIENT) and the chunk bytes expected of a status 0."""

    def __init__(self, name, frame, status, expect, size, residue=None, gpu_accepts=None, fmt=None):
        self.name, self.frame, self.status, self.expect, self.size = name, frame, status, expect, size
        self.residue, self.gpu_accepts, self.fmt = residue, gpu_accepts, fmt


@functools.lru_cache(None)
def _items(family, wide):
    out = []
    for c in B.family(family):
        if wide and not c.is_stream:
            continue  # a frame case carries its own flags
        for r in (c.residues if c.is_stream else (None,)):
            exp = None
            if c.status == B.OK or (c.status == B.LENIENT and c.gpu_accepts):
                exp = c.expect(r or 0, wide)
            out.append(Item(c.id if r is None else f"{c.id}@{r}", c.frame(r or 0, wide).data, c.status, exp, c.size,
                            r if c.is_stream else None, c.gpu_accepts, c.fmt if c.is_stream else None))
    return out


def _with_valid_neighbours(items, wide):
    """Every corrupt or lenient stream item next to a valid stream of its format and size (from the
    lengths and ring families), in the order c v v c c v v c: streams of one format pair up in list
    order, so each wave holds one of them and one valid stream, in alternating halves."""
    pool = {}
    for fam in ("lengths", "ring"):
        for it in _items(fam, wide):
            pool.setdefault((it.fmt, it.size), []).append(it)
    out, seen = [], {}
    for it in items:
        if it.status == B.OK or it.fmt is None:
            out.append(it)
            continue
        key = (it.fmt, it.size)
        k = seen[key] = seen.get(key, -1) + 1
        v = pool[key][k % len(pool[key])]
        v = Item(f"{v.name} beside {it.name}", v.frame, v.status, v.expect, v.size, v.residue, fmt=v.fmt)
        out += [it, v] if k % 2 == 0 else [v, it]
    return out


def _place(items, base):
    """Offsets of the items' frames in one buffer whose address is `base`: a stream case's payload at
    its residue, the others wherever the one before ends (unaligned on purpose)."""
    offs, off = [], 0
    for it in items:
        if it.residue is not None:
            off += (it.residue - (base + off + B.PAYLOAD_OFF)) % 16
            assert (base + off + B.PAYLOAD_OFF) % 16 == it.residue
        offs.append(off)
        off += len(it.frame)
    return offs, off


class Call:
    """One plan over `items` (all of chunk size n) with device input; host input has no plans and
    decodes with zgpu_decode_batch."""

    def __init__(self, items, n, host=False):
        import torch
        from zarrs_amd import CodecChain, Context, make_desc
        from zarrs_amd import _lib as L
        self.L, self.torch, self.items, self.n, self.k = L, torch, items, n, len(items)
        size = sum(len(it.frame) + 16 for it in items) + 64
        if host:
            self.buf = np.zeros(size, np.uint8)
            base = self.buf.ctypes.data
        else:
            self.buf = torch.zeros(size, dtype=torch.uint8, device="cuda")
            base = self.buf.data_ptr()
            assert base % 16 == 0, "the device tensor's base is not 16-byte aligned"
        offs, _ = _place(items, base)
        stage = np.zeros(size, np.uint8)
        for it, o in zip(items, offs):
            stage[o:o + len(it.frame)] = np.frombuffer(it.frame, np.uint8)
        if host:
            self.buf[:] = stage
        else:
            self.buf.copy_(torch.from_numpy(stage))
        self.ch = CodecChain.from_metadata(CODECS, "uint8", 0, Context.default())
        descs = [make_desc((base + o, len(it.frame)), [n], out_start=[i * n]) for i, (it, o) in enumerate(zip(items, offs))]
        self.arr = (L.ChunkDesc * self.k)(*descs)
        self.plan = None if host else C.c_void_p()
        if not host:
            L.check(L.load().zgpu_plan_create(self.ch._h, 1, self.arr, self.k, L.u64s([self.k * n]),
                                              L.ENC_DEVICE | L.OUT_DEVICE, C.byref(self.plan)))
        self.out = torch.empty(GUARD + self.k * n + TAIL, dtype=torch.uint8, device="cuda")

    def execute(self):
        L = self.L
        self.out.fill_(SENTINEL)
        self.torch.cuda.synchronize()
        st = (C.c_int32 * self.k)()
        if self.plan is None:
            rc = L.load().zgpu_decode_batch(self.ch._h, 1, self.arr, self.k, self.out.data_ptr() + GUARD, L.u64s([self.k * self.n]),
                                            L.OUT_DEVICE, st, None)
        else:
            rc = L.load().zgpu_plan_execute(self.plan, self.out.data_ptr() + GUARD, st, None)
        self.torch.cuda.synchronize()
        got = self.out.cpu().numpy()
        end = GUARD + self.k * self.n
        return rc, list(st), got[GUARD:end].reshape(self.k, self.n), np.concatenate([got[:GUARD], got[end:]])

    def counters(self):
        L = self.L
        ctr = (C.c_uint64 * L.N_COUNTERS)()
        if self.plan is not None:
            L.load().zgpu_plan_counters(self.plan, ctr, L.N_COUNTERS)
        else:  # host input: the calling thread's last call
            L.load().zgpu_last_counters(ctr, L.N_COUNTERS)
        return list(ctr)

    def close(self):
        if self.plan is not None:
            self.L.load().zgpu_plan_destroy(self.plan)


def _check(tag, items, rc, st, rows, tail):
    """The problems of one execution: every item's status, the bytes of every item that has to be exact,
    and the sentinels before the first row and after the last."""
    problems = []
    for i, it in enumerate(items):
        exact = it.status == B.OK
        if it.status == B.OK and st[i] != 0:
            problems.append(f"{tag}: {it.name}: status {st[i]}, expected 0")
            continue
        if it.status == B.CORRUPT and st[i] == 0:
            problems.append(f"{tag}: {it.name}: status 0 for a corrupt item")
        if it.status == B.LENIENT:
            if (st[i] == 0) != it.gpu_accepts:
                problems.append(f"{tag}: {it.name}: status {st[i]}, but gpu_accepts is {it.gpu_accepts}")
            exact = st[i] == 0 and it.expect is not None
        if exact:
            exp = np.frombuffer(it.expect, np.uint8)
            bad = np.flatnonzero(rows[i] != exp)
            if len(bad):
                p = int(bad[0])
                problems.append(f"{tag}: {it.name}: {len(bad)} wrong bytes, the first at {p} of {len(exp)} "
                                f"(got {int(rows[i][p]):#04x}, expected {int(exp[p]):#04x})")
    if any(it.status == B.CORRUPT for it in items) and rc == 0:
        problems.append(f"{tag}: return code 0 with corrupt items")
    if not (tail == SENTINEL).all():
        problems.append(f"{tag}: bytes written before the first row or past the last")
    return problems


def _by_size(items):
    g = {}
    for it in items:
        g.setdefault(it.size, []).append(it)
    return sorted(g.items())


def _run_twice(tag, items, n, host=False):
    call = Call(items, n, host)
    problems = []
    try:
        for k in (1, 2):  # the first execution reads the layout back; the second runs k_blosc_layout
            rc, st, rows, tail = call.execute()
            print(f"{tag}/{k}", "rc", rc, "non-zero statuses", sum(1 for s in st if s), "of", len(st))
            problems += _check(f"{tag}/{k}", items, rc, st, rows, tail)
        assert call.counters()[call.L.CTR_BLOSC_RERUN] == 0
    finally:
        call.close()
    return problems


# the frames and finish families hold only whole frames: their flags choose the width
_FAMILY_PATHS = [(f, p) for f in B.FAMILIES for p in PATHS if p != "wide" or f not in ("frames", "finish")]


@pytest.mark.parametrize("family,path", _FAMILY_PATHS, ids=[f"{f}-{p}" for f, p in _FAMILY_PATHS])
def test_family_on_every_path(family, path, monkeypatch):
    monkeypatch.delenv("ZGPU_BLOSC_NO_DIRECT", raising=False)
    if path == "no_direct":
        monkeypatch.setenv("ZGPU_BLOSC_NO_DIRECT", "1")
    items = _with_valid_neighbours(_items(family, path == "wide"), path == "wide")
    assert items
    problems = []
    for n, group in _by_size(items):
        problems += _run_twice(f"{family}/{path}/{n}", group, n, host=path == "host")
    assert not problems, "\n".join(problems[:60])


@pytest.mark.parametrize("name", list(B.pairs_batches()))
def test_pairs_batches(name, monkeypatch):
    """Stream tables of 1023, 1024, 1025 and 2049 entries with stored streams between the compressed
    ones (k_lz_list's rounds of 1024), and every compressor, filter and width in one call."""
    monkeypatch.delenv("ZGPU_BLOSC_NO_DIRECT", raising=False)
    n, frames, _ = B.pairs_batches()[name]
    items = [Item(f"{name}[{i}]", fr, B.OK, chunk, n) for i, (fr, chunk) in enumerate(frames)]
    problems = _run_twice(name, items, n)
    assert not problems, "\n".join(problems[:60])


def test_plan_rerun_when_the_second_batch_needs_more_streams(monkeypatch):
    """A plan over fixed device buffers: one-stream frames first, then frames of 512 streams each in
    the same buffers. The recorded layout is too small: that execution is re-run with a read-back
    layout (CTR_BLOSC_RERUN) and is exact; the small batch afterwards fits the larger layout."""
    import torch
    monkeypatch.delenv("ZGPU_BLOSC_NO_DIRECT", raising=False)
    n = 8192
    small = [Item(it.name, it.frame, it.status, it.expect, n) for it in _items("lengths", False)[:4]]
    large = [Item(f"grid{i}", fr, B.OK, chunk, n) for i, (fr, chunk) in enumerate(B.pairs_batches()["table_2049"][1][:4])]
    cap = max(len(it.frame) for it in small + large)
    call = Call([Item(it.name, it.frame.ljust(cap, b"\0"), it.status, it.expect, n) for it in small], n)
    try:
        offs, _ = _place(call.items, call.buf.data_ptr())
        for batch, rerun in ((small, 0), (small, 0), (large, 1), (large, 0), (small, 0)):
            stage = call.buf.cpu().numpy()
            for it, o in zip(batch, offs):
                stage[o:o + cap] = np.frombuffer(it.frame.ljust(cap, b"\0"), np.uint8)
            call.buf.copy_(torch.from_numpy(stage))
            rc, st, rows, tail = call.execute()
            problems = _check("rerun", batch, rc, st, rows, tail)
            assert not problems, "\n".join(problems)
            assert call.counters()[call.L.CTR_BLOSC_RERUN] == rerun
    finally:
        call.close()
