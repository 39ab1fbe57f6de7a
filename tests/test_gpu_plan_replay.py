"""The N-th execute of one plan (what bench.py times and a hipGraph capture replays) held to a fresh
decode of the same bytes, as the contents of the plan's fixed device buffers change between executes:
statuses that must not outlive a repaired input, inner chunks that became empty, streams with fewer
blocks, windows or checksum ranges than the execute before, direct rows that lose their aligned output,
counters that must not add up. The scripts are tests/plan_replay.py's (test_plan_replay_model.py holds
them to their CPU references); nothing here injects a fault: every input decodes today with a known status.

One plan per family over device tensors that never move; load() overwrites them in place. Before every
execute the output is filled with a sentinel byte that changes from execute to execute, so a write that
was skipped shows instead of being masked by the previous result. Per execute:
  (a) the statuses are the variant's, the return code the first non-zero one;
  (b) every descriptor of status 0 is bit-exact, fill regions included;
  (c) the bytes no descriptor selects still hold this execute's sentinel;
  (d) statuses and zgpu_plan_counters equal those of a fresh zgpu_decode_batch over the same bytes
      (zgpu_last_counters; every counter but BLOSC_RERUN, which only a replayed plan can set);
  (e) zgpu_last_size_mismatch names this execute's first mismatching descriptor and lengths, and is gone
      after the next clean one.
Every script runs in a quarter of a second or less on an MI355X (the longest: sharded gzip with its seven
executes, the checksum ranges with two shards of 516 KiB, bz2), the whole file in about five seconds."""
import ctypes as C

import numpy as np
import pytest

import plan_replay as R
from scatter_cases import fill_bytes

pytestmark = pytest.mark.gpu

SENTINELS = (0xA5, 0x5A, 0xC3, 0x3C, 0x96, 0x69, 0xE7, 0x7E)  # none of them a fill byte (0x11 ..)
ENV_VARS = ["ZGPU_GZIP_DIRECT", "ZGPU_GZIP_PIPE_MAX", "ZGPU_BZ2_SCRATCH_MB", "ZGPU_ZSTD_XWIN", "ZGPU_ZSTD_XPAR", "ZGPU_ZSTD_XDENSE",
            "ZGPU_ZSTD_FORCE_SERIAL", "ZGPU_TILED_PERSIST", "ZGPU_TILED_GRID", "ZGPU_BLOSC_ALIAS", "ZGPU_BLOSC_NO_DIRECT",
            "ZGPU_GROUP_LANES", "ZGPU_SCATTER_LIST", "ZGPU_GZIP_CRC_FORK"]
SLACK = 64  # bytes behind the output: the output offset by one element still lies inside its tensor


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    return Context(0)


@pytest.fixture
def env(monkeypatch):
    """set(mode environment): the variables of a mode, every other knob unset"""
    def set_(mode_env):
        for k in ENV_VARS:
            monkeypatch.delenv(k, raising=False)
        for k, v in mode_env.items():
            monkeypatch.setenv(k, v)
    set_({})
    return set_


def chain_of(ctx, fam):
    from zarrs_amd import CodecChain
    return CodecChain.from_metadata(fam.codecs, fam.dtype, fill_bytes(fam.dtype), ctx)


class Buffers:
    """A family's fixed device tensors: one blob holding every descriptor's bytes (each start one byte
    further off any alignment than the last), and the descriptors over it."""

    def __init__(self, torch, fam):
        from zarrs_amd import make_desc
        self.torch, self.fam = torch, fam
        self.off, p = [], 0
        for n in fam.lengths():
            self.off.append(p)
            p += n + 1
        self.blob = torch.zeros(max(p, 1), dtype=torch.uint8, device="cuda")
        self.descs = [make_desc((0, 0) if d.null else (self.blob.data_ptr() + o, n), list(fam.chunk_shape), list(d.sel_start),
                                list(d.sel_shape), list(d.out_start))
                      for d, o, n in zip(fam.descs, self.off, fam.lengths())]

    def load(self, variant):
        host = bytearray(self.blob.numel())
        for e, o in zip(variant.enc, self.off):
            if e is not None:
                host[o:o + len(e)] = e
        self.blob.copy_(self.torch.frombuffer(host, dtype=self.torch.uint8))
        self.torch.cuda.synchronize()


class Output:
    """A device tensor the plan writes into at `shift` bytes (0: 16-byte aligned), sentinel-filled."""

    def __init__(self, torch, fam):
        self.torch, self.fam = torch, fam
        self.nbytes = int(np.prod(fam.out_shape)) * fam.np_dtype().itemsize
        self.t = torch.zeros(self.nbytes + SLACK, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0

    def fill(self, sentinel):
        self.t.fill_(sentinel)
        self.torch.cuda.synchronize()

    def ptr(self, shift=0):
        return self.t.data_ptr() + shift

    def check(self, variant, sentinel, shift=0, what=""):
        """(b) and (c), and that nothing around the output moved"""
        self.torch.cuda.synchronize()
        fam = self.fam
        raw = self.t.cpu().numpy()
        assert (raw[:shift] == sentinel).all() and (raw[shift + self.nbytes:] == sentinel).all(), f"{what}: bytes around the output"
        got = raw[shift:shift + self.nbytes].copy().view(fam.np_dtype()).reshape(fam.out_shape)
        untouched = np.ones(fam.out_shape, bool)
        for i, (d, st, exp) in enumerate(zip(fam.descs, variant.status, variant.expect)):
            box = tuple(slice(o, o + n) for o, n in zip(d.out_start, d.sel_shape))
            untouched[box] = False
            if st == R.OK:
                assert got[box].tobytes() == exp.tobytes(), f"{what}: descriptor {i} is not the variant's bytes"
        es = fam.np_dtype().itemsize
        rest = got.reshape(-1).view(np.uint8).reshape(-1, es)[untouched.reshape(-1)]
        assert (rest == sentinel).all(), f"{what}: bytes no descriptor selects were written"


def counters_of(buf):
    return [int(x) for x in buf]


class Replay:
    """One plan of a family, executed over and over."""

    def __init__(self, torch, ctx, fam, flags=0):
        from zarrs_amd import _lib as L
        self.L, self.lib, self.torch, self.fam = L, L.load(), torch, fam
        self.ch = chain_of(ctx, fam)
        self.buf = Buffers(torch, fam)
        self.n = len(fam.descs)
        self.arr = (L.ChunkDesc * self.n)(*self.buf.descs)
        self.out = Output(torch, fam)
        self.fresh_out = Output(torch, fam)
        self.plan = C.c_void_p()
        L.check(self.lib.zgpu_plan_create(self.ch._h, len(fam.out_shape), self.arr, self.n, L.u64s(fam.out_shape),
                                          L.ENC_DEVICE | L.OUT_DEVICE | flags, C.byref(self.plan)))
        self.k = 0

    def close(self):
        if self.plan:
            self.lib.zgpu_plan_destroy(self.plan)
            self.plan = None

    def plan_counters(self):
        ctr = (C.c_uint64 * self.L.N_COUNTERS)()
        self.lib.zgpu_plan_counters(self.plan, ctr, self.L.N_COUNTERS)
        return counters_of(ctr)

    def thread_counters(self):
        ctr = (C.c_uint64 * self.L.N_COUNTERS)()
        self.lib.zgpu_last_counters(ctr, self.L.N_COUNTERS)
        return counters_of(ctr)

    def prepare(self, variant):
        """the variant's bytes in the plan's buffers, this execute's sentinel in the output"""
        self.k += 1
        self.sentinel = SENTINELS[self.k % len(SENTINELS)]
        self.buf.load(variant)
        self.out.fill(self.sentinel)

    def enqueue(self, shift=0, stream=None):
        rc = self.lib.zgpu_plan_execute(self.plan, self.out.ptr(shift), None, stream)
        assert rc == 0, self.L.last_error()

    def status(self, stream=None):
        st = (C.c_int32 * self.n)()
        rc = self.lib.zgpu_plan_status(self.plan, st, stream)
        return rc, list(st)

    def execute(self, shift=0):
        st = (C.c_int32 * self.n)()
        rc = self.lib.zgpu_plan_execute(self.plan, self.out.ptr(shift), st, None)
        return rc, list(st)

    def verify(self, variant, rc, st, what, shift=0, fresh=True):
        """(a) .. (e) of one finished execute"""
        L = self.L
        print(what, "rc", rc, "statuses", st, "counters", self.plan_counters())
        assert st == variant.status, f"{what}: statuses {st}, the variant's are {variant.status}"
        assert rc == R.rc_of(variant.status), f"{what}: return code {rc}"
        assert L.last_size_mismatch() == variant.mismatch, f"{what}: size mismatch detail {L.last_size_mismatch()}"
        mine, thread = self.plan_counters(), self.thread_counters()
        assert thread == mine, f"{what}: the thread's counters {thread} are not the plan's {mine}"
        if variant.counters is not None:  # the model's own count: a counter that adds up over executes shows here
            got = {"enc_bytes": mine[L.CTR_ENC_BYTES], "items": mine[L.CTR_ITEMS]}
            assert got == variant.counters, f"{what}: counters {got}, the model resolves {variant.counters}"
        self.out.check(variant, self.sentinel, shift, what)
        if not fresh:
            return
        self.fresh_out.fill(self.sentinel)
        st2 = (C.c_int32 * self.n)()
        rc2 = self.lib.zgpu_decode_batch(self.ch._h, len(self.fam.out_shape), self.arr, self.n, self.fresh_out.ptr(),
                                         L.u64s(self.fam.out_shape), L.ENC_DEVICE | L.OUT_DEVICE, st2, None)
        want = self.thread_counters()
        assert (rc2, list(st2)) == (rc, st), f"{what}: a fresh decode answers {rc2} {list(st2)}"
        assert L.last_size_mismatch() == variant.mismatch, f"{what}: a fresh decode's size mismatch detail"
        self.fresh_out.check(variant, self.sentinel, 0, what + " (fresh decode)")
        for k in range(L.N_COUNTERS):
            if k != L.CTR_BLOSC_RERUN:
                assert mine[k] == want[k], f"{what}: counter {k} is {mine[k]}, a fresh decode counts {want[k]} ({mine} / {want})"

    def step(self, name, what, shift=0):
        v = self.fam.variants[name]
        self.prepare(v)
        rc, st = self.execute(shift)
        self.verify(v, rc, st, what, shift)


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", R.RUNS, ids=[f"{f}-{m}" for f, m in R.RUNS])
def test_script(torch, ctx, env, name, mode):
    fam = R.family(name)
    env(fam.modes[mode])  # read when the plan is made or per execute: set before both
    r = Replay(torch, ctx, fam)
    try:
        for i, v in enumerate(fam.script):
            r.step(v, f"{name}/{mode} execute {i + 1} ({v})")
    finally:
        r.close()


@pytest.mark.parametrize("own_stream", [True, False], ids=["plan_stream", "side_stream"])
@pytest.mark.parametrize("name", ["shard_gzip_crc", "zstd_chunks_u8"])
def test_script_async(torch, ctx, env, name, own_stream):
    """zgpu_plan_execute(status = NULL), then zgpu_plan_status: on the plan's own stream (both NULL) and on
    a torch side stream passed to both; one execute per status call."""
    fam = R.family(name)
    side = None if own_stream else torch.cuda.Stream()
    s = None if own_stream else C.c_void_p(side.cuda_stream)
    r = Replay(torch, ctx, fam)
    try:
        for i, v in enumerate(fam.script):
            var = fam.variants[v]
            r.prepare(var)
            r.enqueue(0, s)
            rc, st = r.status(s)
            r.verify(var, rc, st, f"{name} async execute {i + 1} ({v})")
    finally:
        r.close()


@pytest.mark.parametrize("name", ["shard_gzip_crc", "blosc_lz4", "no_stage_tiled"])
def test_output_alignment_alternates(torch, ctx, env, name):
    """Successive executes write to a 16-byte aligned output and to the same tensor one element further:
    direct rows (k_gzip, k_blosc_finish) and the persistent tiled scatter are taken and left per execute."""
    fam = R.family(name)
    env({"ZGPU_GZIP_DIRECT": "1"} if name == "shard_gzip_crc" else {})
    es = fam.np_dtype().itemsize
    r = Replay(torch, ctx, fam)
    try:
        names = [v for v in fam.script if not any(fam.variants[v].status)]
        for i in range(6):
            shift = es * (i % 2)
            v = fam.variants[names[i % len(names)]]
            r.prepare(v)
            rc, st = r.execute(shift)
            # a fresh decode into an aligned output takes the other path on the odd executes: (d) is test_script's
            r.verify(v, rc, st, f"{name} execute {i + 1} ({v.name}) at +{shift}", shift, fresh=False)
            assert r.lib.zgpu_plan_scatter_path(r.plan) == fam.path[i % 2], (i, r.lib.zgpu_plan_scatter_path(r.plan))
    finally:
        r.close()


def test_two_plans_interleaved(torch, ctx, env):
    """Two plans of one chain on one context, their own buffers and variants, executed asynchronously in
    alternation on two streams and read afterwards: each zgpu_plan_status leaves ITS plan's size mismatch
    and counters with the thread, whatever the other plan's status call left there."""
    fam = R.family("zstd_chunks_u8")
    p, q = Replay(torch, ctx, fam), Replay(torch, ctx, fam)
    sp, sq = torch.cuda.Stream(), torch.cuda.Stream()
    cp, cq = C.c_void_p(sp.cuda_stream), C.c_void_p(sq.cuda_stream)
    try:
        for i, (vp, vq) in enumerate((("A", "B"), ("D", "D2"), ("C", "A"), ("D2", "D"), ("B", "C"))):
            a, b = fam.variants[vp], fam.variants[vq]
            p.prepare(a)
            q.prepare(b)
            p.enqueue(0, cp)
            q.enqueue(0, cq)
            rc, st = p.status(cp)
            p.verify(a, rc, st, f"plan P execute {i + 1} ({vp})", fresh=False)
            rc, st = q.status(cq)
            q.verify(b, rc, st, f"plan Q execute {i + 1} ({vq})", fresh=False)
            # a second status call for the same execute answers the same and adds nothing
            rc2, st2 = q.status(cq)
            q.verify(b, rc2, st2, f"plan Q execute {i + 1} ({vq}), read twice", fresh=False)
    finally:
        p.close()
        q.close()


@pytest.mark.parametrize("lanes", ["4", "2", "1"])
def test_group_replays(torch, ctx, env, lanes):
    """A plan group of three parts, each stepping through a script of its own for four executes, the third
    with failing descriptors in the middle part: statuses concatenated in part order, every part exact,
    the size-mismatch detail in the group's descriptor order, and the next execute clean."""
    from zarrs_amd import PlanGroup
    from zarrs_amd import _lib as L
    env({"ZGPU_GROUP_LANES": lanes})
    fams = [R.family("shard_gzip_crc"), R.zstd_chunks("u8", 3), R.family("no_stage_tiled")]
    scripts = [["A", "B", "B", "A"], ["A", "B", "D", "A"], ["A", "B", "A", "B"]]
    bufs = [Buffers(torch, f) for f in fams]
    outs = [Output(torch, f) for f in fams]
    chains = [chain_of(ctx, f) for f in fams]
    g = PlanGroup([(c, b.descs, f.out_shape) for c, b, f in zip(chains, bufs, fams)])
    try:
        assert len({lane for lane, _, _ in g.layout()}) <= int(lanes)
        ptrs = (C.c_void_p * 3)(*[o.ptr() for o in outs])
        first = [0, len(fams[0].descs), len(fams[0].descs) + len(fams[1].descs)]
        for i in range(4):
            vs = [f.variants[s[i]] for f, s in zip(fams, scripts)]
            sentinel = SENTINELS[i]
            for b, o, v in zip(bufs, outs, vs):
                b.load(v)
                o.fill(sentinel)
            rc = L.load().zgpu_group_execute(g._h, ptrs, g.status, None)
            st = list(g.status[:sum(g.n_descs)])
            want = [s for v in vs for s in v.status]
            print("lanes", lanes, "execute", i + 1, "rc", rc, "statuses", st)
            assert st == want and rc == R.rc_of(want), (i, rc, st, want)
            mm = next(((first[p] + v.mismatch[0],) + v.mismatch[1:] for p, v in enumerate(vs) if v.mismatch), None)
            assert L.last_size_mismatch() == mm, (i, L.last_size_mismatch(), mm)
            ctr = (C.c_uint64 * L.N_COUNTERS)()
            L.load().zgpu_last_counters(ctr, L.N_COUNTERS)
            assert counters_of(ctr) == g.counters(), (i, counters_of(ctr), g.counters())
            for o, v, f in zip(outs, vs, fams):
                o.check(v, sentinel, 0, f"lanes {lanes} execute {i + 1} part {f.name} ({v.name})")
    finally:
        g.close()
