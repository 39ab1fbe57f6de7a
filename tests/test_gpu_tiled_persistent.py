"""The tiled scatter of uniform whole-chunk batches (k_scatter_tiled_p) through the prepared-plan
API: every output byte for byte against the oracle's retrieve_array_subset (a byte-moving kernel
gets no tolerance), the path a plan took from zgpu_plan_scatter_path. Every case runs at the default
grid (one workgroup per unit), with ZGPU_TILED_GRID=3 (the persistent form: a few workgroups wrap
many times over uneven unit counts, loads of the next unit in flight) and with ZGPU_TILED_PERSIST=0
(k_scatter_tiled), so the old and the new paths are both held to the oracle. The control-block
epilogue the issue also describes (ZGPU_CTL_EPILOGUE) showed no gain and is not in the library, so
there is no mode for it; the control-block tests hold for the memset + copy that stays."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
from test_gpu_parity import _encode_grid

pytestmark = pytest.mark.gpu

FILL = 7
MODES = {  # environment of an execute (the switch and the grid cap are read per launch)
    "default": {},
    "grid3": {"ZGPU_TILED_GRID": "3"},
    "nopersist": {"ZGPU_TILED_PERSIST": "0"},
}

# (data type, transpose order, chunk shape, array shape): each the smallest that can still fail
ELIGIBLE = [
    ("float32", [2, 1, 0], [64, 4, 64], [128, 12, 128]),   # one unit per item
    ("float32", [2, 1, 0], [64, 8, 64], [128, 16, 128]),   # two units per item
    ("float32", [2, 1, 0], [128, 4, 64], [256, 8, 128]),   # two tiles along Lx of the encoded chunk
    ("float32", [2, 1, 0], [64, 4, 128], [128, 8, 256]),   # two tiles along A
    ("float32", [2, 1, 0], [64, 6, 64], [128, 12, 128]),   # ragged slab group (B extent 6, TJ 4)
    ("float64", [2, 1, 0], [64, 2, 64], [128, 4, 128]),    # TJ 2
    ("uint16", [2, 1, 0], [64, 4, 64], [128, 8, 128]),     # pitch + 2
    ("uint8", [1, 2, 0], [64, 4, 64], [128, 8, 128]),      # pitch + 4
    ("float32", [1, 0], [64, 64], [128, 128]),             # no B axis
    ("int32", [3, 1, 0, 2], [2, 3, 64, 64], [4, 6, 128, 128]),  # remaining axis (1), B = axis 0
]
# chunks the eligibility rule turns away: an innermost extent of 60, and the 4-D chunk whose encoded
# innermost axis (decoded axis 2 under order [3,1,0,2]) has extent 4, not a multiple of the 64-wide tile
RAGGED = [
    ("float32", [2, 1, 0], [64, 4, 60], [128, 8, 120]),
    ("int32", [3, 1, 0, 2], [2, 64, 4, 64], [4, 128, 8, 128]),
]


def _id(t):
    return f"{t[0]}_{''.join(map(str, t[1]))}_{'x'.join(map(str, t[2]))}"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    return Context(0)


@pytest.fixture
def mode(request, monkeypatch):
    for k in ("ZGPU_TILED_GRID", "ZGPU_TILED_PERSIST"):
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


all_modes = pytest.mark.parametrize("mode", list(MODES), indirect=True)


def _codecs(order):
    return [{"name": "transpose", "configuration": {"order": order}},
            {"name": "bytes", "configuration": {"endian": "big"}}]


@functools.lru_cache(maxsize=None)
def _case(dt, order, cs, shape, drop=()):
    """(oracle chain, array, encoded chunks) of a seeded array, computed once and never changed."""
    rng = np.random.default_rng(len(shape) * 1000 + cs[1] * 10 + cs[0])
    a = (rng.standard_normal(shape) * 1000).astype(np.dtype(O.DTYPES[dt][0]))
    co = O.OracleChain.from_metadata(_codecs(list(order)), dt, FILL, len(shape))
    return co, a, _encode_grid(co, a, list(cs), drop=set(drop))


def _key(t):
    return t[0], tuple(t[1]), tuple(t[2]), tuple(t[3])


class Plan:
    """A prepared plan over the chunks that intersect [start, start + sub) of the array; `enc` maps a
    chunk index to (device address, length), None for a missing chunk."""

    def __init__(self, torch, ctx, dt, order, cs, shape, enc, start=None, sub=None):
        from zarrs_amd import CodecChain, make_desc
        from zarrs_amd import _lib as L
        self.L, self.lib, self.torch = L, L.load(), torch
        nd = len(shape)
        start = start or [0] * nd
        sub = sub or list(shape)
        self.ch = CodecChain.from_metadata(_codecs(list(order)), dt, FILL, ctx)
        self.keys, descs = [], []
        lo = [s // c for s, c in zip(start, cs)]
        hi = [(s + n - 1) // c + 1 for s, n, c in zip(start, sub, cs)]
        for k in np.ndindex(*[h - l for l, h in zip(lo, hi)]):
            k = tuple(int(i + l) for i, l in zip(k, lo))
            s0 = [max(st, i * c) for st, i, c in zip(start, k, cs)]
            s1 = [min(st + n, (i + 1) * c) for st, n, i, c in zip(start, sub, k, cs)]
            descs.append(make_desc(enc.get(k), list(cs), [a - i * c for a, i, c in zip(s0, k, cs)],
                                   [b - a for a, b in zip(s0, s1)], [a - st for a, st in zip(s0, start)]))
            self.keys.append(k)
        self.n = len(descs)
        self.arr = (L.ChunkDesc * self.n)(*descs)
        self.plan = C.c_void_p()
        L.check(self.lib.zgpu_plan_create(self.ch._h, nd, self.arr, self.n, L.u64s(sub),
                                          L.ENC_DEVICE | L.OUT_DEVICE, C.byref(self.plan)))
        self.out = torch.zeros(int(np.prod(sub)) * self.ch.dtype.itemsize, dtype=torch.uint8, device="cuda")
        self.sub = sub

    def path(self):
        return self.lib.zgpu_plan_scatter_path(self.plan)

    def execute(self, with_status=True, stream=None):
        st = (C.c_int32 * self.n)()
        rc = self.lib.zgpu_plan_execute(self.plan, self.out.data_ptr(), st if with_status else None, stream)
        return rc, list(st)

    def status(self, stream=None):
        st = (C.c_int32 * self.n)()
        return self.lib.zgpu_plan_status(self.plan, st, stream), list(st)

    def result(self):
        self.torch.cuda.synchronize()
        return self.out.cpu().numpy().view(self.ch.dtype).reshape(self.sub)

    def close(self):
        self.lib.zgpu_plan_destroy(self.plan)


def _upload(torch, chunks, shift=None, short=None):
    """Device copies of the encoded chunks as {index: (address, length)} (+ the tensors that own
    them): chunk `shift` starts 4 bytes into its buffer, chunk `short` reports one element less."""
    enc, keep = {}, []
    for k, v in chunks.items():
        off = 4 if k == shift else 0
        t = torch.zeros(len(v) + 16, dtype=torch.uint8, device="cuda")
        t[off:off + len(v)] = torch.frombuffer(bytearray(v), dtype=torch.uint8).cuda()
        keep.append(t)
        enc[k] = (t.data_ptr() + off, len(v))
    if short is not None:
        enc[short] = (enc[short][0], enc[short][1] - 4)  # one f32 element
    torch.cuda.synchronize()
    return enc, keep


def _expected_path(L, mode, eligible):
    return L.SCATTER_TILED_PERSISTENT if eligible and mode != "nopersist" else L.SCATTER_TILED


@all_modes
@pytest.mark.parametrize("case", ELIGIBLE, ids=_id)
def test_whole_array_is_persistent(ctx, torch_cuda, mode, case):
    """Whole-array reads of uniform whole chunks take k_scatter_tiled_p and equal the oracle."""
    dt, order, cs, shape = case
    co, a, chunks = _case(*_key(case))
    enc, keep = _upload(torch_cuda, chunks)
    p = Plan(torch_cuda, ctx, dt, order, cs, shape, enc)
    try:
        assert p.path() == _expected_path(p.L, "default", True)  # what the plan is eligible for
        rc, st = p.execute()
        assert rc == 0 and st == [0] * p.n
        assert p.path() == _expected_path(p.L, mode, True)
        exp = O.retrieve_array_subset(co, shape, cs, chunks, [0] * len(shape), shape, nthreads=4)
        assert p.result().tobytes() == exp.tobytes()
    finally:
        p.close()


@all_modes
@pytest.mark.parametrize("case", ELIGIBLE + RAGGED, ids=_id)
def test_not_eligible(ctx, torch_cuda, mode, case):
    """A subset offset by 1 (partial selections, odd output offsets) and chunks of ragged tiles keep the
    one-unit-per-workgroup kernel, whatever the switches say, and still equal the oracle."""
    dt, order, cs, shape = case
    co, a, chunks = _case(*_key(case))
    enc, keep = _upload(torch_cuda, chunks)
    reads = [([1] * len(shape), [s - 2 for s in shape])]
    if case in RAGGED:
        reads.append(([0] * len(shape), list(shape)))
    for start, sub in reads:
        p = Plan(torch_cuda, ctx, dt, order, cs, shape, enc, start, sub)
        try:
            rc, st = p.execute()
            assert rc == 0 and st == [0] * p.n
            assert p.path() == p.L.SCATTER_TILED
            exp = O.retrieve_array_subset(co, shape, cs, chunks, start, sub, nthreads=4)
            assert p.result().tobytes() == exp.tobytes(), (start, sub)
        finally:
            p.close()


FB = ("float32", [2, 1, 0], [64, 8, 64], [128, 16, 128])  # 8 chunks of two units each
MISSING, SHIFTED, SHORT = (1, 0, 0), (0, 1, 1), (1, 1, 0)
SENTINEL = 0xA5


def _fallback_plan(torch, ctx, short=True):
    dt, order, cs, shape = FB
    co, a, chunks = _case(dt, tuple(order), tuple(cs), tuple(shape), (MISSING,))
    enc, keep = _upload(torch, chunks, shift=SHIFTED, short=SHORT if short else None)
    p = Plan(torch, ctx, dt, order, cs, shape, enc)
    p.keep = keep
    exp = O.retrieve_array_subset(co, shape, cs, chunks, [0, 0, 0], shape, nthreads=4)
    return p, exp


def _check_fallbacks(p, exp, rc, st, short=True):
    """Statuses and bytes of the plan with one missing, one misaligned and (short) one short chunk."""
    L, cs = p.L, FB[2]
    want = [L.DECODED_SIZE_MISMATCH if (short and k == SHORT) else 0 for k in p.keys]
    assert st == want and rc == (L.DECODED_SIZE_MISMATCH if short else 0)
    got = p.result()
    box = tuple(slice(i * c, (i + 1) * c) for i, c in zip(SHORT, cs))
    if short:  # the short chunk's region of the pre-filled output is untouched, every other chunk exact
        sent = np.frombuffer(bytes([SENTINEL]) * 4, dtype=got.dtype)[0]
        assert (got[box].view(np.uint32) == sent.view(np.uint32)).all()
        exp = exp.copy()
        exp[box] = sent
    miss = tuple(slice(i * c, (i + 1) * c) for i, c in zip(MISSING, cs))
    assert (got[miss] == FILL).all()
    assert got.tobytes() == exp.tobytes()


@all_modes
def test_per_unit_fallbacks(ctx, torch_cuda, mode):
    """Inside one k_scatter_tiled_p launch: a missing chunk is filled, a chunk whose bytes start 4 bytes into
    its buffer goes through the element-wise body, a chunk one element short reports
    DECODED_SIZE_MISMATCH and leaves its region alone."""
    p, exp = _fallback_plan(torch_cuda, ctx)
    try:
        p.out.fill_(SENTINEL)
        rc, st = p.execute()
        assert p.path() == _expected_path(p.L, mode, True)
        _check_fallbacks(p, exp, rc, st)
    finally:
        p.close()


@all_modes
def test_control_block(ctx, torch_cuda, mode):
    """The control block across executes: the same statuses three times in a row, through
    zgpu_plan_status after an execute without statuses, and on a second stream."""
    torch = torch_cuda
    p, exp = _fallback_plan(torch, ctx)
    try:
        for _ in range(3):
            p.out.fill_(SENTINEL)
            torch.cuda.synchronize()
            rc, st = p.execute()
            _check_fallbacks(p, exp, rc, st)
        p.out.fill_(SENTINEL)
        torch.cuda.synchronize()
        rc, _ = p.execute(with_status=False)
        assert rc == 0
        rc, st = p.status()
        _check_fallbacks(p, exp, rc, st)
        s2 = torch.cuda.Stream()
        p.out.fill_(SENTINEL)
        torch.cuda.synchronize()
        rc, st = p.execute(stream=s2.cuda_stream)
        _check_fallbacks(p, exp, rc, st)
        rc, _ = p.execute(with_status=False, stream=s2.cuda_stream)
        assert rc == 0
        rc, st = p.status(stream=s2.cuda_stream)
        _check_fallbacks(p, exp, rc, st)
    finally:
        p.close()


@all_modes
def test_good_plan_after_bad(ctx, torch_cuda, mode):
    """A good plan executed after a bad one reports all zeros (nothing of the bad plan's control block
    is left behind), and the bad one still reports its own afterwards."""
    bad, exp_bad = _fallback_plan(torch_cuda, ctx)
    good, exp = _fallback_plan(torch_cuda, ctx, short=False)
    try:
        bad.out.fill_(SENTINEL)
        rc, st = bad.execute()
        _check_fallbacks(bad, exp_bad, rc, st)
        for _ in range(2):
            rc, st = good.execute()
            _check_fallbacks(good, exp, rc, st, short=False)
        torch_cuda.cuda.synchronize()
        rc, st = bad.execute()
        _check_fallbacks(bad, exp_bad, rc, st)
    finally:
        bad.close()
        good.close()
