"""The final decode stage (scatter.hip) on the GPU, one test per case of scatter_cases.py: each case is
there for one branch of k_scatter_rows / k_scatter_tiled / k_scatter_generic, the reference is a slice
of the case's numpy array (scatter_cases.expected, held to the oracle by test_scatter_cases_model.py),
and every comparison is on bytes.

Every selection is decoded into a buffer with a border on every side of every axis, pre-filled with
0xA5: the box must equal the reference and every byte outside it must still be 0xA5 (a vector store
one lane past a ragged row shows). Two border layouts, because a border of one element puts every
output row of a type narrower than 8 bytes off the 16-byte boundaries the vector branches need:
  border1   one element on every side, out_start = [1] * nd (element paths for es < 8)
  border16  the same, but 16 bytes (at least one element) before and after each row, on a 16-byte
            aligned buffer: output rows are 16-byte aligned wherever the selection's rows are
Each plan runs twice into a re-poisoned buffer, from device-resident encoded chunks (through a
prepared plan, whose zgpu_plan_scatter_path must be the case's) and from host bytes (decode_batch)."""
import ctypes as C

import numpy as np
import pytest

import scatter_cases as S

pytestmark = pytest.mark.gpu

LAYOUTS = ("border1", "border16")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    return Context(0)


def _border(case, layout):
    b = [1] * len(case.chunk)
    if layout == "border16":
        b[-1] = max(1, 16 // S.es_of(case.dtype))
    return b


def _upload(torch, case, chunks):
    """The encoded chunks in one device buffer, each src_off bytes past a 256-byte boundary:
    {grid index: (address, length)} and the tensor that owns them."""
    pitch = lambda n: (n + case.src_off + 255) // 256 * 256  # noqa: E731
    host = np.zeros(sum(pitch(len(v)) for v in chunks.values()) + 256, np.uint8)
    at, pos = {}, 0
    for k, v in chunks.items():
        host[pos + case.src_off:pos + case.src_off + len(v)] = np.frombuffer(v, np.uint8)
        at[k] = (pos + case.src_off, len(v))
        pos += pitch(len(v))
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 256 == 0
    return {k: (dev.data_ptr() + o, n) for k, (o, n) in at.items()}, dev


def _descs(case, start, shape, border, enc):
    """Descriptors of the chunks that intersect [start, start + shape), written border elements into
    the output; `enc` maps a grid index to (address, length) or bytes, a missing chunk is absent."""
    from zarrs_amd import make_desc
    cs = case.chunk
    lo = [s // c for s, c in zip(start, cs)]
    hi = [(s + n - 1) // c + 1 for s, n, c in zip(start, shape, cs)]
    out = []
    for k in np.ndindex(*[h - l for l, h in zip(lo, hi)]):
        k = tuple(int(i + l) for i, l in zip(k, lo))
        s0 = [max(st, i * c) for st, i, c in zip(start, k, cs)]
        s1 = [min(st + n, (i + 1) * c) for st, n, i, c in zip(start, shape, k, cs)]
        out.append(make_desc(enc.get(k), list(cs), [a - i * c for a, i, c in zip(s0, k, cs)],
                             [b - a for a, b in zip(s0, s1)], [a - st + bd for a, st, bd in zip(s0, start, border)]))
    return out


def _check(torch, out, case, start, shape, border, what):
    """The box is the reference, everything around it the sentinel."""
    torch.cuda.synchronize()
    es = S.es_of(case.dtype)
    full = [n + 2 * b for n, b in zip(shape, border)]
    got = out.cpu().numpy().reshape(full + [es]).copy()
    box = tuple(slice(b, b + n) for b, n in zip(border, shape))
    exp = np.frombuffer(S.expected(case.name, start, shape), np.uint8).reshape(list(shape) + [es])
    bad = np.argwhere((got[box] != exp).any(axis=-1))
    assert got[box].tobytes() == exp.tobytes(), \
        f"{what}: {len(bad)} of {exp.size // es} elements differ, first at {bad[0].tolist()}: " \
        f"{got[box][tuple(bad[0])].tobytes().hex()} for {exp[tuple(bad[0])].tobytes().hex()}"
    got[box] = S.SENTINEL
    out_of_box = np.argwhere((got != S.SENTINEL).any(axis=-1))
    assert not len(out_of_box), f"{what}: {len(out_of_box)} elements outside the box written, first at " \
                                f"{out_of_box[0].tolist()} (box {list(border)} + {list(shape)})"


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_case(ctx, torch_cuda, monkeypatch, case):
    from zarrs_amd import CodecChain
    from zarrs_amd import _lib as L
    torch, lib = torch_cuda, L.load()
    if case.wide is None:
        monkeypatch.delenv("ZGPU_UNSHUFFLE_WIDE", raising=False)
    else:
        monkeypatch.setenv("ZGPU_UNSHUFFLE_WIDE", case.wide)
    chunks = S.case_data(case.name)[2]
    ch = CodecChain.from_metadata(S.codecs_of(case), case.dtype, S.fill_bytes(case.dtype), ctx)
    assert ch.dtype.itemsize == S.es_of(case.dtype)
    enc, keep = _upload(torch, case, chunks)
    nd = len(case.chunk)
    for layout in LAYOUTS:
        border = _border(case, layout)
        for start, shape in case.sels:
            what = f"{layout} {list(start)}+{list(shape)}"
            full = [n + 2 * b for n, b in zip(shape, border)]
            out = torch.empty(int(np.prod(full)) * S.es_of(case.dtype), dtype=torch.uint8, device="cuda")
            assert out.data_ptr() % 16 == 0
            descs = _descs(case, start, shape, border, enc)
            n = len(descs)
            arr = (L.ChunkDesc * n)(*descs)
            plan = C.c_void_p()
            L.check(lib.zgpu_plan_create(ch._h, nd, arr, n, L.u64s(full), L.ENC_DEVICE | L.OUT_DEVICE,
                                         C.byref(plan)))
            try:
                assert S.PATH_NAMES[lib.zgpu_plan_scatter_path(plan)] == S.PATH_NAMES[case.path], what
                for run in (1, 2):
                    out.fill_(S.SENTINEL)
                    torch.cuda.synchronize()
                    st = (C.c_int32 * n)()
                    rc = lib.zgpu_plan_execute(plan, out.data_ptr(), st, None)
                    assert rc == 0 and list(st) == [0] * n, (what, run, L.last_error())
                    assert S.PATH_NAMES[lib.zgpu_plan_scatter_path(plan)] == S.PATH_NAMES[case.path], what
                    _check(torch, out, case, start, shape, border, f"{what} device run {run}")
            finally:
                lib.zgpu_plan_destroy(plan)
            out.fill_(S.SENTINEL)
            torch.cuda.synchronize()
            st = ch.decode_batch(_descs(case, start, shape, border, chunks), out, full, enc_device=False)
            assert st == [0] * n, what
            _check(torch, out, case, start, shape, border, f"{what} from host bytes")
    del keep
