"""The write-side mirror of test_gpu_scatter_cases.py: encode_chunks (k_encode_gather aligned and
unaligned, k_encode_tiled<1,2,4,8>, the gather fallback for 16-byte elements under a transpose) for
every distinct chain and chunk shape of scatter_cases.py, byte for byte against scatter_cases.encode_ref
(held to the oracle's encoder by test_scatter_cases_model.py).

The arrays are random bytes of shape [c0 + 1, c1 + 2, ..., 2 * c_last - 1], so the grid has chunks that
cross the array's end on every axis; what lies past the end is the fill value, es distinct bytes, and
goes through the chain's byte order like the data. Rows of 2 * c_last - 1 elements leave no array row
16-byte aligned, so each case also runs on rows of 2 * c_last: k_encode_tiled's 16-byte loads."""
import numpy as np
import pytest

import scatter_cases as S
from test_gpu_encode import _Typed

pytestmark = pytest.mark.gpu

CASES = S.encode_cases()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    return Context(0)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_encode_case(ctx, torch_cuda, case):
    from zarrs_amd import CodecChain
    cs = list(case.chunk)
    ch = CodecChain.from_metadata(S.codecs_of(case), case.dtype, S.fill_bytes(case.dtype), ctx)
    for shape in S.encode_array_shapes(cs):
        a = S.random_array(f"encode-{case.name}-{shape[-1]}", case.dtype, shape)
        grid = [-(-s // c) for s, c in zip(shape, cs)]
        starts = [[i * c for i, c in zip(k, cs)] for k in np.ndindex(*grid)]
        dev = torch_cuda.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        got = ch.encode_chunks(_Typed(dev, shape, S.es_of(case.dtype)), cs, starts)
        torch_cuda.cuda.synchronize()
        assert len(got) == len(starts)
        for st, g in zip(starts, got):
            exp = S.encode_ref(S.padded_chunk(a, case.dtype, cs, st), case.orders, case.endian, case.shuffle,
                               case.crc)
            g = g.cpu().numpy().tobytes()
            assert len(g) == len(exp), (shape, st)
            if g != exp:
                d = np.flatnonzero(np.frombuffer(g, np.uint8) != np.frombuffer(exp, np.uint8))
                raise AssertionError(f"array {shape}, chunk at {st}: {len(d)} of {len(exp)} bytes differ, first at "
                                     f"{d[0]}: {g[d[0]:d[0] + 16].hex()} for {exp[d[0]:d[0] + 16].hex()}")
