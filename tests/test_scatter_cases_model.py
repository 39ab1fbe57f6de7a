"""scatter_cases.py held to the C oracle and to its own table. No GPU: this pins the reference and the
cases that test_gpu_scatter_cases.py and test_gpu_encode_cases.py feed the kernels.

The oracle (pinned by the reference project's fixtures) has no bfloat16; a bfloat16 case is held to
the uint16 chain over the same bytes."""
import numpy as np
import pytest

import oracle as O
import scatter_cases as S

IDS = [c.name for c in S.CASES]


def _oracle(case):
    dt = "uint16" if case.dtype == "bfloat16" else case.dtype
    return O.OracleChain.from_metadata(S.codecs_of(case), dt, S.fill_bytes(case.dtype), len(case.chunk))


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_encode_ref_is_the_oracles_encode(case):
    co = _oracle(case)
    a, _, chunks = S.case_data(case.name)
    assert set(chunks) == set(np.ndindex(*case.grid)) - case.drop
    for k, enc in chunks.items():
        blk = np.ascontiguousarray(a[tuple(slice(i * n, (i + 1) * n) for i, n in zip(k, case.chunk))])
        assert co.encode(blk) == enc, k
        assert co.decode(enc, case.chunk).tobytes() == blk.tobytes(), k


@pytest.mark.parametrize("case", S.encode_cases(), ids=[c.name for c in S.encode_cases()])
def test_edge_chunks_against_the_oracle(case):
    """The write side's chunks, the ones that cross the array's end included."""
    co = _oracle(case)
    fv = S.fill_bytes(case.dtype)
    for shape in S.encode_array_shapes(case.chunk):
        a = S.random_array(f"encode-{case.name}-{shape[-1]}", case.dtype, shape)
        grid = [-(-s // c) for s, c in zip(shape, case.chunk)]
        crossing = 0
        for k in np.ndindex(*grid):
            st = [i * c for i, c in zip(k, case.chunk)]
            blk = S.padded_chunk(a, case.dtype, case.chunk, st)
            if any(s + c > n for s, c, n in zip(st, case.chunk, shape)):
                crossing += 1
                assert blk.tobytes()[-len(fv):] == fv  # the last element lies past the end
            assert co.encode(blk) == S.encode_ref(blk, case.orders, case.endian, case.shuffle, case.crc), k
        assert crossing or len(shape) == 1


def test_expected_is_a_slice_of_the_array():
    """A selection's reference bytes: the array's, and the fill value inside a missing chunk."""
    c = S.BY_NAME["rows-vec-complex128-le-3x5x2"]
    a, ref, _ = S.case_data(c.name)
    assert S.expected(c.name, [0, 0, 0], c.chunk) == np.ascontiguousarray(a[:3, :5, :2]).tobytes()
    assert c.drop == {(1, 1, 1)}
    assert S.expected(c.name, [3, 5, 2], c.chunk) == S.fill_bytes("complex128") * 30
    assert S.fill_bytes("complex128") == bytes(range(0x11, 0x21))


def test_contents_are_raw_bytes():
    """Random bytes, not random values: NaNs and bools other than 0 / 1 are in the arrays."""
    a = np.concatenate([S.case_data(c.name)[0].reshape(-1) for c in S.CASES if c.dtype == "float32"])
    assert np.isnan(a).any()
    b = np.concatenate([S.case_data(c.name)[0].reshape(-1) for c in S.CASES if c.dtype == "bool"])
    assert (b.view(np.uint8) > 1).any()


def test_every_cell_has_a_case():
    have = {(c.group, c.dtype) for c in S.CASES}
    missing = [(g, dt) for g, dts in S.CELLS.items() for dt in dts if (g, dt) not in have]
    assert not missing
    assert {c.group for c in S.CASES} == set(S.CELLS)
    for g in ("rows-vec", "rows-elem", "tiled-small"):  # both byte orders where the table asks for them
        for dt in S.CELLS[g]:
            assert any(c.group == g and c.dtype == dt and c.endian == "big" for c in S.CASES), (g, dt)
    for dt in S.CELLS["unshuffle-wide"]:
        for endian in ("little", "big"):
            assert {c.wide for c in S.CASES if c.group == "unshuffle-wide" and c.dtype == dt and
                    c.endian == endian} == {None, "1", "2"}


def test_every_note_names_its_own_branch():
    notes = [c.note for c in S.CASES]
    assert all(notes) and len(set(notes)) == len(notes)


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_case_is_well_formed(case):
    nd = len(case.chunk)
    assert case.path == S.model_path(case)
    assert len(case.array) == nd and all(a % c == 0 for a, c in zip(case.array, case.chunk))
    assert all(k in set(np.ndindex(*case.grid)) for k in case.drop)
    moved = 0
    for start, shape in case.sels:
        assert all(n > 0 and s + n <= a for s, n, a in zip(start, shape, case.array))
        moved = max(moved, int(np.prod(shape)) * S.es_of(case.dtype))
    assert moved < 1 << 20
    if case.src_off:
        assert not case.crc and case.grid == (1,) * nd
    if case.path == S.TILED:
        # never the persistent form test_gpu_tiled_persistent.py pins: ragged tiles, or no item whole
        a_axis = S.composed_axes(case.orders, nd)[-1]
        ragged = case.chunk[a_axis] % 64 or case.chunk[-1] % 64
        partial = all(any(s % c or (s + n) % c for s, n, c in zip(start, shape, case.chunk))
                      for start, shape in case.sels)
        assert ragged or partial


def test_python_mirror_names_every_type():
    """zarrs_amd.codec names every type of chain.cpp's table at its size; bfloat16 as two opaque bytes."""
    from zarrs_amd import codec
    for dt, (_, es, _) in S.TYPES.items():
        assert np.dtype(codec.DTYPES[dt]).itemsize == es, dt
        assert codec.fill_value_bytes(dt, S.fill_bytes(dt)) == S.fill_bytes(dt)
    assert codec.fill_value_bytes("bfloat16", 0) == b"\0\0"
    assert codec.fill_value_bytes("bfloat16", "0x3f80") == b"\x80\x3f"
    with pytest.raises(ValueError):
        codec.fill_value_bytes("bfloat16", 1.5)
