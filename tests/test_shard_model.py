"""The shard model (tests/shard_model.py) against what it does not share code with: crc32c known answers
and the oracle's crc32c, the reference's own sharded fixture (written by zarrs, chunk 1 stored before
chunk 0), the oracle's writer for the canonical layout, and then the oracle's reader held to the model
on every case of the table, as a full decode and as each partial selection. CPU only."""
import itertools

import numpy as np
import pytest

import fixtures as F
import oracle as O
import shard_model as S
from scatter_cases import fill_bytes


def test_crc32c():
    # the two known answers of test_oracle_golden.py (crc32c.rs:100-127; RFC 3720's check value)
    assert S.crc32c(bytes(range(6))).to_bytes(4, "little") == bytes([20, 133, 9, 65])
    assert S.crc32c(b"123456789") == 0xE3069283
    rng = np.random.default_rng(0)
    for n in range(71):
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert S.crc32c(b) == O.crc32c(b), n


def test_junk_is_never_zero_and_index_round_trips():
    assert all(S.junk(300, s).count(0) == 0 for s in range(9))
    ent = [(5, 7), (S.MAX, S.MAX), (2 ** 40, 1), (S.MAX, 3)]
    for endian, crcs in itertools.product(("little", "big"), ((), ("end",), ("start",), ("end", "start", "end", "end"))):
        raw = S.pack_index(ent, endian, crcs)
        assert len(raw) == S.index_bytes(4, crcs)
        assert S.parse_index(raw, 4, endian, crcs) == ent
        for i, p in enumerate(S.crc_positions(4, crcs)):
            bad = bytearray(raw)
            bad[p] ^= 1
            assert S.parse_index(bytes(bad), 4, endian, crcs) == S.INVALID_CHECKSUM, (crcs, i)
            assert S.parse_index(bytes(bad), 4, endian, crcs, validate=False) == ent
    # the layout of the words, spelled out: offset then size, entry after entry
    assert S.pack_index([(1, 2), (3, 4)], "little", ()) == b"".join(v.to_bytes(8, "little") for v in (1, 2, 3, 4))
    assert S.pack_index([(1, 2)], "big", ("start",))[4:] == (1).to_bytes(8, "big") + (2).to_bytes(8, "big")


def test_zero_bytes_status_per_chain():
    for ch in S.CHAINS:
        assert S.decode_inner(ch, b"", (2, 3), "uint16", True, False)[0] == ch.zero_status(), ch.name


FIX = S.Shard((4, 4), S.Chain("fixture", b2b=("gzip",)))


def test_model_reads_reference_fixture():
    m, chunks = F.load_array(F.SHARDED)
    assert m["codecs"][0]["configuration"]["chunk_shape"] == [4, 4] and m["chunk_shape"] == [4, 8]
    exp = np.arange(64, dtype=np.uint16).reshape(8, 8)
    for (i, j), enc in sorted(chunks.items()):
        st, got, stats = S.read_shard(FIX, (4, 8), "uint16", enc)
        assert st == 0 and np.array_equal(got, exp[4 * i:4 * i + 4])
        st, got, _ = S.read_shard(FIX, (4, 8), "uint16", enc, ((1, 3), (2, 3)))
        assert st == 0 and np.array_equal(got, exp[4 * i + 1:4 * i + 3, 3:6])


def test_build_shard_reproduces_reference_fixture():
    _, chunks = F.load_array(F.SHARDED)
    for key in ((0, 0), (1, 0)):
        enc = chunks[key]
        ent = S.entries_of(FIX, (4, 8), enc)
        order = tuple(sorted(range(2), key=lambda k: S.parse_index(enc[-36:], 2, "little", ("end",))[k][0]))
        if key == (0, 0):
            assert order == (1, 0)  # zarrs stored chunk 1 first
        shard, _ = S.build_shard(ent, S.Layout(order=order), "end", ("little", ("end",)))
        assert shard == enc


CANON_CHAINS = [S.LE, S.BE, S.LE_CRC, S.TR_BE, S.Chain("bytes_crc_start", b2b=("crc32c_start",))]


@pytest.mark.parametrize("chain", CANON_CHAINS, ids=[c.name for c in CANON_CHAINS])
@pytest.mark.parametrize("endian", ["little", "big"])
@pytest.mark.parametrize("location", ["start", "end"])
def test_canonical_layout_equals_oracle_writer(chain, endian, location):
    for dt, shape, inner, crcs in (("uint16", (4, 6), (2, 3), ("end",)), ("float64", (4, 4, 6), (2, 2, 3), ()),
                                   ("uint8", (6, 3), (2, 3), ("start", "end"))):
        if chain.order and len(shape) != 2:
            continue
        sh = S.Shard(inner, chain, location=location, endian=endian, crcs=crcs, empty=frozenset((1,)))
        case = S.Case("canon", "canon", dt, shape, sh)
        a, enc = case.built()
        oc = O.OracleChain.from_metadata(case.codecs(), dt, fill_bytes(dt), len(shape))
        assert oc.encode(a) == enc


def _oracle(case, sel, validate):
    """(status, array) of the oracle's read: the shard as the one chunk of an array of its shape"""
    a, enc = case.built()
    oc = O.OracleChain.from_metadata(case.codecs(), case.dtype, fill_bytes(case.dtype), len(case.shape))
    try:
        if sel is None:
            return 0, oc.decode(enc, case.shape, validate)
        return 0, O.retrieve_array_subset(oc, case.shape, case.shape, {tuple([0] * len(case.shape)): enc},
                                          list(sel[0]), list(sel[1]), validate_checksums=validate)
    except O.OracleError as e:
        return e.status, None


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_oracle_agrees_with_model(case):
    a, enc = case.built()
    for sel in (None,) + case.sels:
        st, exp, stats = case.expect(sel)
        got_st, got = _oracle(case, sel, case.validate)
        assert got_st == st, (sel, O.STATUS_NAMES[got_st], O.STATUS_NAMES[st])
        if st == 0:
            assert got.tobytes() == exp.tobytes(), sel
            if not case.shard.flip:  # nothing corrupt: the model's read is the slice of the array
                box = tuple(slice(s, s + n) for s, n in zip(*sel)) if sel else ...
                assert exp.tobytes() == np.ascontiguousarray(a[box]).tobytes(), sel


def test_table_reaches_what_it_claims():
    """The cases' own claims, so that a change to the builder cannot quietly empty them."""
    B = S.BY_NAME
    _, enc = B["ends_at_len_in_index"].built()
    ent = S.parse_index(enc[-68:], 4, "little", ("end",))
    assert ent[1][0] + ent[1][1] == len(enc) and ent[1][0] > len(enc) - 68
    _, enc = B["entry_into_index"].built()
    assert S.parse_index(enc[:68], 4, "little", ("end",))[3] == (16, 16)
    _, enc = B["all_empty_end"].built()
    assert len(enc) == S.index_bytes(4, ("end",)) and B["all_empty_end"].expect()[0] == 0
    _, enc = B["overlap_half"].built()
    ent = S.parse_index(enc[-68:], 4, "little", ("end",))
    assert ent[2][0] == ent[1][0] + ent[1][1] // 2
    for name in ("gaps_1_3_17_start", "gaps_17_1_3_permuted_end", "reversed_bytes_gzip_crc", "three_hundred"):
        c = B[name]
        _, enc = c.built()
        n = int(np.prod(c.shard.grid(c.shape)))
        x = S.index_bytes(n, c.shard.crcs)
        idx = S.parse_index(enc[:x] if c.shard.location == "start" else enc[-x:], n, c.shard.endian, c.shard.crcs)
        if c.shard.layout.order is not None:  # stored out of C order
            assert [o for o, _ in idx] != sorted(o for o, _ in idx), name
        if c.shard.layout.gap:  # junk between the stored inner chunks, so the sizes do not fill the body
            base = x if c.shard.location == "start" else 0
            assert sum(s for _, s in idx) < len(enc) - x and min(o for o, _ in idx) == base + c.shard.layout.pre, name
    for c in S.CASES:  # every case names every reader, and a refusal carries its reason
        r = S.readers(c)
        assert set(r) == set(S.READERS) and all(v is None or isinstance(v, str) for v in r.values())
        assert (r["store"] is not None) == (c.shard.depth() > 1)
    # every status the table expects, full and partial
    seen = {c.expect(sel)[0] for c in S.CASES for sel in (None,) + c.sels}
    assert seen >= {S.OK, S.INVALID_CHECKSUM, S.DECODED_SIZE_MISMATCH, S.SHARD_INDEX_OOB, S.CRC_INPUT_TOO_SHORT,
                    S.SHARD_TOO_SMALL}
    # the poisoned cases: every partial selection reads, the full read fails
    for c in S.CASES:
        if c.group == "partial":
            assert c.expect()[0] != 0 and all(c.expect(sel)[0] == 0 for sel in c.sels), c.name
