"""CPU check of the blosc frames with hand-placed zstd and zlib streams (tests/blosc_inner_streams.py) that
test_gpu_blosc_inner.py feeds the blosc stage. The referee is c-blosc 1.21 through the oracle: every valid
case's frame decodes to exactly the case's chunk, every other case is refused; no case is left out
(LENIENT, the cases c-blosc and the kernels would decide differently by design, is empty). libzstd and
zlib decode every inner stream to its stated bytes. The alias rule of k_zstd_plan and the plane test of
k_blosc_finish, restated in blosc_inner_streams, give every alias case the entries and the plane
relations it was built for, and the families together hold every alias source, every plane relation
and both sides of every boundary of the rule.

Cases per family: zstd_wrapped 94, alias_planes 66, alias_rule 23, alias_layouts 49, zlib_wrapped 263
(35 corrupt), sizes 12 (8 of a wrong size), mixed 5."""
import os
import re
import zlib

import pytest

import blosc_inner_streams as I
import oracle as O
import zstd_frames as Z
import zstd_launch_model as M

_CASES = I.all_cases()
_IDS = [c.id for c in _CASES]
LENIENT = []  # ids of cases c-blosc and the kernels decide differently by design: none
COUNTS = {"zstd_wrapped": 94, "alias_planes": 66, "alias_rule": 23, "alias_layouts": 49, "zlib_wrapped": 263, "sizes": 12,
          "mixed": 5}
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zarrs_amd", "csrc")


@pytest.fixture(scope="module")
def co():
    return O.OracleChain.from_metadata([{"name": "bytes", "configuration": {"endian": "little"}},
                                        {"name": "blosc", "configuration": {"cname": "zstd", "clevel": 5, "shuffle": "noshuffle",
                                                                            "typesize": 1, "blocksize": 0}}], "uint8", 0, 1)


def _oracle(co, frame, n):
    """The chunk bytes c-blosc decodes, or None when it refuses the frame (or decodes another size)."""
    try:
        return co.decode(bytes(frame), (n,)).tobytes()
    except O.OracleError:
        return None


def test_ids_and_counts():
    assert len(set(_IDS)) == len(_IDS)
    assert {f: len(I.family(f)) for f in I.FAMILIES} == COUNTS
    assert LENIENT == []


@pytest.mark.parametrize("c", _CASES, ids=_IDS)
def test_cblosc_referees_every_case(c, co):
    got = _oracle(co, c.frame, c.size)
    if c.status == I.OK:
        assert c.expect is not None and len(c.expect) == c.size
        assert got == c.expect, f"{c.id}: c-blosc disagrees"
    else:
        assert c.expect is None and got is None, f"{c.id}: c-blosc accepts it"


@pytest.mark.parametrize("c", _CASES, ids=_IDS)
def test_stream_decoders(c):
    """libzstd and zlib decode every inner stream to its stated bytes (or refuse it: dec None); a
    stream of a wrong size decodes to that size."""
    for b, j, ne, s in c.streams():
        if s.kind == "stored":
            assert s.payload == s.dec and len(s.dec) == ne
        elif s.kind == "zstd":
            assert s.dec is not None
            assert Z.zstd_decompress(s.payload, len(s.dec) + 8) == s.dec, (c.id, b, j)
        else:
            try:
                got = zlib.decompress(s.payload)
            except zlib.error:
                got = None
            assert got == s.dec, (c.id, b, j)
        assert (c.status == I.OK) <= (s.dec is not None and len(s.dec) == ne)
    assert c.status == I.OK or any(s.dec is None or len(s.dec) != ne for _, _, ne, s in c.streams())


# ---- intent ---------------------------------------------------------------------------------------
_ALIAS = [c for c in _CASES if c.family.startswith("alias_")]


@pytest.mark.parametrize("c", _ALIAS, ids=[c.id for c in _ALIAS])
def test_alias_sets_and_planes(c):
    """Every stream of an alias case gets, by the restated rule, exactly the entries it was built for
    (offset, length and source), the rule is exact for it (no sequences of libzstd's decide), it is
    meant for the block-parallel pipeline and fits it at the blosc geometry, and a case at a named
    position has the plane relations of that position."""
    slot = I.sub_slot(max(ne for _, _, ne, _ in c.streams()))
    for b, j, ne, s in c.streams():
        assert s.kind == "zstd" and s.want is not None and s.parallel is True
        ent, exact = s.aliases()
        assert exact and ent == s.want, (c.id, b, j, ent, s.want)
        assert Z.fits_parallel(s.payload, slot), (c.id, b, j)
        assert all(o + n <= ne for o, n, _ in ent)
    lo, hi = c.alias_count()
    assert lo == hi == sum(len(s.want) for *_, s in c.streams())
    rel = c.planes()
    pos = c.tags.get("position")
    if c.family == "alias_planes":
        nonzero = {k: v for k, v in rel.items() if v != "outside"}
        want = {"on_plane": {(0, 1): "inside"},
                "inside_plane": {(0, 1): "straddle"},
                "two_planes": {(0, 1): "inside", (0, 2): "inside"} if c.ts == 4 else {(0, 0): "inside", (0, 1): "inside"},
                "mid_to_mid": {(0, 0): "straddle", (0, 1): "straddle"},
                "one_before_boundary": {(0, 0): "straddle", (0, 1): "straddle"},
                "one_after_boundary": {(0, 0): "straddle", (0, 1): "straddle"},
                "two_in_one_plane": {(0, 0): "straddle"},
                "two_in_two_planes": {(0, 0): "inside", (0, 1): "inside"},
                "rle_beside_raw": {(0, 0): "straddle", (0, 1): "straddle"}}[pos]
        assert nonzero == want, (c.id, nonzero)
        assert len(rel) == c.ts


def test_zstd_wrapped_geometry(co):
    """The wrapped zstd cases keep their capacities inside blosc: the call's sub_slot (the chunk: one
    stream per frame, one chunk size per call) gives zstd_scratch_sizes the layout each capacity case was
    built for, so every case is on the side of the scratch it was meant for; none needs rebuilding."""
    wrapped = I.family("zstd_wrapped")
    names = {c.tags["zstd_case"] for c in wrapped}
    for f in Z.FAMILIES:
        for z in Z.FAMILIES[f]():
            assert (len(z.expect) <= I.ZSTD_WRAP_MAX) == (z.name in names), z.name
    assert any(c.blocks[0][0][1].parallel is None for c in wrapped), "the serial decoder's cases go in too"
    for c in wrapped:
        (ne, s), = c.blocks[0]
        assert ne == c.size == len(s.dec) and c.ts == 1 and c.mode == 0
        assert Z.layout(I.sub_slot(ne)) == Z.layout(len(s.dec))
        sz = M.sizes(1, I.sub_slot(ne), 256, {"alias": True, "latency": False}, M.KNOBS)  # the blosc stage's ZstdWants
        assert (sz["blk_cap"], sz["lit_stride"], sz["seq_cap"]) == Z.layout(len(s.dec)) and sz["ext"] == 0
        assert Z.fits_parallel(s.payload, I.sub_slot(ne)) == (s.parallel is True), c.id
        ent, exact = s.aliases()
        assert exact, f"{c.id}: the alias count of the call is not decided by this module"


def test_coverage():
    """Every alias source, every plane relation, and both sides of every boundary of the rule."""
    planes, rule, lay = I.family("alias_planes"), I.family("alias_rule"), I.family("alias_layouts")
    for ts, _ in I.GEOMS:
        have = {(c.tags["position"], c.tags["source"]) for c in planes if c.ts == ts}
        assert {(p, s) for p in I.POSITIONS for s in I.SOURCES} <= have
        assert {"two_in_one_plane", "two_in_two_planes", "rle_beside_raw"} <= {p for p, _ in have}
        for src in I.SOURCES:  # each source inside a plane (the fast path reads it) and straddling one
            rels = {r for c in planes if c.ts == ts and c.tags["source"] == src for r in c.planes().values()}
            assert rels == {"inside", "outside", "straddle"}, (ts, src, rels)
    used = {s for c in planes + rule + lay for *_, st in c.streams() for _, _, s in st.aliases()[0]}
    assert used == set(I.SOURCES)
    by = {c.id: c for c in rule}
    for src in ("raw", "rle", "lit_raw"):  # XDIRECT
        assert [len(by[f"rule_size_{n}_{src}"].blocks[0][0][1].want) for n in (4095, 4096, 4097)] == [0, 1, 1]
    assert (I.XDIRECT - 1, I.XDIRECT, I.XDIRECT + 1) == (4095, 4096, 4097)
    for k in (3, 4):  # ZALIAS: the candidates past the second go through k_zstd_direct
        s = by[f"rule_{k}_candidates"].blocks[0][0][1]
        blks = I.stream_blocks(s.payload, s.parts)
        assert sum(b.size >= I.XDIRECT for b in blks) == k and len(s.want) == I.ZALIAS
        assert s.want == [(b.off, b.size, b.source) for b in blks if b.size >= I.XDIRECT][:2]
    for via in ("explicit", "rep0", "rep1", "rep2"):  # a later match's source: the last byte, the first after
        for word, n in (("reads_last_byte", 0), ("starts_after", 1)):
            s = by[f"rule_match_{via}_{word}"].blocks[0][0][1]
            blks = I.stream_blocks(s.payload, s.parts)
            cand = [b for b in blks if b.size >= I.XDIRECT]
            least = min(b.least for b in blks if b.least is not None and b.off > cand[0].off)
            assert len(cand) == 1 and least == cand[0].off + cand[0].size - 1 + n and len(s.want) == n
            y = [b for b in s.parts[0].blocks if b.kind == Z.CMP and len(b.seqs) == 1 and b.seqs[0][0] == 10]
            assert len(y) == 1 and (y[0].seqs[0][2] > 3) == (via == "explicit")
            assert via == "explicit" or y[0].seqs[0][2] == int(via[3]) + 1
    for ck in ("plain", "checksummed"):
        s = by[f"rule_raw_blocks_{ck}"].blocks[0][0][1]
        assert I.frames_of(s.payload)[0][0] == (ck == "checksummed") and len(s.want) == (0 if ck == "checksummed" else 2)
    assert len(I.frames_of(by["rule_two_frames"].blocks[0][0][1].payload)) >= 2
    assert by["rule_skippable_in_front"].blocks[0][0][1].payload.startswith(Z.skippable())
    layouts = {c.tags["layout"] for c in lay}
    assert layouts == {"split", "ts1", "ts3", "ts8", "ts16", "bitshuffle", "bs32776", "leftover"}
    sp = next(c for c in lay if c.tags["layout"] == "split")
    assert len(sp.blocks[0]) == 4 and all(s.want for _, s in sp.blocks[0])
    assert all(c.bs % 16 == 8 and len(c.blocks) == 2 for c in lay if c.tags["layout"] == "bs32776")
    left = [c for c in lay if c.tags["layout"] == "leftover"]
    assert {c.tags["source"] for c in left} == set(I.SOURCES)
    assert all(len(c.blocks) == 3 and c.blocks[2][0][0] == 5000 and c.blocks[2][0][1].want for c in left)
    # wrong sizes on both sides of ne and of sub_slot, for both decoders; every compressor in one call
    ne, slot = I.SIZES_NE, I.sub_slot(I.SIZES_NE)
    for kind in ("zstd", "zlib"):
        got = {c.tags["decodes_to"] for c in I.family("sizes") if c.tags["kind"] == kind and c.tags["ne"] == ne}
        assert got == {ne - 1, ne, ne + 1, slot + 1} and ne + 1 <= slot
        assert any(c.tags["decodes_to"] > 4 * slot and c.tags["ne"] < slot // 2 for c in I.family("sizes") if c.tags["kind"] == kind)
    assert all(lo == hi == 0 for lo, hi in (c.alias_count() for c in I.family("sizes")))
    assert [c.tags["kind"] for c in I.family("mixed")] == ["zstd", "zlib", "lz4", "memcpy", "zstd+stored"]
    assert len({c.size for c in I.family("mixed")}) == 1
    zl = I.family("zlib_wrapped")
    assert {c.tags.get("trailer") for c in zl} >= {"flipped", "cut"}
    assert any("split4" in c.tags for c in zl) and any(c.status != I.OK for c in zl)
    assert max(c.size for c in _CASES) <= 128 * 1024


def test_constants_are_the_kernels():
    """XDIRECT, ZALIAS and the 256-byte slot rounding, read out of the sources."""
    zstd = open(os.path.join(_CSRC, "kernels", "zstd.hip")).read()
    params = open(os.path.join(_CSRC, "kernels", "zstd_params.hpp")).read()
    plan = open(os.path.join(_CSRC, "plan_exec.cpp")).read()
    assert int(re.search(r"constexpr uint32_t XDIRECT = (\d+);", zstd).group(1)) == I.XDIRECT
    assert int(re.search(r"constexpr uint32_t ZALIAS = (\d+);", params).group(1)) == I.ZALIAS
    m = re.search(r"D\.sub_slot = \(caps\.max_ne \+ (\d+)\) & ~\(uint64_t\)(\d+);", plan)
    assert m and int(m.group(1)) == int(m.group(2)) == I.SLOT_ROUND - 1
    assert "smin >= off + osz" in zstd and "l < ao || l + neb > ao + al" in open(os.path.join(_CSRC, "kernels", "blosc.hip")).read()
