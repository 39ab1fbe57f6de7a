"""CPU check of the hand-built blosc frames (tests/blosc_frames.py) that test_gpu_blosc_frames.py feeds the
blosc kernels. For lz4 and blosclz the referee is c-blosc 1.21 through the oracle: every valid case's
frame (narrow and wide form) decodes to exactly the case's expected chunk bytes, every corrupt case
raises, every lenient case raises while the reference executor decodes it. Every stream case's intent
holds in the model of LzG at every residue the case claims, with both lane-group widths.

Snappy parity rests on the reference executor alone: the host c-blosc is built without snappy and
no snappy library is installed. The executor is pinned by decoding what the seeded snappy encoder
that test_gpu_blosc.py uses writes back to its input, and by agreeing with the LZ4 executor (which c-blosc
referees) on token lists that both formats express."""
import numpy as np
import pytest

import blosc_frames as B
import oracle as O

_CASES = B.all_cases()
_IDS = [c.id for c in _CASES]


@pytest.fixture(scope="module")
def co():
    return O.OracleChain.from_metadata([{"name": "bytes", "configuration": {"endian": "little"}},
                                        {"name": "blosc", "configuration": {"cname": "lz4", "clevel": 5, "shuffle": "noshuffle",
                                                                            "typesize": 1, "blocksize": 0}}], "uint8", 0, 1)


def _oracle(co, frame, n):
    """The chunk bytes c-blosc decodes, or None when it refuses the frame (or decodes another size)."""
    try:
        return co.decode(bytes(frame), (n,)).tobytes()
    except O.OracleError:
        return None


def _cblosc_can(c):
    f = c.frame().data
    return len(f) < 16 or f[2] & 2 or f[2] >> 5 != B.COMP["snappy"]


@pytest.mark.parametrize("c", _CASES, ids=_IDS)
def test_case_verdict_and_intent(c, co):
    assert c.is_stream or not c.intent
    for r in (c.residues if c.is_stream else (0,)):
        ex = c.executed(r) if c.is_stream else None
        for wide in ((False, True) if c.is_stream else (False,)):
            fr = c.frame(r, wide).data
            if c.status == B.OK:
                want = c.expect(r, wide)
                assert len(want) == c.size
                if _cblosc_can(c):
                    assert _oracle(co, fr, c.size) == want, f"{c.id}: c-blosc disagrees (r {r}, wide {wide})"
            else:
                if _cblosc_can(c) and not c.cblosc_unspecified:
                    assert _oracle(co, fr, c.size) is None, f"{c.id}: c-blosc accepts it"
                if c.status == B.LENIENT and not c.is_stream:
                    assert len(c.expect_bytes) == c.size
                elif c.status == B.LENIENT and not c.cblosc_unspecified:
                    assert ex[0] == B.OK and len(ex[1]) == (c.ne or c.size), c.id
                elif c.is_stream:  # the executor is the only referee of snappy: it must refuse, or decode another size
                    assert ex[0] == B.CORRUPT or len(ex[1]) != (c.ne or c.size), c.id
        if not c.is_stream:
            continue
        for G in (B.G_NARROW, B.G_WIDE):
            t = B.model(c.fmt, c.stream(r), r, G, c.cap or c.size)
            if c.status == B.OK:
                assert not t.err and t.out == ex[1], f"{c.id}: the model and the executor differ"
            for text, pred in c.intent:
                assert pred(t), f"{c.id}: the model (r {r}, G {G}) does not show: {text}"
            if c.status == B.LENIENT:
                assert t.err != c.gpu_accepts, f"{c.id}: the model of the kernel"


def test_no_duplicate_ids_or_traces():
    assert len(set(_IDS)) == len(_IDS)
    seen, dups = {}, []
    for c in _CASES:
        if not c.is_stream or c.status != B.OK:
            continue
        t = B.model(c.fmt, c.stream(c.residues[0]), c.residues[0], B.G_NARROW, c.size)
        key = (c.fmt, repr(t.fills), repr(t.lits), repr(t.matches))
        if key in seen and c.same_trace_as != seen[key]:
            dups.append((c.id, seen[key]))
        seen.setdefault(key, c.id)
    assert not dups, f"cases with equal traces: {dups}"


def test_constants_are_the_kernels():
    """LZW, LZR and G_NARROW are the defaults of ZG_LZW, ZG_LZ_RING and ZG_LZM_G in blosc.hip."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zarrs_amd", "csrc", "kernels",
                            "blosc.hip")).read()
    got = {k: int(re.search(rf"#define {k} (\d+)", src).group(1)) for k in ("ZG_LZW", "ZG_LZ_RING", "ZG_LZM_G")}
    assert got == {"ZG_LZW": B.LZW, "ZG_LZ_RING": B.LZR, "ZG_LZM_G": B.G_NARROW}
    assert B.G_WIDE == 64  # k_*m<64>: the wide path's lane group is the wave


def test_families_cover_both_sides():
    for f in B.FAMILIES:
        assert B.family(f), f
    ring = {c.id for c in B.family("ring")}
    for fmt in B.FMTS:
        assert {f"ring_{fmt}_off_plus_ml_LZR{d:+d}" for d in (-1, 0, 1)} <= ring
    assert all(c.status == B.LENIENT for c in B.family("lenient"))
    assert not any(c.status == B.LENIENT for f in B.FAMILIES if f != "lenient" for c in B.family(f))
    assert all(set(c.residues) >= {0, 1, 15} for c in B.family("window") if len(c.residues) > 1)
    for fmt in B.FMTS:
        assert any(c.fmt == fmt and c.residues == B.ALL_R for c in B.family("window"))


def test_pairs_batches(co):
    for name, (n, items, table) in B.pairs_batches().items():
        assert table is None or sum(B.count_streams(fr) for fr, _ in items) == table, name
        if name == "one_token_beside_thousands_odd_count":  # every frame one stream: the lists follow the items' order
            assert all(B.count_streams(fr) == 1 for fr, _ in items) and len(items) == 3 * len(B.FMTS)
            for i, (fr, _) in enumerate(items):
                fmt, k = B.FMTS[i // 3], i % 3
                p = int.from_bytes(fr[16:20], "little")
                t = B.model(fmt, fr[p + 4:p + 4 + int.from_bytes(fr[p:p + 4], "little")], 0, B.G_NARROW)
                assert fr[2] >> 5 == B.COMP[fmt] and (len(t.matches) > 1000) == (k == 1), (name, i)
        for fr, chunk in items:
            assert len(chunk) == n
            if fr[2] >> 5 != B.COMP["snappy"]:
                assert _oracle(co, fr, n) == chunk, name


@pytest.mark.parametrize("seed", range(5))
def test_snappy_executor_decodes_the_existing_encoder(seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, 3000, dtype=np.uint8)
    data = np.resize(np.concatenate([a, np.repeat(a[:40], 50), a[:1500]]), 9000 + 700 * seed).tobytes()
    z = B._snappy_compress(data, rng)
    assert B.execute("snappy", z) == (B.OK, data)
    t = B.model("snappy", z, seed, B.G_NARROW)
    assert not t.err and t.out == data


def test_executors_agree_on_shared_token_lists(co):
    for ops in B.shared_token_lists():
        want = B.ops_decode(ops)
        for fmt in B.FMTS:
            assert B.execute(fmt, B.ENC[fmt](ops).bytes()) == (B.OK, want), fmt
        n = len(want)
        for fmt in ("lz4", "blosclz"):  # and c-blosc agrees with the two it can decode
            fr = B.assemble([[B.S(B.ENC[fmt](ops).bytes(), n)]], comp=B.COMP[fmt], typesize=1, nbytes=n, blocksize=n)
            assert _oracle(co, fr.data, n) == want, fmt


def test_shuffles_invert_and_match_cblosc():
    rng = np.random.default_rng(2)
    for ts in (1, 2, 3, 4, 8, 16):
        for n in (ts * 64, ts * 64 + 3, ts * 61):
            a = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            for mode in (1, 2):
                assert B.unfiltered(B.filtered(a, ts, mode), ts, mode) == a
    a = np.repeat(rng.integers(0, 256, 64, dtype=np.uint8), 512).tobytes()
    for sh, mode in (("shuffle", 1), ("bitshuffle", 2)):  # c-blosc's own frame: its streams are the filtered block
        enc = O.OracleChain.from_metadata(
            [{"name": "bytes", "configuration": {"endian": "little"}},
             {"name": "blosc", "configuration": {"cname": "lz4", "clevel": 5, "shuffle": sh, "typesize": 4, "blocksize": 0}}],
            "uint8", 0, 1).encode(np.frombuffer(a, np.uint8))
        bs = int.from_bytes(enc[8:12], "little")
        assert not enc[2] & 2 and bs == len(a), "one compressed block"
        ns = 4 if B.cblosc_splits(not enc[2] & 0x10, 4, bs) else 1
        p, got = int.from_bytes(enc[16:20], "little"), b""
        for _ in range(ns):
            cs = int.from_bytes(enc[p:p + 4], "little")
            z = enc[p + 4:p + 4 + cs]
            got += z if cs == bs // ns else B.execute("lz4", z)[1]
            p += 4 + cs
        assert got == B.filtered(a, 4, mode), sh
