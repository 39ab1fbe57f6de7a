"""CPU check of the hand-built DEFLATE streams (tests/deflate_streams.py) that test_gpu_deflate_streams.py
feeds k_gzip: every valid case decodes to its `expect` under zlib (the gzip and the zlib wrapper) and
under the CPU model of the segmented decode with the kernel's constants (tools/gzip_seg_model.py);
every corrupt case is refused by zlib (build_table's rule: an invalid stream is what zlib's inflate
refuses); a size case decodes under zlib to a length other than its chunk's; and every case reaches,
in the model, the state it is there for - controls next to an edge do not. The executor-ring cases
state theirs twice: under BATCH_CAP = RING / 2 they reach the ring-edge states (or, the controls, just
miss them); under the kernel's constants no stream does, which is checked for every case."""
import zlib

import pytest

import deflate_streams as D

M = D.M
_ALL = [(f, c.name) for f in D.FAMILIES for c in D.family(f)]


def _case(fam, name):
    return next(c for c in D.family(fam) if c.name == name)


@pytest.mark.parametrize("fam,name", _ALL, ids=[n for _, n in _ALL])
def test_case_agrees_with_zlib_and_its_intent(fam, name):
    c = _case(fam, name)
    gz, zl = c.enc("gz"), c.enc("zlib")
    if c.status == D.CORRUPT:
        with pytest.raises(zlib.error):
            zlib.decompress(gz, 31)
        with pytest.raises(zlib.error):
            zlib.decompress(zl, 15)
        assert not c.intent
        return
    want = c.expect if c.status == D.OK else c.decoded
    assert zlib.decompress(gz, 31) == want
    assert zlib.decompress(zl, 15) == want
    if c.status == D.SIZE:
        assert len(want) != c.size
        return
    assert len(want) == c.size and c.size in D.SIZES
    st = {}
    assert M.inflate_stream(gz, 10, 8, stats=st, **M.KERNEL) == want
    for text, pred in c.intent + D.SAFE:
        assert pred(st), f"{name}: the model does not show: {text}"
    if c.intent_ring_half:
        st = {}
        assert M.inflate_stream(gz, 10, 8, stats=st, batch_cap=M.BATCH_CAP_RING_HALF, **M.KERNEL) == want
        for text, pred in c.intent_ring_half:
            assert pred(st), f"{name}: the model with BATCH_CAP = RING / 2 does not show: {text}"


def test_families_cover_the_issue():
    """The sweeps hold both sides of each edge: cases in the state and controls beside it."""
    ring = D.family("executor_ring")
    hits = [c for c in ring if any(p is D.short_unflushed for _, p in c.intent_ring_half)]
    ctrl = [c for c in ring if c.name.startswith("ring_D") and c not in hits]
    assert len(hits) >= 16 and len(ctrl) >= 16
    assert {c.name for c in hits} >= {f"ring_D{d}" for d in range(747, 763)}
    for f in D.FAMILIES:
        cs = D.family(f)
        assert any(c.status == D.OK for c in cs)
        assert all(len(c.expect) == c.size for c in cs if c.status == D.OK)


def test_table_shape_and_header_windows():
    """The model's table facts against sets whose shape is known by hand."""
    assert M.table_shape(D.FIXED_LL, 9) == (9, 0)
    assert M.table_shape(D.SKEW16, 9) == (15, 64)      # one root prefix holds the codes of 10..15 bits
    assert M.table_shape(D.SKEW16, 8) == (15, 128)
    assert M.table_shape([1], 8) == (1, 0) and M.table_shape([0], 8) == (0, 0)
    # 40 two-bit symbols: 32 start in the first window's 63 bits, all 32 are taken; the rest follow
    w = M.header_windows([(8, 2, 1)] * 40, 40)
    assert [len(x["take"]) for x in w] == [32, 8] and w[0]["starts"] == 32
    # one-bit symbols: 63 starts, 32 taken
    w = M.header_windows([(8, 1, 1)] * 100, 100)
    assert w[0]["starts"] == 63 and len(w[0]["take"]) == 32


def test_executor_accounting():
    """ExecAcct on a hand-checked sequence: 64 literals make one batch; pending bytes flush at 256."""
    a = M.ExecAcct()
    a.stored(100)
    a.round([65] * 64 + [(1 << 31) | (50 << 9) | 258] * 3)
    b = a.batches
    assert [(x["B"], x["f"], x["syms"]) for x in b] == [(64, 0, 64), (516, 64, 2), (258, 0, 1)]
    assert M.RING == 1024 and M.FLUSH_MIN - 1 + M.BATCH_CAP - 1 + 258 <= M.RING - 31  # the kernel's static_assert
    assert a.pos == 100 + 64 + 774 and a.flushed == a.pos
    m = b[1]["matches"][0]
    assert m["src"] == 164 - 50 and m["start_in_ring"] and not m["last_flushed"]
