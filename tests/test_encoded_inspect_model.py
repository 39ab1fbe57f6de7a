"""The readers of tests/encoded_inspect.py are right (CPU only): what they report of a stream is what
the hand builders put into it (deflate_streams, zstd_frames, blosc_frames), and on zlib's and libzstd's
own output their tokens replay to the input. The GPU encoder tests' intents rest on them."""
import zlib

import numpy as np
import pytest

import blosc_frames as BF
import deflate_streams as D
import encoded_inspect as I
import zstd_frames as ZF


def _rand(seed, n, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, n, dtype=np.uint8).tobytes()


# ---- DEFLATE ---------------------------------------------------------------------------------------
def _builder_tokens(tokens):
    out = []
    for t in tokens:
        if isinstance(t, int):
            out.append(("L", t))
        else:
            out.append(("M", t[1], t[2], D.len_code(t[1], t[3] if len(t) > 3 else None)[0]))
    return out


def _deflate_block_lists():
    lits = list(_rand(1, 300))
    toks = lits + [("m", 3, 1), ("m", 258, 300), ("m", 258, 7, 284), ("m", 257, 2), ("m", 10, 303), 7, ("m", 4, 700)]
    long = list(_rand(2, 40000))
    far = long + [("m", 40, 32768), ("m", 3, 24577), ("m", 258, 1)]
    fl, fd = D.flat_lens(toks)
    ll138 = [6] * 10 + [7] * 20 + [0] * 138 + [7] * 87 + [0, 7]
    used = [s for s in range(255) if ll138[s]]
    ops138 = D.plain_ops(ll138[:30]) + [(18, 138)] + D.plain_ops(ll138[168:] + [0])
    return {
        "fixed": [D.Fixed(toks)],
        "dynamic_plain": [D.Dynamic(toks)],
        "dynamic_rle": [D.Dynamic(toks, rle=True)],
        "dynamic_hclen19": [D.Dynamic(toks, hclen=19, rle=True)],
        "dynamic_given_lens": [D.Dynamic(toks, ll=fl, dd=fd + [0, 0, 0], rle=True)],
        "stored_padded": [D.Fixed(lits[:5]), D.Stored(_rand(3, 1000), pad=0x55), D.Dynamic(toks[:200], rle=True)],
        "stored_empty_and_max": [D.Stored(b""), D.Stored(_rand(4, 65535)), D.Fixed([])],
        "window_and_run": [D.Dynamic(far, rle=True)],
        "run_18_of_138": [D.Dynamic([used[b % len(used)] for b in _rand(45, 300)], ll=ll138, dd=[0], ops=ops138,
                                    cl=D.spread(19, [0, 6, 7, 18], [2, 2, 2, 2]))],
        "no_distance_codes": [D.Dynamic(lits, dd=[0], rle=True)],
    }


@pytest.mark.parametrize("name", list(_deflate_block_lists()))
def test_deflate_tokens_returns_what_the_builder_wrote(name):
    blocks = _deflate_block_lists()[name]
    raw, starts = D.deflate(blocks)
    got, decoded, used = I.deflate_tokens(raw + b"trailer")
    assert used == len(raw) and decoded == D.execute(blocks) == I.replay_deflate(got)
    assert len(got) == len(blocks) and [g.final for g in got] == [0] * (len(blocks) - 1) + [1]
    for b, g, st in zip(blocks, got, starts):
        if isinstance(b, D.Stored):
            assert g.btype == 0 and g.data == b.data and g.data_bit == st and g.size == len(b.data)
            continue
        assert g.tokens == _builder_tokens(b.tokens), name
        assert g.size == len(D.execute([D.Stored(b"\0" * 40000), b])) - 40000
        if isinstance(b, D.Fixed):
            assert g.btype == 1 and g.hlit is None and g.clsyms == []
            continue
        fl, fd = D.flat_lens(b.tokens)
        ll, dd = b.ll if b.ll is not None else fl, b.dd if b.dd is not None else fd
        ops = b.ops if b.ops is not None else (D.rle_ops(list(ll) + list(dd)) if b.rle else D.plain_ops(list(ll) + list(dd)))
        assert g.btype == 2 and (g.hlit, g.hdist) == (len(ll), len(dd)) and g.ll == list(ll) and g.dd == list(dd)
        assert g.clsyms == [tuple(o) for o in ops], name
        if b.hclen is not None:
            assert g.hclen == b.hclen


@pytest.mark.parametrize("level", [0, 1, 9])
def test_deflate_tokens_replays_zlib_output(level):
    rng = np.random.default_rng(level)
    text = b" ".join(ZF.WORDS[i] for i in rng.integers(0, len(ZF.WORDS), 30000))
    data = text + _rand(5, 70000) + bytes(70000) + text[:50000]
    for wbits, reader in ((31, I.gzip_member), (15, I.zlib_stream)):
        c = zlib.compressobj(level, zlib.DEFLATED, wbits)
        enc = c.compress(data) + c.flush()
        blocks, decoded = reader(enc)
        assert decoded == data and I.replay_deflate(blocks) == data
        assert sum(b.size for b in blocks) == len(data)
        assert all(3 <= t[1] <= 258 and 1 <= t[2] <= 32768 for t in I.matches(blocks))
        if level == 0:
            assert {b.btype for b in blocks} == {0} and max(b.size for b in blocks) <= 65535
        else:
            assert any(t[1] == 258 and t[3] == 285 for t in I.matches(blocks))  # the zero run


def test_deflate_tokens_refuses_broken_streams():
    raw, _ = D.deflate([D.Dynamic(list(_rand(6, 500)) + [("m", 5, 9)], rle=True)])
    with pytest.raises(ValueError):
        I.deflate_tokens(raw[:len(raw) // 2])
    with pytest.raises(ValueError):
        I.deflate_tokens(D.deflate([D.Fixed([1, 2, ("m", 3, 5)])])[0])  # a distance before the start
    with pytest.raises(ValueError):
        I.deflate_tokens(D.deflate([D.Stored(b"abc", nlen_field=0)])[0])


# ---- zstd ------------------------------------------------------------------------------------------
def _planted(seed, n, copies):
    """Random bytes with a few planted repeats: raw literals and a handful of sequences per block."""
    rng = np.random.default_rng(seed)
    a = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    for k in range(copies):
        ln = int(rng.integers(8, 200))
        dst = int(rng.integers(n // 2, n - ln))
        src = int(rng.integers(0, dst - ln))
        a[dst:dst + ln] = a[src:src + ln]
    return bytes(a)


def test_zstd_blocks_replays_libzstd_frames():
    """libzstd level 1 frames, flushed in pieces (several blocks a frame): every block up to the first
    one the reader cannot follow (other table modes, Huffman literals) replays, with the frame's bytes
    before it as history, to libzstd's own decode of the block; predefined-mode blocks exist."""
    checked = 0
    for seed in range(12):
        data = _planted(seed, 6000 + 500 * seed, 1 + seed % 5)
        frame = ZF.stream_frame(data, 2500, level=1)
        assert ZF.zstd_decompress(frame, len(data)) == data
        blocks = I.zstd_blocks(frame, strict=False)
        walked = ZF.walk(frame)[0]
        pos, pairs = 0, []
        for b, (t, _, o, plen) in zip(blocks, walked):
            if b.size is None or (b.type == ZF.CMP and b.lits is None):
                break
            pairs.append((b, frame[o:o + plen] if b.type != ZF.CMP else None))
            got = I.replay_zstd(pairs, b"")
            assert got == data[:pos + b.size], (seed, pos)
            if b.type == ZF.CMP and b.nseq:
                assert b.modes == 0 and sum(s[0] for s in b.seqs) <= b.regen
                checked += 1
            pos += b.size
    assert checked >= 5, checked


def test_zstd_blocks_refuses_other_table_modes():
    data = (b"".join(ZF.WORDS[i % len(ZF.WORDS)] for i in np.random.default_rng(3).integers(0, 1000, 20000)))
    frame = ZF.stream_frame(data, 0, level=3)
    assert any(b.modes for b in I.zstd_blocks(frame, strict=False) if b.type == ZF.CMP)
    with pytest.raises(NotImplementedError, match="Symbol_Compression_Modes"):
        I.zstd_blocks(frame)


@pytest.mark.parametrize("family", list(ZF.FAMILIES))
def test_zstd_blocks_agrees_with_sections(family):
    """(literals type, regenerated size, sequence count) of every compressed block, on every frame of
    tests/zstd_frames.py (zstd_frames.sections reads them all); block types and sizes against
    zstd_frames.walk, and the Last_Block bit, which the reader takes from each block header, set on the
    last block alone."""
    n = 0
    for c in ZF.FAMILIES[family]():
        want = ZF.sections(c.enc)  # it reads every frame of the families
        frames = I.zstd_frames(c.enc, strict=False)
        got = [(b.ltype, b.regen, b.nseq) for f in frames for b in f.blocks if b.type == ZF.CMP]
        assert got == want, c.name
        for f, blks in zip(frames, ZF.walk(c.enc)):
            assert [b.type for b in f.blocks] == [t for t, _, _, _ in blks]
            assert [b.last for b in f.blocks] == [False] * (len(blks) - 1) + [True]
            assert all(b.size == s for b, (t, s, _, _) in zip(f.blocks, blks) if t != ZF.CMP)
            if all(b.size is not None for b in f.blocks) and f.content_size is not None:
                assert sum(b.size for b in f.blocks) == f.content_size
        n += 1
    assert n, family


def test_zstd_blocks_reads_hand_built_sequences_and_headers():
    """Predefined-mode sequences cannot come from zstd_frames.build (it writes RLE tables); the model
    of the GPU encoder's literal sections plus a predefined bitstream written here: every ll / ml /
    offset code, both sides of each range boundary."""
    import zstd_huf_model as M
    llt, oft, mlt = I.fse_dtable(I.LL_NORM, 6), I.fse_dtable(I.OF_NORM, 5), I.fse_dtable(I.ML_NORM, 6)
    for tab, norm in ((llt, I.LL_NORM), (oft, I.OF_NORM), (mlt, I.ML_NORM)):
        for s, c in enumerate(norm):
            assert sum(1 for e in tab if e[0] == s) == abs(c)

    def enc_state(tab, sym, nxt):
        """The state of `sym` whose range holds the next state (None: any state of sym)."""
        for u, (s, nb, base) in enumerate(tab):
            if s == sym and (nxt is None or base <= nxt < base + (1 << nb)):
                return u
        raise AssertionError((sym, nxt))

    seqs = [(ll, ml, ov) for ll, ml, ov in zip(
        [0, 15, 16, 23, 24, 31, 32, 47, 48, 63, 64, 127, 128, 300, 0, 1],
        [3, 34, 35, 42, 43, 50, 51, 66, 67, 98, 99, 130, 131, 258, 259, 70000],
        [4, 5, 6, 7, 8, 1 << 10, (1 << 11) - 1, 1 << 16, (1 << 20) + 5, 1, 2, 3, 4, 4, 4, 4])]
    w = M.BitW()
    sl = so = sm = None
    for i in range(len(seqs) - 1, -1, -1):
        ll, ml, ov = seqs[i]
        llc, mlc, ofc = ZF._code_of(ZF.LL_CODES, ll), ZF._code_of(ZF.ML_CODES, ml), ov.bit_length() - 1
        if sl is not None:  # the decoder updates LL, ML, OF in that order: written in reverse
            u = enc_state(oft, ofc, so)
            w.put(so - oft[u][2], oft[u][1])
            so = u
            u = enc_state(mlt, mlc, sm)
            w.put(sm - mlt[u][2], mlt[u][1])
            sm = u
            u = enc_state(llt, llc, sl)
            w.put(sl - llt[u][2], llt[u][1])
            sl = u
        else:
            sl, so, sm = enc_state(llt, llc, None), enc_state(oft, ofc, None), enc_state(mlt, mlc, None)
        w.put(ll - ZF.LL_CODES[llc][0], ZF.LL_CODES[llc][1])
        w.put(ml - ZF.ML_CODES[mlc][0], ZF.ML_CODES[mlc][1])
        w.put(ov - (1 << ofc), ofc)
    w.put(sm, 6)
    w.put(so, 5)
    w.put(sl, 6)
    body = w.close_backward()
    assert I._sequences(body, len(seqs)) == seqs
    with pytest.raises(ValueError):
        I._sequences(body + b"\x01", len(seqs))
    # literal section headers of the GPU encoder's model: type, Size_Format, sizes, streams, tree
    rng = np.random.default_rng(9)
    for n, sf, hdr, streams in ((1000, 0, 3, 1), (1024, 2, 4, 4), (16384, 3, 5, 4)):
        for kind, a in (("direct", rng.choice(4, n, p=[.55, .25, .12, .08]).astype(np.uint8)),
                        ("fse", (128 + rng.normal(0, 18, n)).clip(0, 255).astype(np.uint8))):
            frame = M.frame_of_literal_blocks(bytes(a), block=n)
            (b,) = I.zstd_blocks(frame)
            assert (b.ltype, b.sf, b.lhdr, b.regen, b.streams, b.nseq, b.size) == (2, sf, hdr, n, streams, 0, n)
            assert b.tree == kind and b.csize == ZF.walk(frame)[0][0][3] - hdr - 1, (n, kind)
            lens = M.huff_lengths(np.bincount(a, minlength=256).tolist(), M.HUF_MAX_BITS)
            assert b.max_bits == max(lens)
            o = ZF.walk(frame)[0][0][2]
            got = I.huf_lengths_of(frame[o + hdr:o + hdr + b.csize])
            assert got + [0] * (256 - len(got)) == lens, (n, kind)


# ---- blosc LZ streams and frames -------------------------------------------------------------------
def _lz_ops():
    r = BF.rnd
    return [("lit", r(14, 1)), ("match", 14, 8), ("lit", r(15, 2)), ("match", 3, 18), ("lit", r(16, 3)), ("match", 40, 19),
            ("lit", r(269, 4)), ("match", 300, 20), ("lit", r(270, 5)), ("match", 1, 273), ("lit", r(271, 6)),
            ("match", 7, 274), ("match", 8, 275), ("lit", r(9000, 7)), ("match", 8191, 9), ("match", 8192, 263),
            ("lit", r(33, 8)), ("match", 8193, 264), ("lit", r(64, 9)), ("match", 2047, 11), ("lit", r(65, 10)),
            ("match", 2048, 12), ("lit", r(60, 11)), ("match", 5, 64), ("lit", r(61, 12)), ("match", 6, 65),
            ("lit", r(256, 13)), ("match", 11000, 67), ("lit", r(257, 14)), ("match", 30, 68), ("lit", r(12, 15))]


@pytest.mark.parametrize("fmt", BF.FMTS)
def test_lz_tokens_returns_the_builders_ops(fmt):
    ops = _lz_ops()
    if fmt != "lz4":  # blosclz and snappy matches start at 3 / 1 bytes; lz4's at 4
        ops = ops + [("match", 100, 3), ("lit", BF.rnd(5, 16))]
    z = BF.ENC[fmt](ops).bytes()
    tok = I.lz_tokens(fmt, z)
    assert tok.decoded == BF.ops_decode(ops)
    want_m = [(o[2], o[1]) for o in ops if o[0] == "match"]
    assert [(m[0], m[1]) for m in I.merged_matches(tok)] == _merge(want_m, ops)
    lits = [len(o[1]) for o in ops if o[0] == "lit"]  # no two literal ops are adjacent: one run per op
    if fmt == "blosclz":  # runs of at most 32
        assert tok.lits == [k for n in lits for k in [32] * (n // 32) + ([n % 32] if n % 32 else [])]
        forms = {(m[1], m[2]): m[3] for m in tok.elements if m[0] == "match"}
        assert forms[(8, 14)] == ("near", 0) and forms[(9, 8191)] == ("near", 1) and forms[(263, 8192)] == ("far", 1)
        assert forms[(264, 8193)] == ("far", 2) and forms[(12, 2048)] == ("near", 1)
    elif fmt == "lz4":
        assert tok.lits == lits
        forms = {e[1]: e[2] for e in tok.elements if e[0] == "lit"}
        assert (forms[14], forms[15], forms[269], forms[270], forms[271]) == (0, 1, 1, 2, 2)
        forms = {e[1]: e[3] for e in tok.elements if e[0] == "match"}
        assert (forms[18], forms[19], forms[273], forms[274], forms[275]) == (0, 1, 1, 2, 2)
    else:
        assert tok.lits == lits and tok.preamble == (len(tok.decoded), 2)
        forms = {e[1]: e[2] for e in tok.elements if e[0] == "lit"}
        assert (forms[60], forms[61], forms[256], forms[257]) == (0, 1, 1, 2)
        assert {e[3] for e in tok.elements if e[0] == "match"} == {2}
        z1 = BF.SnW().preamble(21).literal(BF.rnd(10)).copy(5, 11, 1).bytes()
        assert I.lz_tokens("snappy", z1).elements[-1] == ("match", 11, 5, 1)


def _merge(pairs, ops):
    """The builder's matches with neighbours of one offset joined, as merged_matches joins pieces."""
    out, prev = [], False
    for o in ops:
        if o[0] == "lit":
            prev = False
            continue
        if prev and out[-1][1] == o[1]:
            out[-1] = (out[-1][0] + o[2], o[1])
        else:
            out.append((o[2], o[1]))
        prev = True
    return out


def test_lz_tokens_refuses_a_corrupt_stream():
    z = BF.enc_lz4(_lz_ops()).bytes()
    with pytest.raises(ValueError):
        I.lz_tokens("lz4", z[:-3])


@pytest.mark.parametrize("fmt", BF.FMTS)
def test_blosc_streams_returns_the_frames_streams(fmt):
    """grid_frame's layouts: split and unsplit blocks with a short last block, stored streams among
    compressed ones; a memcpyed frame."""
    kinds = set()
    for ts, split, bs, nbytes in ((4, True, 2048, 2048 * 3 + 600), (4, False, 2048, 2048 * 2), (1, True, 4096, 4096),
                                  (4, True, 256, 1024)):
        fr, chunk, k = BF.grid_frame(fmt, nbytes, bs, ts, split, stored=lambda i: i % 3 == 1, seed=5)
        frame = fr.data
        f = I.blosc_streams(frame)
        assert (f.typesize, f.nbytes, f.blocksize, f.cbytes, f.memcpyed, f.comp) == (ts, nbytes, bs, len(frame), False, fmt)
        assert len(f.streams) == k == BF.count_streams(frame)
        dec = {}
        for i, s in enumerate(f.streams):
            assert s.stored == (len(s.payload) == s.size) and s.csize == len(s.payload)
            d = s.payload if s.stored else I.lz_tokens(fmt, s.payload).decoded
            assert len(d) == s.size
            dec[s.block] = dec.get(s.block, b"") + d
        kinds |= {(ts, s.stored) for s in f.streams}
        assert b"".join(BF.unfiltered(dec[b], ts, 0) for b in sorted(dec)) == chunk
    assert {(4, True), (4, False)} <= kinds
    data = BF.rnd(500)
    m = I.blosc_streams(BF.header(flags=0x02 | 0x01, typesize=4, nbytes=500, blocksize=500, cbytes=516) + data)
    assert m.memcpyed and m.streams == []
    with pytest.raises(ValueError):
        I.blosc_streams(BF.header(flags=0x02, typesize=4, nbytes=500, blocksize=500, cbytes=515) + data)


# ---- the encoder inputs' name list -------------------------------------------------------------------
def test_encoder_input_names_and_sizes():
    """tests/test_gpu_encoder_edges.py parametrises over encoder_inputs.NAMES without building the
    inputs: the list is the cases' names (all_cases() asserts it), no name twice; every input stays
    within about 1.2 MiB and every codec is one the write path has."""
    import encoder_inputs as E
    cases = E.all_cases()
    assert len(set(E.NAMES)) == len(E.NAMES) == len(cases)
    assert max(len(c.data) for c in cases) <= 1200 * 1024 + 4096
    assert {c.codec for c in cases} <= {"gzip", "zlib", "zstd", "zstd_ck", "blosc-lz4", "blosc-lz4hc", "blosc-blosclz",
                                        "blosc-snappy", "blosc-zlib", "blosc-zstd"}
    assert all(c.intent for c in cases)
