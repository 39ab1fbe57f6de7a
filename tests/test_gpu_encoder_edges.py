"""The GPU encoders at their formats' limits: every input of tests/encoder_inputs.py (built to reach
one edge of k_gzip_encode, k_zstd_encode_seg / k_zstd_frame or k_lz4_encode<FMT> and the blosc framing)
is encoded through the public write path (CodecChain.encode_chunks over [bytes, <codec>], uint8), and
the encoded chunk
  1. decodes to the input with a decoder that is not this project's: zlib (gzip members, RFC 1950
     streams), libzstd, c-blosc through the oracle chain, and for snappy and blosclz streams the
     reference executors of tests/blosc_frames.py;
  2. is no longer than the chain's encoded_bound;
  3. shows, to tests/encoded_inspect.py, the edge the input exists for (the case's intent);
  4. is read back by the GPU decoder to the input.
Cases of one codec configuration and one length share an encode_chunks call.

The batch of unequal zstd items (z5_blosc_zstd_unequal_streams) reaches launch_zstd_encode through
blosc-zstd with a block size of 1 MiB + 4 KiB over 1 MiB + 70 KiB: two streams of one launch, the short
one leaving its second (item, segment) unit idle."""
import json
import zlib

import numpy as np
import pytest

import blosc_frames as BF
import encoded_inspect as I
import encoder_inputs as E
import oracle as O
import zstd_frames as ZF

pytestmark = pytest.mark.gpu

BYTES = {"name": "bytes", "configuration": {"endian": "little"}}


def _key(c):
    return json.dumps(E.codec_metadata(c), sort_keys=True), len(c.data)


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def cases():
    """The inputs, built when the first test runs (collection only reads encoder_inputs.NAMES)."""
    return {c.name: c for c in E.all_cases()}


@pytest.fixture(scope="module")
def encoded(ctx, cases):
    """name -> (chain, encoded device tensor): the cases of one codec configuration and length are
    encoded by one encode_chunks call, when the first of them is asked for."""
    import torch
    from zarrs_amd import CodecChain
    groups, done = {}, {}
    for c in cases.values():
        groups.setdefault(_key(c), []).append(c)

    def get(name):
        if name not in done:
            cs = groups[_key(cases[name])]
            n = len(cs[0].data)
            ch = CodecChain.from_metadata([BYTES, E.codec_metadata(cs[0])], "uint8", 0, ctx)
            x = torch.from_numpy(np.frombuffer(b"".join(c.data for c in cs), np.uint8).copy()).cuda()
            enc = ch.encode_chunks(x, [n], [[i * n] for i in range(len(cs))])
            for c, e in zip(cs, enc):
                done[c.name] = (ch, e)
        return done[name]
    return get


def _blosc_lz_decode(case, enc):
    """A c-blosc 1.x frame of lz4 / blosclz / snappy streams decoded by the reference executors."""
    f = I.blosc_streams(enc)
    if f.memcpyed:
        return enc[16:]
    fmt = {"lz4hc": "lz4"}.get(f.comp, f.comp)
    blocks = {}
    for s in f.streams:
        d = s.payload if s.stored else BF.execute(fmt, s.payload, s.size)
        assert s.stored or (d[0] == BF.OK and len(d[1]) == s.size), (case.name, s.block, d[0])
        blocks[s.block] = blocks.get(s.block, b"") + (d if s.stored else d[1])
    mode = 1 if f.flags & 1 else 2 if f.flags & 4 else 0
    return b"".join(BF.unfiltered(blocks[b], f.typesize, mode) for b in sorted(blocks))


def _independent_decode(case, enc):
    n = len(case.data)
    if case.codec == "gzip":
        return zlib.decompress(enc, 31)
    if case.codec == "zlib":
        return zlib.decompress(enc, 15)
    if case.codec.startswith("zstd"):
        return ZF.zstd_decompress(enc, n)
    kind = case.codec.split("-", 1)[1]
    if kind in ("snappy", "blosclz"):
        got = _blosc_lz_decode(case, enc)
        if kind == "snappy":  # the oracle's c-blosc is built without snappy
            return got
        assert got == case.data, (case.name, "blosc_frames executor")
    co = O.OracleChain.from_metadata([BYTES, E.codec_metadata(case)], "uint8", 0, 1)
    return co.decode(enc, [n]).tobytes()


def _show(case, v):
    """What the failure message prints of the view: the tokens or headers the intents look at."""
    if isinstance(v, E.DeflateView):
        return {"blocks": [(b.btype, b.size, b.bitpos, b.hlit, b.hdist, b.hclen) for b in v.blocks],
                "matches": v.matches[:40], "clsyms": [b.clsyms for b in v.blocks][:2]}
    if isinstance(v, E.ZstdView):
        return {"frame": (v.frame.fcs_bytes, v.frame.content_size, v.frame.checksum),
                "blocks": [(b.type, b.size, b.ltype, b.sf, b.lhdr, b.regen, b.csize, b.streams, b.tree, b.max_bits, b.nseq)
                           for b in v.blocks][:20],
                "sequences": [s for s in v.seqs if s[2] < 60000][:40]}
    f = v.frame
    return {"frame": (f.flags, f.typesize, f.nbytes, f.blocksize, f.cbytes, f.memcpyed),
            "streams": [(s.block, s.csize, s.stored, s.size) for s in f.streams], "matches": v.matches[:40],
            "elements": [t.elements[:40] for t in v.streams if isinstance(t, I.LzTokens)][:2]}


@pytest.mark.parametrize("name", E.NAMES)
def test_encoder_edge(cases, encoded, name):
    import torch
    from zarrs_amd import make_desc
    case = cases[name]
    ch, e = encoded(name)
    n = len(case.data)
    enc = e.cpu().numpy().tobytes()
    # 1. an independent decoder reads it
    assert _independent_decode(case, enc) == case.data, name
    # 2. within the chain's bound
    assert len(enc) <= ch.encoded_bound([n]), (name, len(enc), ch.encoded_bound([n]))
    if name.startswith("g5_zlib"):
        assert len(enc) <= n + (n >> 12) + (n >> 14) + (n >> 25) + 13, (name, len(enc))
    # 3. the edge the case exists for
    v = E.view(case, enc)
    for text, pred in case.intent:
        assert pred(v), "%s: %s\n%s" % (name, text, _show(case, v))
    # 4. the GPU decoder reads it back
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert ch.decode_batch([make_desc((e.data_ptr(), e.numel()), [n])], out, [n], enc_device=True) == [0]
    assert out.cpu().numpy().tobytes() == case.data, name


def test_no_frame_of_the_suite_uses_a_repeat_offset(cases, encoded):
    """Offsets 1, 2 and 3 are written as Offset_Value 4, 5 and 6: no zstd frame here holds a value
    below 4, the streams of the blosc-zstd frame included (every case asserts it for itself; this is the
    count: the two sequence-count cases alone hold 127 + 128)."""
    total = 0
    for name, c in cases.items():
        if not c.codec.endswith("zstd") and not c.codec.startswith("zstd"):
            continue
        v = E.view(c, encoded(name)[1].cpu().numpy().tobytes())
        views = [v] if c.codec.startswith("zstd") else [s for s in v.streams if s is not None]  # blosc-zstd: its streams
        for zv in views:
            assert all(s[3] >= 1 for s in zv.seqs), name
            total += len(zv.seqs)
    assert total >= 255, total
