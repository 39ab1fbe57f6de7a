"""GPU zstd decode of frames libzstd's one-shot encoder never makes (tests/zstd_frames.py: streaming
frames flushed into many tiny blocks, and hand-assembled frames at the decoder's capacities, table
sizes, window spans and repeat-offset rules), bit-exact against libzstd / the reference executor
(tests/test_zstd_frames_model.py ties those two together on the CPU), on every executor path, with
the path taken asserted from the call's device counters."""
import numpy as np
import pytest

import zstd_frames as Z

pytestmark = pytest.mark.gpu

BYTES_LE = {"name": "bytes", "configuration": {"endian": "little"}}
ZSTD_VARS = ["ZGPU_ZSTD_XWIN", "ZGPU_ZSTD_XPAR", "ZGPU_ZSTD_XDENSE", "ZGPU_ZSTD_FORCE_SERIAL"]
PATHS = {
    "latency": {"ZGPU_ZSTD_XWIN": "1", "ZGPU_ZSTD_XPAR": "1"},
    "window": {"ZGPU_ZSTD_XWIN": "1", "ZGPU_ZSTD_XPAR": "0"},
    "wave": {"ZGPU_ZSTD_XWIN": "0", "ZGPU_ZSTD_XDENSE": "0"},
    "wave_dense": {"ZGPU_ZSTD_XWIN": "0", "ZGPU_ZSTD_XDENSE": "1"},
    "serial": {"ZGPU_ZSTD_FORCE_SERIAL": "1"},  # read when the call's plan is made
}


def _codecs(checksum):
    return [BYTES_LE, {"name": "zstd", "configuration": {"level": 3, "checksum": checksum}}]


def _decode(cases, checksum, env, monkeypatch):
    """One decode_batch call over `cases` (all of one chunk size) with the ZGPU_ZSTD_* variables of
    `env` (every other one unset): (statuses, decoded rows, the call's counters)."""
    import torch
    from zarrs_amd import CodecChain, Context, make_desc
    from zarrs_amd import _lib as L
    n = len(cases[0].expect)
    assert all(len(c.expect) == n for c in cases)
    for v in ZSTD_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev = torch.frombuffer(bytearray(b"".join(c.enc for c in cases)), dtype=torch.uint8).cuda()
    descs, off = [], 0
    for i, c in enumerate(cases):
        descs.append(make_desc((dev.data_ptr() + off, len(c.enc)), [n], out_start=[i * n]))
        off += len(c.enc)  # unaligned frame starts on purpose
    ch = CodecChain.from_metadata(_codecs(checksum), "uint8", 0, Context.default())
    out = torch.zeros(len(cases) * n, dtype=torch.uint8, device="cuda")
    try:
        st = ch.decode_batch(descs, out, [len(cases) * n], enc_device=True)
    except Exception as e:  # noqa: BLE001  (a non-zero status raises: report it with the case names below)
        st = [getattr(e, "status", -1), str(e)]
    return st, out.cpu().numpy().reshape(len(cases), n), L.last_counters()


def _where(c, got):
    """First wrong byte of a case, and the block it lies in when the case is one frame."""
    exp = np.frombuffer(c.expect, np.uint8)
    bad = np.flatnonzero(got != exp)
    if not len(bad):
        return None
    p, pos, blk = int(bad[0]), 0, None
    if c.specs is not None and len(c.specs) == 1:
        for i, b in enumerate(c.specs[0].blocks):
            pos += (len(b.data) if b.kind == Z.RAW else b.n if b.kind == Z.RLE
                    else len(b.literals()) + sum(s[1] for s in b.seqs))
            if p < pos:
                blk = f"block {i} of {len(c.specs[0].blocks)}"
                break
    return f"{c.name}: {len(bad)} wrong bytes, the first at {p} of {len(exp)}" + (f", in {blk}" if blk else "")


def _groups(cases):
    """The cases by (chunk size, checksummed): one call each."""
    g = {}
    for c in cases:
        g.setdefault((len(c.expect), c.checksummed), []).append(c)
    return sorted(g.items())


def _run_family(family, path, monkeypatch):
    problems = []
    for (n, ck), cases in _groups(Z.FAMILIES[family]()):
        st, got, ctr = _decode(cases, ck, PATHS[path], monkeypatch)
        tag = f"{family}/{path}/{n}{'/ck' if ck else ''}"
        print(tag, "statuses", st, "counters", ctr)
        if st != [0] * len(cases):
            problems.append(f"{tag}: statuses {st}")
        for i, c in enumerate(cases):
            w = _where(c, got[i])
            if w:
                problems.append(f"{tag}: {w}")
        k, must = len(cases), sum(c.parallel is True for c in cases)
        ser, par, lat = ctr["zstd_serial"], ctr["zstd_parallel"], ctr["zstd_latency"]
        if path == "serial":
            ok = ser == k and par == 0 and lat == 0
        else:  # cases that may take either decoder (parallel None) count on one side or the other
            ok = ser + par == k and must <= par <= k and lat == (par if path == "latency" else 0)
        if not ok:
            problems.append(f"{tag}: counters {ctr} for {k} items ({must} meant for the parallel pipeline)")
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("family", list(Z.FAMILIES))
def test_family_on_every_path(family, path, monkeypatch):
    _run_family(family, path, monkeypatch)


@pytest.mark.parametrize("chunk,k", [(4096, 63), (8192, 63), (4096, 17), (8192, 33)])
def test_lone_chain_takes_the_latency_mode_by_default(chunk, k, monkeypatch):
    """A lone frame with no ZGPU_ZSTD_* variable set (a per-chunk call through a codec plugin) takes the
    latency mode, and a chain k blocks deep decodes exactly there. Four depths of the exact-depth family:
    the deepest chain (63) at 4 KiB and 8 KiB, and the first depth past what the earlier round rule was
    read to cover at each size (17 and 33); test_family_on_every_path runs every depth on the forced
    latency path."""
    c = [c for c in Z.family_chains_exact() if c.name == f"depth_{chunk}_k{k}"]
    assert len(c) == 1
    st, got, ctr = _decode(c, False, {}, monkeypatch)
    print(c[0].name, "status", st, "counters", ctr)
    assert st == [0]
    assert _where(c[0], got[0]) is None, _where(c[0], got[0])
    assert ctr["zstd_latency"] == 1 and ctr["zstd_parallel"] == 1 and ctr["zstd_serial"] == 0, ctr


def test_default_executor_changes_where_the_batch_fills_the_device(monkeypatch):
    """With no ZGPU_ZSTD_* variable set, the latency mode takes a batch while n_items * 3 < 4 * CUs
    (the launch policy's table) and no batch past that: lo = (4 * CUs - 1) // 3 frames of one
    4 KiB chain all finish there, lo + 1 frames all finish in the block-parallel pipeline without it (341
    and 342 on 256 CUs)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lo = (4 * cus - 1) // 3
    c = [c for c in Z.family_chains_exact() if c.name == "depth_4096_k17"]
    assert len(c) == 1 and c[0].parallel is True
    for n, lat in ((lo, lo), (lo + 1, 0)):
        st, got, ctr = _decode(c * n, False, {}, monkeypatch)
        print(cus, "CUs,", n, "frames: counters", ctr)
        assert st == [0] * n
        assert (got == np.frombuffer(c[0].expect, np.uint8)).all()
        assert ctr["zstd_latency"] == lat and ctr["zstd_parallel"] == n and ctr["zstd_serial"] == 0, ctr


@pytest.mark.parametrize("path", list(PATHS))
def test_skippable_frames_alone_decode_to_nothing(path, monkeypatch):
    """An input of skippable frames only holds no data: ZSTD_decompress returns 0 bytes and no error
    (test_zstd_frames_model.py), so zarrs' zstd codec hands `bytes` nothing (zstd_codec.rs:119-123) and the
    chunk fails with the size error, not as a corrupt stream. In front of a frame they are passed over."""
    from types import SimpleNamespace
    from zarrs_amd import _lib as L
    for enc in (Z.skippable(), Z.skippable() + Z.skippable(b"", 7)):
        st, _, _ = _decode([SimpleNamespace(enc=enc, expect=bytes(16))], False, PATHS[path], monkeypatch)
        assert st[0] == L.DECODED_SIZE_MISMATCH, st
    data = bytes(range(16))
    st, got, _ = _decode([SimpleNamespace(enc=Z.skippable() + Z.stream_frame(data, 0), expect=data)], False, PATHS[path],
                         monkeypatch)
    assert st == [0] and got[0].tobytes() == data
