"""The frames of tests/zstd_frames.py against libzstd on the CPU: ZSTD_decompress of every frame the
GPU tests decode returns exactly the reference executor's bytes (hand-built frames) or the original
data (streaming frames), and every case has the shape it is meant to have (block counts and types,
sequence counts). This keeps the builder right independently of the decoder under test."""
import numpy as np
import pytest

import zstd_frames as Z


@pytest.mark.parametrize("family", list(Z.FAMILIES))
def test_libzstd_decodes_every_case_to_its_expected_bytes(family):
    cases = Z.FAMILIES[family]()
    assert cases and len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert len(c.expect) <= 256 << 10 or len(c.expect) == 1 << 20, c.name
        assert Z.zstd_decompress(c.enc, len(c.expect)) == c.expect, c.name
        if c.specs is not None:
            assert Z.execute(c.specs) == c.expect, c.name
            if len(c.specs) > 1 and b"skipped" not in c.enc:  # frame by frame as well
                assert b"".join(Z.zstd_decompress(Z.build(f), len(c.expect)) for f in c.specs) == c.expect, c.name


@pytest.mark.parametrize("family", list(Z.FAMILIES))
def test_every_case_has_its_shape(family):
    for c in Z.FAMILIES[family]():
        assert c.check is not None, c.name
        c.check(c)
        c.check_path()


def test_executor_repeat_offsets_by_hand():
    """RFC 8878 3.1.1.5 on frames small enough to follow by hand (the history starts as 1, 4, 8)."""
    lits = bytes(range(10, 22))
    # ll > 0, value 2: the second entry, 4; history (4, 1, 8). Then ll == 0, value 1: the second entry
    # again, 1; history (1, 4, 8)
    fr = Z.Frame([Z.cmp_block(lits, [(12, 3, 2)]), Z.cmp_block(b"", [(0, 3, 1)])])
    out = bytearray(lits)
    out += out[-4:-1]
    out += bytes([out[-1]]) * 3
    assert Z.execute([fr]) == bytes(out) == Z.zstd_decompress(Z.build(fr), 64)
    # ll == 0, value 3 with history (4, 1, 8): the first entry less one, 3
    fr2 = Z.Frame([Z.cmp_block(lits, [(12, 3, 2)]), Z.cmp_block(b"", [(0, 4, 3)])])
    out2 = bytearray(lits)
    out2 += out2[-4:-1]
    for _ in range(4):
        out2.append(out2[-3])
    assert Z.execute([fr2]) == bytes(out2) == Z.zstd_decompress(Z.build(fr2), 64)


def test_streaming_shapes_named_in_the_builder():
    """windowLog 10 gives 1 KiB blocks (64 for 64 KiB of 4-symbol noise); ending a fully flushed frame
    appends an empty raw last block; an unpledged frame has no content size but a window descriptor."""
    noise = np.random.default_rng(4).integers(0, 4, 65536, dtype=np.uint8).tobytes()
    assert len(Z.blocks(Z.stream_frame(noise, 0, window_log=10))) == 64
    f = Z.stream_frame(b"abc" * 100, 100, end_empty=True)
    assert Z.blocks(f)[-1] == (Z.RAW, 0) and Z.zstd_decompress(f, 300) == b"abc" * 100
    assert Z.stream_frame(b"x" * 1000, 100, pledged=False)[4] >> 5 == 0  # no FCS field, not single-segment
    assert Z.stream_frame(b"x" * 1000, 100, pledged=True)[4] & 0x20


def test_libzstd_decodes_no_frame_to_nothing():
    """no bytes, and skippable frames alone: 0 bytes and no error (what the GPU decoder must hand on)"""
    assert Z.zstd_decompress(b"", 16) == b""
    assert Z.zstd_decompress(Z.skippable(), 16) == b""
    assert Z.zstd_decompress(Z.skippable() + Z.skippable(b"", 7), 16) == b""
