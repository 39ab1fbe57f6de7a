"""The hand-built bzip2 streams of bz2_streams.py, held to libbz2 (Python's bz2 module, the library
zarr-python wrote the reference fixtures with and the family zarrs' bzip2 crate wraps) and to their own
intent. No GPU: this pins the test vectors that test_gpu_bz2.py feeds the kernels.

A stream is valid if and only if bz2.BZ2Decompressor reaches eof without raising; unused_data is the
trailing part that is ignored."""
import bz2

import pytest

import bz2_streams as S

FAMILIES = S.families()
CASES = [(f, c) for f, cases in FAMILIES.items() for c in cases]


def libbz2(stream: bytes):
    """(valid, decoded bytes, unused bytes) as bz2.BZ2Decompressor sees the stream."""
    d = bz2.BZ2Decompressor()
    try:
        out = d.decompress(stream)
    except (OSError, ValueError, EOFError):
        return False, b"", b""
    return d.eof, out, d.unused_data


@pytest.mark.parametrize("family,case", CASES, ids=[f"{f}-{c.name}" for f, c in CASES])
def test_case_against_libbz2(family, case):
    ok, out, _ = libbz2(case.stream)
    if case.status == S.OK:
        assert ok and out == case.expect
    else:
        assert not ok


@pytest.mark.parametrize("family,case", CASES, ids=[f"{f}-{c.name}" for f, c in CASES])
def test_case_reaches_its_edge(family, case):
    for text, pred in case.intent:
        assert pred(case.trace), text
    for text, pred in case.miss:
        assert not pred(case.trace), text


def test_no_case_is_without_an_intent():
    """Every case proves its edge from the assembler's own trace, and every family with edges that a
    plain block could reach by accident has a control that misses them."""
    for f, c in CASES:
        assert c.intent or c.miss, (f, c.name)
    for f in ("tables", "groups", "runs", "mtf", "bwt", "rle1", "magic"):
        assert any(c.miss for c in FAMILIES[f]), f
    assert bz2.decompress(S.stream([S.block_of(S._text(900, 17), 3)])) == S._text(900, 17)  # the corrupt family's base


def test_every_family_of_the_issue_is_there():
    names = {c.name for _, c in CASES}
    assert set(FAMILIES) == {"tables", "groups", "runs", "mtf", "bwt", "rle1", "magic", "corrupt"}
    for n in ("ngroups2", "ngroups6_selector_change_every_group", "selector_mtf_maximum", "code_1bit_and_20bit",
              "all_258_symbols", "one_byte_value_alphabet3", "length_deltas_1_20_1", "block_of_50_symbols",
              "block_of_51_symbols", "block_of_100_symbols", "run_65536", "run_to_the_block_limit",
              "run_past_the_block_limit", "mtf_index_255", "origptr_0", "origptr_last", "one_symbol",
              "all_equal_stable_sort", "four_equal_count_0", "count_equals_the_run_byte", "stretch_mod5_4",
              "run_cut_by_the_block_end", "run_crossing_two_blocks", "long_input_without_sync_point",
              "every_position_a_sync_point", "block_magic_inside_the_payload", "second_stream_ignored",
              "bad_block_crc", "bad_combined_crc", "randomised_bit", "empty_input"):
        assert n in names, n


def test_trailing_bytes_are_unused_data():
    by = {c.name: c for _, c in CASES}
    ok, _, unused = libbz2(by["second_stream_ignored"].stream)
    assert ok and unused.startswith(b"BZh9")
    ok, _, unused = libbz2(by["block_magic_in_trailing_junk"].stream)
    assert ok and unused.endswith(b"tail")


def test_transforms_against_libbz2():
    """The naive RLE1 / BWT / MTF and the assembler write what libbz2 reads back; the CRC is libbz2's."""
    for data in (b"", b"a", b"banana" * 40, bytes(300), bytes(range(256)) * 3, S._text(2000, 4)):
        blocks = [S.block_of(data)] if data else []
        s = S.stream(blocks, 5)
        assert bz2.decompress(s) == data
        if data:
            assert S.execute(blocks, 5)[0] == data
    real = bz2.compress(b"hello, bzip2", 9)
    assert int.from_bytes(real[10:14], "big") == S.crc(b"hello, bzip2")  # byte-aligned first block: its CRC


def test_open_run_at_a_block_end_is_a_libbz2_error():
    """Four equal bytes that end a block without their count byte: libbz2 reads the count past the block
    and reports a data error, so the decoder must too (the control with a count byte decodes)."""
    c = S.crc(b"abcdddd")
    bad = S.stream([S.raw_block(b"abc" + b"dddd", crc=c)], combined=S.combine([c]))
    assert not libbz2(bad)[0]
    good = S.stream([S.raw_block(b"abc" + b"dddd\x00")])
    assert libbz2(good)[:2] == (True, b"abcdddd")
