"""cast_one / cast_mapped / cast_infallible of zarrs_amd/csrc/kernels/cast.hpp on the CPU, against the exact
model (tests/cast_value_model.py): a stand-alone program (tests/c/cast_value_harness.cpp) that includes
that header alone, built with the undefined-behaviour and float-cast-overflow sanitizers (an unchecked
float -> integer conversion, a shift past the width or a signed overflow ends the program), runs every
(source, target) pair x rounding mode x out_of_range on the edge list of the source type, on the part of
it the model casts without error, and on 64 xorshift64 elements. One process per source type."""
import os
import subprocess

import pytest

import cast_value_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cast") / "cast_value_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "c", "cast_value_harness.cpp")])
    return exe


def run(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def line(s, t, r, oor, elems, smap=()):
    maps = " ".join(f"{M.to_bytes([k], s).hex()}={M.to_bytes([v], t).hex()}" for k, v in smap)
    return f"cast {s} {t} {r} {oor or 'none'} {M.to_bytes(elems, s).hex() or '-'} {maps}".rstrip()


def expect(s, t, r, oor, elems, smap=()):
    out, bad = M.cast_list(elems, s, t, r, oor, smap)
    return f"ERR {bad}" if bad is not None else ("OK " + M.to_bytes(out, t).hex()).rstrip() + ("" if out else "")


def modes(t):
    return [None, "clamp"] + ([] if M.is_float(t) else ["wrap"])


@pytest.mark.parametrize("s", M.TYPES)
def test_every_pair_matches_the_model(harness, s):
    edges, rnd = M.edge_elements(s), M.xorshift_elements(s)
    lines, want, what = [], [], []
    for t in M.TYPES:
        for r in M.ROUNDINGS:
            for oor in modes(t):
                clean = M.error_free(edges, s, t, r, oor)
                assert len(clean) >= 4, (s, t, r, oor)  # 0, 1, 2 and 3 at the least: not "both fail" alone
                for elems in (edges, clean, rnd):
                    lines.append(line(s, t, r, oor, elems))
                    want.append(expect(s, t, r, oor, elems))
                    what.append((s, t, r, oor, len(elems)))
                assert want[-2].startswith("OK ")
    got = run(harness, lines)
    bad = [(w, g, x) for w, g, x in zip(what, got, want) if g != x]
    assert not bad, f"{len(bad)} of {len(lines)} cases differ; first: {bad[0]}"


def test_wrap_into_a_float_target_is_the_decode_rule(harness):
    """out_of_range = wrap with a float target is refused at binding, but decode runs it (an integer-encoded
    float array): the overflow goes to the bound or to infinity by the rounding mode"""
    lines, want = [], []
    for s in M.TYPES:
        for t in M.FLOATS:
            for r in M.ROUNDINGS:
                e = M.edge_elements(s)
                lines.append(line(s, t, r, "wrap", e))
                want.append(expect(s, t, r, "wrap", e))
    assert run(harness, lines) == want


def test_scalar_map_comes_first_and_never_fails(harness):
    nan, inf = M.canonical_nan("float32"), M.inf_bits("float32", False)
    one = M.scalar_bits(1.0, "float32")
    smap = [(nan, 0), (one, 2), (one, 3), (inf, 255), (M.scalar_bits(-0.0, "float32"), 9)]
    elems = [M.scalar_bits(0.0, "float32"), M.scalar_bits(-0.0, "float32"), one, nan, inf, M.scalar_bits(7.0, "float32")]
    lines = [line("float32", "uint8", "nearest-even", None, elems, smap),
             line("float32", "uint8", "nearest-even", None, elems + [nan | 1], smap),  # another NaN: no key
             line("uint8", "float32", "nearest-even", None, [0, 1, 255], [(0, nan), (255, 0x12345678)])]
    got = run(harness, lines)
    assert got[0] == "OK 000902" + "00ff07"
    assert got[1] == "ERR 6"
    assert got == [expect("float32", "uint8", "nearest-even", None, elems, smap),
                   expect("float32", "uint8", "nearest-even", None, elems + [nan | 1], smap),
                   expect("uint8", "float32", "nearest-even", None, [0, 1, 255], [(0, nan), (255, 0x12345678)])]
    full = [(M.scalar_bits(float(k), "float32"), k) for k in range(M.MAP_MAX)]
    last = [M.scalar_bits(float(M.MAP_MAX - 1), "float32")]
    assert run(harness, [line("float32", "uint8", "towards-zero", None, last, full)]) == [f"OK {M.MAP_MAX - 1:02x}"]


def test_cast_infallible_is_never_wrong(harness):
    """wherever the predicate holds, the model casts the edge list and the random elements without a
    failure; and it holds wherever the value sets say it can (it is exact, not merely safe)"""
    cases = [(s, t, oor) for s in M.TYPES for t in M.TYPES for oor in M.OUT_OF_RANGE]
    got = run(harness, [f"infallible {s} {t} {oor or 'none'}" for s, t, oor in cases])
    for (s, t, oor), g in zip(cases, got):
        assert g == ("1" if M.infallible(s, t, oor) else "0"), (s, t, oor)
        if g == "1":
            for r in M.ROUNDINGS:
                for elems in (M.edge_elements(s), M.xorshift_elements(s)):
                    assert M.cast_list(elems, s, t, r, oor)[1] is None, (s, t, r, oor)
    assert got[cases.index(("uint16", "float16", None))] == "0"
    assert got[cases.index(("uint64", "bfloat16", None))] == "1"
    assert got[cases.index(("float32", "int64", "clamp"))] == "0"
