"""The write path's encoded bytes against digests recorded before its host side was refactored
(tests/golden/encode_digests.json, written by tools/encode_golden.py at the commit before encode_layout.cpp
and never regenerated from the code under test): every case's inputs are rebuilt from their seeds and every
encoded chunk must have the recorded length and SHA-256. Two recordings in separate processes agreed on
every case, so every case is held to its digest."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import encode_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_digests.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from zarrs_amd import Context
    return Context(0)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(list(G.ENCODE_CASES) + list(G.STORE_CASES))
    assert set(G.DETERMINISTIC) <= set(GOLDEN)
    for name, rec in GOLDEN.items():
        assert len(rec["lens"]) == len(rec["sha256"]) >= 1 and all(len(h) == 64 for h in rec["sha256"]), name


@pytest.mark.parametrize("name", list(G.ENCODE_CASES))
def test_encoded_chunks_match_the_recording(ctx, torch_cuda, name):
    assert G.digest(G.encode_case(ctx, torch_cuda, name)) == GOLDEN[name]


@pytest.mark.parametrize("name", list(G.STORE_CASES))
def test_stored_shards_match_the_recording(ctx, name):
    assert G.digest(G.store_case(ctx, name)) == GOLDEN[name]
