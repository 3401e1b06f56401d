"""The launch sequence of text generation's host code, pinned: for every scenario of generation_stub.SCENARIOS the ordered list of C
entries called (with their integer scalars: row counts, rows, src_lmax, kv_lmax, G, S, advance_pos, slot ...) and the workspace
buffers (name, shape, dtype) in allocation order equal what tests/golden/generation_trace.json holds.  The golden file was
recorded with ``python tests/generation_stub.py`` at the commit before generation.py was split out of model.py; a change to it
is a change of launches or buffers and needs its own reason."""
import json
import os

import pytest

import generation_stub

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generation_trace.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_every_scenario(golden):
    assert sorted(golden) == sorted(f"{name}/{kv}" for name in generation_stub.SCENARIOS for kv in ("fp16", "fp8"))
    assert golden["pool_empty/fp16"] == dict(calls=[], workspace=[])  # no request: nothing launched, nothing allocated
    for key, want in golden.items():
        if not key.startswith("pool_empty"):
            names = [c[0] for c in want["calls"]]
            assert "tcavt_llama_stack_forward" in names and any(n.startswith("tcavt_sample_") for n in names), key


@pytest.mark.parametrize("kv_cache", ["fp16", "fp8"])
@pytest.mark.parametrize("name", list(generation_stub.SCENARIOS))
def test_launch_sequence_and_workspace_match_the_golden_trace(golden, name, kv_cache):
    got = json.loads(json.dumps(generation_stub.record(name, kv_cache)))  # (tuples -> lists, as the file has them)
    want = golden[f"{name}/{kv_cache}"]
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]  # the entries first: the shorter message
    assert got["calls"] == want["calls"]
    assert got["workspace"] == want["workspace"]
