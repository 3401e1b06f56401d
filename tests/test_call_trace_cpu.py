"""The C calls of the model's host code, pinned across the split of model.py: for every scenario of
tests/golden/make_call_trace.py (forwards, training steps of both variants with and without dropout, the bf16 and
TCAVT_PY_TLAYERS=1 compositions, the LM passes) the ordered list of C entries with every argument -- scalars verbatim, structs
field by field, pointers as their aliasing pattern within the call -- and the workspace buffers (name, shape, dtype) in
allocation order equal what tests/golden/call_trace.json holds.  The file was recorded at the commit before the split.

One stated difference.  tcavt_ltsf_backward, tcavt_tlayer_stack_backward and tcavt_cross_attn_backward used to be handed a
second forward struct that the backward rebuilt from workspace names, holding only the fields the backward reads; they are now
handed the struct the forward's own stage call filled.  For these three entries the struct behind ``fwd`` (and ``xattn.fwd``,
and the TLayer array behind ``fwd->layers``) is compared after removing, on both sides, the pointer fields that are NULL in
the recorded file (NULL and zero fields are absent from a dump, so: the pointers the recorded struct does not have) -- the forward's struct carries more: biases, ``lane``, ``dec_t``, ``wk_t`` ... -- and renumbering the
pointers; every field the backward had set, and every field of the backward's own struct, still has to agree, aliasing
included.  One scalar of the forward's struct is exempt as well: ``add_last`` (the forward head adds x[:, :, -1:]; the backward
never reads it and its rebuilt struct left it 0).  The test then asserts by address that ``fwd`` IS the struct object the
preceding forward call of that module passed.  For that to be one object, phase 2 of tcavt_ltsf_forward continues on the
struct phase 1 filled instead of a second one: its call is compared under the same rule (the phase-1 pointers, NULL in the
recorded phase-2 call and not read by phase 2, are removed), every scalar included."""
import ctypes
import importlib.util
import json
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_call_trace", os.path.join(HERE, "golden", "make_call_trace.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

STAGE_BACKWARDS = tuple(rec.STAGE_FORWARDS.values())


@pytest.fixture(scope="module")
def golden():
    return rec.load(os.path.join(HERE, "golden", "call_trace.json"))


def _is_pointer(v):
    return isinstance(v, str) and re.fullmatch(r"p\d+", v) is not None


def _prune(x, want):
    """x without the pointers that `want` does not have (NULL there), all the way down, and without ``add_last``; a scalar that
    `want` does not have (zero there) stays and fails the comparison."""
    if isinstance(x, dict):
        return {k: _prune(v, want.get(k, v)) for k, v in x.items() if k != "add_last" and (k in want or not _is_pointer(v))}
    if isinstance(x, list):
        assert len(x) == len(want)
        return [_prune(a, w) for a, w in zip(x, want)]
    return x


def _renumber(x, seen):
    if isinstance(x, dict):
        return {k: _renumber(v, seen) for k, v in x.items()}
    if isinstance(x, list):
        return [_renumber(v, seen) for v in x]
    if _is_pointer(x):
        return "p%d" % seen.setdefault(x, len(seen))
    return x


def _comparable(call, want):
    """A call as it is compared: a stage backward with its forward struct cut down to what the recorded one names."""
    name, args = call
    if name == "tcavt_ltsf_forward" and args[1] == 2:
        return _renumber([name, [{k: v for k, v in args[0].items() if k in want[1][0] or not _is_pointer(v)}] + list(args[1:])], {})
    if name not in STAGE_BACKWARDS:
        return call
    a, w = dict(args[0]), want[1][0]
    a["fwd"] = _prune(a["fwd"], w["fwd"])
    if name == "tcavt_ltsf_backward":
        a["xattn"] = dict(a["xattn"], fwd=_prune(a["xattn"]["fwd"], w["xattn"]["fwd"]))
    return _renumber([name, [a] + list(args[1:])], {})


def test_golden_covers_every_scenario(golden):
    assert sorted(golden) == sorted(rec.SCENARIOS)
    names = lambda key: [c[0] for c in golden[key]["calls"]]
    for key in ("step_frozen", "step_frozen_dropout", "nolora_step_frozen"):  # the three stage backwards' default path
        assert names(key).count("tcavt_ltsf_backward") == 1 and names(key).count("tcavt_tlayer_stack_backward") == 1
    assert not any(n in STAGE_BACKWARDS or n in rec.STAGE_FORWARDS for n in names("py_tlayers_step_frozen"))


@pytest.mark.parametrize("name", list(rec.SCENARIOS))
def test_calls_and_workspaces_match_the_golden_trace(golden, name):
    dump, stub = rec.record(name)
    got, want = json.loads(json.dumps(dump)), golden[name]  # (tuples -> lists, as the file has them)
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]  # the entries first: the shorter message
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        g, w = _comparable(g, w), _comparable(w, w)
        if g != w:
            print(f"call {i} differs\n got: {json.dumps(g)}\nwant: {json.dumps(w)}")
        assert g == w, f"call {i} ({w[0]})"
    assert got["workspace"] == want["workspace"]
    # the stage backwards are handed the very struct the preceding stage forward of the same module passed
    for i, entry, bwd in stub.stage_backwards:
        fwd_entry = [k for k, v in rec.STAGE_FORWARDS.items() if v == entry][0]
        before = [obj for j, e, obj in stub.stage_forwards if j < i and e == fwd_entry]
        if entry == "tcavt_tlayer_stack_backward":  # the lane-polygon encoder's stack is the fp32 one (the Q-Former's are 16-bit)
            before = [obj for obj in before if obj.dtype16 == 0]
        assert before, f"call {i}: {entry} without a preceding {fwd_entry}"
        assert ctypes.addressof(bwd.fwd.contents) == ctypes.addressof(before[-1]), f"call {i}: {entry}.fwd is not the forward's struct"
        if entry == "tcavt_ltsf_backward":
            assert ctypes.addressof(bwd.xattn.fwd.contents) == ctypes.addressof(before[-1]) + type(before[-1]).xattn.offset
