"""constraint= on the host, against the stub library (tests/generation_stub.py) -- no GPU: the call sequence with a constraint is
the sequence without it plus one tcavt_constraint_build, one tcavt_constraint_mask before and one tcavt_constraint_advance after
every selection entry (inside the log-probability bracket), and a call without the argument is the call of before."""
import json
import os

import pytest
import torch

import generation_stub as GS

from tcavt_amd.constraint import TokenConstraint

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generation_trace.json")
PLAIN = dict(no_repeat_ngram_size=0)
BATCH = {  # name -> keyword arguments of generate_batch on 3 prompts
    "plain": dict(max_new_tokens=5),
    "n4": dict(max_new_tokens=5, num_return_sequences=4),
    "n4_shared": dict(max_new_tokens=5, num_return_sequences=4, share_prefix=True),
    "logprobs": dict(max_new_tokens=5, return_logprobs=True),
    "rules_info": dict(max_new_tokens=6, poll_every=2, stop_token_ids=[3, 5], return_info=True),
    "per_request": dict(max_new_tokens=4, temperature=[0.7, 0.9, 1.1]),
}
POOL = {"g1": (5, GS.POOL_1), "g4": (7, dict(GS.POOL_2, admit_group=4)), "g2_logprobs": (7, dict(GS.POOL_2, return_logprobs=True))}
SAMPLERS = ("tcavt_sample_logits", "tcavt_sample_logits_slots", "tcavt_sample_logits_rows", "tcavt_sample_tokens",
            "tcavt_sample_tokens_per_request")


def _constraint(cfg):
    return TokenConstraint.from_sequences(cfg.llama.vocab, [[11, 12], [20, 21, 22]], 5)


def _run(entry, R, kw, constrained):
    """-> (result of the call, recorded calls, workspace requests)"""
    with GS.stubbed() as stub:
        cfg, m = GS.tiny_model()
        vis, ids, mask = GS._requests(cfg, R)
        kw = dict(PLAIN, **kw)
        if constrained:
            kw.update(constraint=_constraint(cfg), constraint_start=[0] * R)
        if entry == "generate_batch":
            res = m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, pad_token_id=7, **kw)
        else:
            res = m.mllm.generate_pool(vis, ids, mask, use_graph=False, pad_token_id=7, **kw)
        m.mllm.check_flags()
    bufs = [[n, list(shape), str(dt)] for ws in (m.mllm._ws, m.mllm.llama_wrapper._ws) for n, shape, dt in ws._bufs]
    return res, stub.calls, bufs


def _rows(call):
    """Logits rows of a sampler, logprob or constraint call."""
    name, sc = call
    return sc[0]["rows"] if isinstance(sc[0], dict) else sc[0]


def _check(calls, plain_calls, logprobs):
    names = [c[0] for c in calls]
    assert names.count("tcavt_constraint_build") == 1
    build = calls[names.index("tcavt_constraint_build")][1][0]
    assert (build["n_states"], build["n_classes"]) == (7, 7) and build["V"] > 0
    n_sel = 0
    for i, c in enumerate(calls):
        if c[0] in SAMPLERS:
            n_sel += 1
            assert names[i - 1] == "tcavt_constraint_mask" and names[i + 1] == "tcavt_constraint_advance", names[max(i - 3, 0):i + 4]
            assert calls[i - 1][1] == calls[i + 1][1]  # one argument struct serves both launches
            assert _rows(calls[i - 1]) == _rows(c)
            assert names.index("tcavt_constraint_build") < i
            if logprobs:
                assert names[i - 2] == "tcavt_logprob_begin" and names[i + 2] == "tcavt_logprob_finish"
    assert n_sel > 0 and names.count("tcavt_constraint_mask") == names.count("tcavt_constraint_advance") == n_sel
    assert [c for c in calls if not c[0].startswith("tcavt_constraint_")] == plain_calls


@pytest.mark.parametrize("name", sorted(BATCH))
def test_generate_batch_brackets_every_selection(name):
    kw = BATCH[name]
    plain, plain_calls, plain_bufs = _run("generate_batch", 3, kw, False)
    res, calls, bufs = _run("generate_batch", 3, kw, True)
    _check(calls, plain_calls, bool(kw.get("return_logprobs")))
    rows = 3 * kw.get("num_return_sequences", 1)
    if kw.get("return_info"):
        state = res[1]["constraint_state"]
        assert tuple(state.shape) == (rows,) and state.dtype == torch.int32 and state.device.type == "cpu"
    elif isinstance(res, tuple):
        assert "constraint_state" not in res[1]
    # the constraint adds workspaces under new names and moves none of the others
    added = [b for b in bufs if b not in plain_bufs]
    assert [b for b in bufs if b in plain_bufs] == plain_bufs
    assert added and all(b[0] == "gen.cs.ws" and b[1] == [rows * 16] for b in added)


@pytest.mark.parametrize("name", sorted(POOL))
def test_generate_pool_brackets_every_selection(name):
    R, kw = POOL[name]
    plain, plain_calls, plain_bufs = _run("generate_pool", R, kw, False)
    res, calls, bufs = _run("generate_pool", R, kw, True)
    _check(calls, plain_calls, bool(kw.get("return_logprobs")))
    added = [b for b in bufs if b not in plain_bufs]
    assert [b for b in bufs if b in plain_bufs] == plain_bufs
    tags = {"pool.cs.ws", "pool.pf.cs.ws"} if kw["admit_group"] == 1 else {"pool.cs.ws", "pool.pg.cs.ws"}
    assert {b[0] for b in added} == tags
    sel = [_rows(c) for c in calls if c[0] in SAMPLERS]
    assert set(sel) == {kw["admit_group"], kw["slots"]}  # the admission's rows and the decode loop's slots
    # every start table and state array has the call's geometry
    for c in calls:
        if c[0] in ("tcavt_constraint_mask", "tcavt_constraint_advance"):
            assert c[1][0]["n_req"] == R and c[1][0]["n_state"] in (1, kw["slots"])


def test_pool_info_carries_the_final_states():
    (out, stats), calls, _ = _run("generate_pool", 5, dict(GS.POOL_1, return_info=True), True)
    assert tuple(stats["constraint_state"].shape) == (5,) and stats["constraint_state"].dtype == torch.int32
    (out, stats), calls, _ = _run("generate_pool", 0, dict(max_new_tokens=5, slots=2, return_info=True), True)
    assert calls == [] and tuple(stats["constraint_state"].shape) == (0,)


def test_without_the_argument_the_calls_are_those_of_the_golden_trace():
    with open(GOLDEN) as f:
        golden = json.load(f)
    now = GS.record_all()
    assert now == golden
    for rec in now.values():
        assert not any(c[0].startswith("tcavt_constraint_") for c in rec["calls"])
        assert not any(".cs." in b[0] for b in rec["workspace"])


@pytest.mark.parametrize("entry,R,kw", [("generate_batch", 3, BATCH["n4"]), ("generate_pool", 5, GS.POOL_1), ("generate_pool", 7, GS.POOL_2)])
def test_none_is_the_call_without_the_argument(entry, R, kw):
    res0, calls0, bufs0 = _run(entry, R, kw, False)
    res1, calls1, bufs1 = _run(entry, R, dict(kw, constraint=None, constraint_start=None), False)
    assert calls1 == calls0 and bufs1 == bufs0 and torch.equal(res0, res1)
