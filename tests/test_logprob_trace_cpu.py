"""return_logprobs on the host, against the stub library (tests/generation_stub.py) -- no GPU: every sampler call is bracketed by
exactly one tcavt_logprob_begin and one tcavt_logprob_finish of the same geometry, the sampler entry is the one the call chooses
without the flag, the info carries the three arrays, and a call with the flag off is the call that does not pass it."""
import pytest
import torch

import generation_stub as GS

RULES = dict(stop_token_ids=[3, 5], min_new_tokens=1, eos_token_id=2)
BATCH = {  # name -> keyword arguments of generate_batch on 3 prompts
    "n1": dict(max_new_tokens=5),
    "n3": dict(max_new_tokens=5, num_return_sequences=3),
    "n3_shared": dict(max_new_tokens=5, num_return_sequences=3, share_prefix=True),
    "rules": dict(max_new_tokens=6, poll_every=2, **RULES),
    "info": dict(max_new_tokens=4, return_info=True),
}
POOL = {"g1": (5, GS.POOL_1), "g2": (7, GS.POOL_2), "g2_rules": (7, dict(GS.POOL_2, **RULES))}  # name -> (requests, arguments)
SAMPLERS = ("tcavt_sample_logits", "tcavt_sample_logits_slots", "tcavt_sample_logits_rows", "tcavt_sample_tokens")


def _run(entry, R, kw):
    """-> (result of the call, recorded calls, workspace requests)"""
    with GS.stubbed() as stub:
        cfg, m = GS.tiny_model()
        vis, ids, mask = GS._requests(cfg, R)
        if entry == "generate_batch":
            res = m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, pad_token_id=7, **kw)
        else:
            res = m.mllm.generate_pool(vis, ids, mask, use_graph=False, pad_token_id=7, **kw)
    bufs = [[n, list(shape), str(dt)] for ws in (m.mllm._ws, m.mllm.llama_wrapper._ws) for n, shape, dt in ws._bufs]
    return res, stub.calls, bufs


def _geometry(call):
    """(rows, V, n_state) of a sampler or logprob call."""
    name, sc = call
    if name in ("tcavt_sample_tokens", "tcavt_logprob_begin", "tcavt_logprob_finish"):
        return sc[0]["rows"], sc[0]["V"], sc[0]["n_state"]
    if name == "tcavt_sample_logits_rows":
        return sc[0], sc[1], sc[2]
    return sc[0], sc[1], sc[0]  # batch / slots: one state entry per logits row


def _check_brackets(calls, plain_calls):
    names = [c[0] for c in calls]
    n_sel = 0
    for i, c in enumerate(calls):
        if c[0] in SAMPLERS:
            n_sel += 1
            assert names[i - 1] == "tcavt_logprob_begin" and names[i + 1] == "tcavt_logprob_finish", names[max(i - 2, 0):i + 3]
            assert _geometry(calls[i - 1]) == _geometry(c) == _geometry(calls[i + 1])
            assert calls[i - 1][1] == calls[i + 1][1]  # one argument struct serves both launches
    assert n_sel > 0 and names.count("tcavt_logprob_begin") == names.count("tcavt_logprob_finish") == n_sel
    # without the bracket the recorded calls are those of the call without the flag: same sampler entries, same everything else
    assert [c for c in calls if not c[0].startswith("tcavt_logprob_")] == plain_calls


@pytest.mark.parametrize("name", sorted(BATCH))
def test_generate_batch_brackets_every_selection(name):
    kw = BATCH[name]
    plain, plain_calls, plain_bufs = _run("generate_batch", 3, kw)
    (out, info), calls, bufs = _run("generate_batch", 3, dict(kw, return_logprobs=True))
    _check_brackets(calls, plain_calls)
    rows, N = 3 * kw.get("num_return_sequences", 1), kw["max_new_tokens"]
    assert tuple(out.shape) == (rows, N)
    for key, shape, dt in (("token_logprobs", (rows, N), torch.float32), ("sum_logprob", (rows,), torch.float32),
                           ("n_scored", (rows,), torch.int32)):
        assert tuple(info[key].shape) == shape and info[key].dtype == dt and info[key].device.type == "cpu", key
    assert ("finish_reason" in info) == bool(kw.get("return_info")) and "steps" in info
    # the flag adds workspaces under new names, after the first selection's own, and moves none of the others
    added = [b for b in bufs if b not in plain_bufs]
    assert [b for b in bufs if b in plain_bufs] == plain_bufs
    assert added and all(b[0] == "gen.lp.ws" for b in added)


@pytest.mark.parametrize("name", sorted(POOL))
def test_generate_pool_brackets_every_selection(name):
    R, kw = POOL[name]
    plain, plain_calls, plain_bufs = _run("generate_pool", R, kw)
    (out, stats), calls, bufs = _run("generate_pool", R, dict(kw, return_logprobs=True))
    _check_brackets(calls, plain_calls)
    N = max(kw["max_new_tokens"])
    for key, shape, dt in (("token_logprobs", (R, N), torch.float32), ("sum_logprob", (R,), torch.float32), ("n_scored", (R,), torch.int32)):
        assert tuple(stats[key].shape) == shape and stats[key].dtype == dt and stats[key].device.type == "cpu", key
    assert ("finish_reason" in stats) == ("stop_token_ids" in kw)
    added = [b for b in bufs if b not in plain_bufs]
    assert [b for b in bufs if b in plain_bufs] == plain_bufs
    tags = {"pool.lp.ws", "pool.pf.lp.ws"} if kw["admit_group"] == 1 else {"pool.lp.ws", "pool.pg.lp.ws"}
    assert {b[0] for b in added} == tags
    # the three sampler uses are all there: the admission's rows and the decode loop's slots
    sel = [_geometry(c)[0] for c in calls if c[0] in SAMPLERS]
    assert set(sel) == {kw["admit_group"], kw["slots"]}


def test_empty_pool_returns_empty_records():
    (out, stats), calls, _ = _run("generate_pool", 0, dict(max_new_tokens=5, slots=2, return_logprobs=True))
    assert calls == [] and tuple(stats["token_logprobs"].shape) == (0, 5) and stats["n_scored"].dtype == torch.int32


@pytest.mark.parametrize("entry,R,kw", [("generate_batch", 3, BATCH["n3"]), ("generate_batch", 3, BATCH["rules"]),
                                        ("generate_pool", 5, GS.POOL_1), ("generate_pool", 7, GS.POOL_2)])
def test_flag_off_is_the_call_without_the_argument(entry, R, kw):
    res0, calls0, bufs0 = _run(entry, R, kw)
    res1, calls1, bufs1 = _run(entry, R, dict(kw, return_logprobs=False))
    assert calls1 == calls0 and bufs1 == bufs0
    assert torch.is_tensor(res1) and torch.equal(res0, res1)  # no info tuple appears
    assert not any(c[0].startswith("tcavt_logprob_") for c in calls0)
    assert not any(".lp." in b[0] for b in bufs0)


@pytest.mark.parametrize("bad", [1, 0, None, "yes", 1.0])
def test_non_bool_is_refused_before_any_entry(bad):
    with GS.stubbed() as stub:
        cfg, m = GS.tiny_model()
        vis, ids, mask = GS._requests(cfg, 3)
        with pytest.raises(ValueError, match="return_logprobs must be a bool"):
            m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, max_new_tokens=3, return_logprobs=bad)
        with pytest.raises(ValueError, match="return_logprobs must be a bool"):
            m.mllm.generate_pool(vis, ids, mask, max_new_tokens=3, slots=2, return_logprobs=bad)
        assert stub.calls == [] and not m.mllm._ws._bufs
