"""top_logprobs on the host, against the stub library (tests/generation_stub.py, which records the new entry as it stands) -- no
GPU: every token selection of generate_batch, of the pool's step and of both admission forms is
    logprob_begin, logprob_topk, [constraint_mask], the selection, [constraint_advance], logprob_finish,
the launch is absent and no new workspace name is requested without the argument (a call with return_logprobs=True included), and
the illegal values are refused before any entry is called."""
import pytest
import torch

import generation_stub as GS

SAMPLERS = ("tcavt_sample_logits", "tcavt_sample_logits_slots", "tcavt_sample_logits_rows", "tcavt_sample_tokens",
            "tcavt_sample_tokens_per_request")
BATCH = {
    "n1": dict(max_new_tokens=5),
    "n3_shared": dict(max_new_tokens=5, num_return_sequences=3, share_prefix=True),
    "rules": dict(max_new_tokens=6, poll_every=2, stop_token_ids=[3, 5], min_new_tokens=1, eos_token_id=2),
}
POOL = {"g1": (5, GS.POOL_1), "g2": (7, GS.POOL_2)}


def _run(entry, R, kw, constraint=False):
    """-> (result of the call, recorded calls, workspace requests)"""
    with GS.stubbed() as stub:
        cfg, m = GS.tiny_model()
        vis, ids, mask = GS._requests(cfg, R)
        if constraint:
            from tcavt_amd.constraint import TokenConstraint

            kw = dict(kw, constraint=TokenConstraint.from_allowed_tokens(m.mllm.llama_wrapper.shape.vocab, [3, 4, 9]),
                      no_repeat_ngram_size=0)
        if entry == "generate_batch":
            res = m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, pad_token_id=7, **kw)
        else:
            res = m.mllm.generate_pool(vis, ids, mask, use_graph=False, pad_token_id=7, **kw)
    bufs = [[n, list(shape), str(dt)] for ws in (m.mllm._ws, m.mllm.llama_wrapper._ws) for n, shape, dt in ws._bufs]
    return res, stub.calls, bufs


def _check_order(calls, k, constraint=False):
    """Every selection sits in the full bracket; -> the rows of every selection."""
    names = [c[0] for c in calls]
    before = ["tcavt_logprob_begin", "tcavt_logprob_topk"] + (["tcavt_constraint_mask"] if constraint else [])
    after = (["tcavt_constraint_advance"] if constraint else []) + ["tcavt_logprob_finish"]
    rows = []
    for i, c in enumerate(calls):
        if c[0] in SAMPLERS:
            assert names[i - len(before):i] == before and names[i + 1:i + 1 + len(after)] == after, names[max(i - 4, 0):i + 4]
            begin, topk = calls[i - len(before)], calls[i - len(before) + 1]
            assert topk[1][0]["k"] == k and topk[1][0]["reserved0"] == 0 and topk[1][0]["workspace_bytes"] > 0
            rows.append(begin[1][0]["rows"])
    n_sel = len(rows)
    assert n_sel > 0 and names.count("tcavt_logprob_topk") == names.count("tcavt_logprob_begin") == names.count("tcavt_logprob_finish") == n_sel
    return rows


@pytest.mark.parametrize("name", sorted(BATCH))
@pytest.mark.parametrize("constraint", (False, True))
def test_generate_batch_launch_order(name, constraint):
    kw = dict(BATCH[name], return_logprobs=True)
    if constraint and "min_new_tokens" in kw:
        kw = dict(kw, min_new_tokens=0)  # (a constraint needs min_new_tokens = 0)
    (_, base_info), base_calls, base_bufs = _run("generate_batch", 3, kw, constraint)
    (out, info), calls, bufs = _run("generate_batch", 3, dict(kw, top_logprobs=4), constraint)
    _check_order(calls, 4, constraint)
    # without the new launch the calls are those of return_logprobs=True alone, and only new workspace names are added
    assert [c for c in calls if c[0] != "tcavt_logprob_topk"] == base_calls
    assert [b for b in bufs if b in base_bufs] == base_bufs
    added = [b for b in bufs if b not in base_bufs]
    assert added and all(b[0] == "gen.lp.top.ws" for b in added)
    rows, N = tuple(out.shape)
    for key, dt in (("top_token_ids", torch.int64), ("top_token_logprobs", torch.float32)):
        assert tuple(info[key].shape) == (rows, N, 4) and info[key].dtype == dt and info[key].device.type == "cpu", key
    # the stub writes nothing: the caller's initial values are what comes back
    assert bool((info["top_token_ids"] == -1).all()) and bool((info["top_token_logprobs"] == float("-inf")).all())
    assert "top_token_ids" not in base_info and "top_token_logprobs" not in base_info


@pytest.mark.parametrize("name", sorted(POOL))
@pytest.mark.parametrize("constraint", (False, True))
def test_generate_pool_launch_order_in_the_step_and_in_an_admission(name, constraint):
    R, kw = POOL[name]
    kw = dict(kw, return_logprobs=True)
    (_, base_stats), base_calls, base_bufs = _run("generate_pool", R, kw, constraint)
    (out, stats), calls, bufs = _run("generate_pool", R, dict(kw, top_logprobs=20), constraint)
    sel_rows = _check_order(calls, 20, constraint)
    assert set(sel_rows) == {kw["admit_group"], kw["slots"]}  # the admissions' rows and the decode step's slots
    assert [c for c in calls if c[0] != "tcavt_logprob_topk"] == base_calls
    assert [b for b in bufs if b in base_bufs] == base_bufs
    tags = {"pool.lp.top.ws", "pool.pf.lp.top.ws"} if kw["admit_group"] == 1 else {"pool.lp.top.ws", "pool.pg.lp.top.ws"}
    assert {b[0] for b in bufs if b not in base_bufs} == tags
    N = max(kw["max_new_tokens"])
    assert tuple(stats["top_token_ids"].shape) == tuple(stats["top_token_logprobs"].shape) == (R, N, 20)
    assert stats["top_token_ids"].dtype == torch.int64 and stats["top_token_logprobs"].dtype == torch.float32
    assert "top_token_ids" not in base_stats


@pytest.mark.parametrize("entry,R,kw", [("generate_batch", 3, BATCH["n1"]), ("generate_batch", 3, BATCH["rules"]),
                                        ("generate_pool", 5, GS.POOL_1), ("generate_pool", 7, GS.POOL_2)])
@pytest.mark.parametrize("logprobs", (False, True))
def test_without_the_argument_nothing_changes(entry, R, kw, logprobs):
    kw = dict(kw, return_logprobs=logprobs)
    res0, calls0, bufs0 = _run(entry, R, kw)
    res1, calls1, bufs1 = _run(entry, R, dict(kw, top_logprobs=None))
    assert calls1 == calls0 and bufs1 == bufs0
    assert not any(c[0] == "tcavt_logprob_topk" for c in calls0)
    assert not any(".top." in b[0] for b in bufs0)
    if logprobs:
        assert sorted(res0[1]) == sorted(res1[1]) and "top_token_ids" not in res1[1]


def test_empty_pool_returns_empty_records():
    (out, stats), calls, _ = _run("generate_pool", 0, dict(max_new_tokens=5, slots=2, return_logprobs=True, top_logprobs=3))
    assert calls == []
    assert tuple(stats["top_token_ids"].shape) == (0, 5, 3) and stats["top_token_ids"].dtype == torch.int64
    assert tuple(stats["top_token_logprobs"].shape) == (0, 5, 3) and stats["top_token_logprobs"].dtype == torch.float32


@pytest.mark.parametrize("bad", [0, 21, -1, True, False, 2.5, "5", [5]])
def test_illegal_values_are_refused_before_any_entry(bad):
    with GS.stubbed() as stub:
        cfg, m = GS.tiny_model()
        vis, ids, mask = GS._requests(cfg, 3)
        with pytest.raises(ValueError, match="top_logprobs must be None or an int in \\[1, 20\\]"):
            m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, max_new_tokens=3, return_logprobs=True, top_logprobs=bad)
        with pytest.raises(ValueError, match="top_logprobs must be None or an int in \\[1, 20\\]"):
            m.mllm.generate_pool(vis, ids, mask, max_new_tokens=3, slots=2, return_logprobs=True, top_logprobs=bad)
        assert stub.calls == [] and not m.mllm._ws._bufs


def test_the_argument_needs_return_logprobs_and_inherits_its_refusals():
    with GS.stubbed() as stub:
        cfg, m = GS.tiny_model()
        vis, ids, mask = GS._requests(cfg, 3)
        with pytest.raises(ValueError, match="top_logprobs needs return_logprobs=True"):
            m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, max_new_tokens=3, top_logprobs=5)
        with pytest.raises(ValueError, match="top_logprobs needs return_logprobs=True"):
            m.mllm.generate_pool(vis, ids, mask, max_new_tokens=3, slots=2, top_logprobs=5)
        with pytest.raises(ValueError, match="return_logprobs is not built for num_beams > 1"):
            m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, max_new_tokens=3, return_logprobs=True, top_logprobs=5,
                                  num_beams=2, do_sample=False)
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens is not built for return_logprobs=True"):
            m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, max_new_tokens=3, return_logprobs=True, top_logprobs=5,
                                  prompt_lookup_num_tokens=2)
        assert stub.calls == [] and not m.mllm._ws._bufs
