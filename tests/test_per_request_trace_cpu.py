"""Per-request sampling parameters on the host, against the stub library (tests/generation_stub.py) -- no GPU: a generate_pool / a
generate_batch call with ONE argument given as a list records the launch sequence of the same call with scalars, every sampler
entry replaced one for one by tcavt_sample_tokens_per_request (computed here from the two recordings); wrong lengths, bad elements
and lists together with beams or prompt lookup raise ValueError before any entry is called or any workspace buffer requested; an
empty request list returns the empty result; a call with scalars is the call of before."""
import pytest
import torch

import generation_stub as GS

SAMPLERS = ("tcavt_sample_logits", "tcavt_sample_logits_slots", "tcavt_sample_logits_rows", "tcavt_sample_tokens")
NEW = "tcavt_sample_tokens_per_request"
RULES = dict(stop_token_ids=[3, 5], return_info=True)


@pytest.fixture(autouse=True)
def _stub_plays_the_new_entry(monkeypatch):
    """The stub plays a sampler's part in the bookkeeping by name; the new entry does what tcavt_sample_tokens does there."""
    monkeypatch.setattr(GS.StubLibrary, "_sample_tokens_per_request", lambda self, args, req, stream: self._sample_tokens(args, stream),
                        raising=False)


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
    """(rows, V, n_state) of a sampler call."""
    name, sc = call
    if name in ("tcavt_sample_tokens", NEW):
        return sc[0]["rows"], sc[0]["V"], sc[0]["n_state"]
    if name == "tcavt_sample_logits_rows":
        return sc[0], sc[1], sc[2]
    return sc[0], sc[1], sc[0]  # batch / slots: one state entry per logits row


def _check_one_for_one(calls, plain_calls, n_req):
    assert len(calls) == len(plain_calls)
    n_sel = 0
    for c, p in zip(calls, plain_calls):
        if p[0] in SAMPLERS:
            n_sel += 1
            assert c[0] == NEW, (c[0], p[0])
            assert _geometry(c) == _geometry(p)
            if p[0] == "tcavt_sample_tokens":
                assert c[1][0] == p[1][0]  # the same argument struct, integer for integer
            assert c[1][1]["n_req"] == n_req
        else:
            assert c == p
    assert n_sel > 0 and not any(c[0] in SAMPLERS for c in calls)


POOL = {  # name -> (requests, scalar arguments, the one argument as a list)
    "g1_temperature": (5, GS.POOL_1, dict(temperature=[0.7, 0.9, 1.3, 1.0, 0.5])),
    "g1_do_sample": (5, GS.POOL_1, dict(do_sample=[True, False, True, False, True])),
    "g2_seed": (7, GS.POOL_2, dict(seed=torch.arange(7) + (1 << 40))),
    "g2_rules_eos": (7, dict(GS.POOL_2, **RULES), dict(eos_token_id=[None, 2, None, 4, 2, None, 9])),
    "g1_rules_min_new": (5, dict(GS.POOL_1, **RULES), dict(min_new_tokens=[0, 2, 0, 1, 3])),
}
BATCH = {
    "n1_top_k": (dict(max_new_tokens=5), dict(top_k=[1, 40, 256])),
    "n1_top_p": (dict(max_new_tokens=1), dict(top_p=(0.5, 0.9, 1.0))),
    "n2_repetition_penalty": (dict(max_new_tokens=5, num_return_sequences=2), dict(repetition_penalty=[1.0, 1.2, 1.5])),
    "n3_shared_ngram": (dict(max_new_tokens=5, num_return_sequences=3, share_prefix=True), dict(no_repeat_ngram_size=torch.tensor([0, 3, 2]))),
    "rules_poll_min_new": (dict(max_new_tokens=6, poll_every=2, eos_token_id=2, **RULES), dict(min_new_tokens=[1, 0, 2])),
    "logprobs_temperature": (dict(max_new_tokens=4, return_logprobs=True), dict(temperature=[0.7, 1.0, 1.3])),
}


@pytest.mark.parametrize("name", sorted(POOL))
def test_generate_pool_replaces_every_sampler_entry(name):
    R, kw, listed = POOL[name]
    plain, plain_calls, plain_bufs = _run("generate_pool", R, kw)
    res, calls, bufs = _run("generate_pool", R, dict(kw, **listed))
    _check_one_for_one(calls, plain_calls, R)
    assert bufs == plain_bufs  # the table is no workspace buffer
    out, out_plain = (res[0], plain[0]) if isinstance(res, tuple) else (res, plain)
    assert out.shape == out_plain.shape
    # the three sampler uses are all there: the admission's rows and the decode loop's slots
    assert {_geometry(c)[0] for c in calls if c[0] == NEW} == {kw["admit_group"], kw["slots"]}


@pytest.mark.parametrize("name", sorted(BATCH))
def test_generate_batch_replaces_every_sampler_entry(name):
    kw, listed = BATCH[name]
    plain, plain_calls, plain_bufs = _run("generate_batch", 3, kw)
    res, calls, bufs = _run("generate_batch", 3, dict(kw, **listed))
    _check_one_for_one(calls, plain_calls, 3 * kw.get("num_return_sequences", 1))  # one entry per decode row
    assert bufs == plain_bufs


@pytest.mark.parametrize("entry,R,kw", [("generate_batch", 3, dict(max_new_tokens=5, num_return_sequences=2)),
                                        ("generate_batch", 3, dict(max_new_tokens=6, poll_every=2, **RULES)),
                                        ("generate_pool", 5, GS.POOL_1), ("generate_pool", 7, dict(GS.POOL_2, **RULES))])
def test_scalars_are_the_call_of_before(entry, R, kw):
    """Every argument one value, the defaults spelled out or not: no new entry, and 0-d tensors count as one value."""
    res0, calls0, bufs0 = _run(entry, R, kw)
    spelled = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.9, repetition_penalty=1.2, no_repeat_ngram_size=3, seed=0,
                   min_new_tokens=0)
    res1, calls1, bufs1 = _run(entry, R, dict(kw, **spelled))
    res2, calls2, bufs2 = _run(entry, R, dict(kw, temperature=torch.tensor(0.9), seed=torch.tensor(0)))
    assert calls1 == calls0 and bufs1 == bufs0 and calls2 == calls0 and bufs2 == bufs0
    assert not any(c[0] == NEW for c in calls0)


def _refused(entry, R, kw, match):
    with GS.stubbed() as stub:
        cfg, m = GS.tiny_model()
        vis, ids, mask = GS._requests(cfg, R)
        with pytest.raises(ValueError, match=match):
            if entry == "generate_batch":
                m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, pad_token_id=7, **kw)
            else:
                m.mllm.generate_pool(vis, ids, mask, use_graph=False, pad_token_id=7, **kw)
        assert stub.calls == [] and not m.mllm._ws._bufs and not m.mllm.llama_wrapper._ws._bufs


BAD = [  # (argument as given, what the error names)
    (dict(temperature=[0.9, 1.0]), r"temperature has 2 values for 3 requests"),
    (dict(seed=[1, 2, 3, 4]), r"seed has 4 values for 3 requests"),
    (dict(top_k=torch.zeros(2, 3)), r"top_k"),
    (dict(temperature=[0.9, 0.0, 1.0]), r"temperature\[1\]"),
    (dict(temperature=[0.9, 1.0, -1.0]), r"temperature\[2\]"),
    (dict(top_k=[40, 0, 5]), r"top_k\[1\]"),
    (dict(top_k=[257, 1, 5]), r"top_k\[0\]"),
    (dict(top_p=[0.9, 0.9, 0.0]), r"top_p\[2\]"),
    (dict(top_p=[1.5, 0.9, 1.0]), r"top_p\[0\]"),
    (dict(repetition_penalty=[1.2, 0.0, 1.0]), r"repetition_penalty\[1\]"),
    (dict(no_repeat_ngram_size=[0, 3, -1]), r"no_repeat_ngram_size\[2\]"),
    (dict(min_new_tokens=[0, -1, 0], eos_token_id=2), r"min_new_tokens\[1\]"),
    (dict(min_new_tokens=[0, 2, 0]), r"min_new_tokens\[1\].*nothing to ban"),
    (dict(min_new_tokens=[1, 2, 1], eos_token_id=[2, 2, None]), r"min_new_tokens\[2\].*nothing to ban"),
    (dict(temperature=[0.9, "hot", 1.0]), r"temperature\[1\]"),
    (dict(top_k=[40, 2.5, 5]), r"top_k\[1\]"),
    (dict(do_sample=[True, False, True], temperature=0.0), r"temperature = 0.0 .*request 0"),  # a scalar that is illegal for a request
]


@pytest.mark.parametrize("entry", ["generate_batch", "generate_pool"])
@pytest.mark.parametrize("bad,match", BAD, ids=[m for _, m in BAD])
def test_wrong_lengths_and_bad_elements_are_refused_before_any_entry(entry, bad, match):
    kw = dict(max_new_tokens=4, **bad) if entry == "generate_batch" else dict(max_new_tokens=4, slots=2, **bad)
    _refused(entry, 3, kw, match)


def test_greedy_requests_do_not_need_legal_warper_values():
    """temperature, top_k and top_p of a greedy request are not looked at, as for a greedy call."""
    kw = dict(max_new_tokens=3, slots=2, do_sample=[False, True, False], temperature=[0.0, 0.9, -1.0], top_k=[0, 40, 1000])
    res, calls, _ = _run("generate_pool", 3, kw)
    assert any(c[0] == NEW for c in calls)


@pytest.mark.parametrize("other", [dict(num_beams=2, do_sample=False), dict(prompt_lookup_num_tokens=3)], ids=["beams", "prompt_lookup"])
@pytest.mark.parametrize("listed", [dict(repetition_penalty=[1.0, 1.2, 1.5]), dict(eos_token_id=[2, None, 2]), dict(seed=[1, 2, 3])],
                         ids=["repetition_penalty", "eos_token_id", "seed"])
def test_lists_are_refused_with_beams_and_prompt_lookup(listed, other):
    _refused("generate_batch", 3, dict(max_new_tokens=4, **listed, **other), "per-request values .* are not built for")


def test_an_empty_request_list_returns_the_empty_result():
    res, calls, _ = _run("generate_pool", 0, dict(max_new_tokens=5, slots=2, temperature=[], seed=[]))
    assert calls == [] and tuple(res.shape) == (0, 5)
    (out, stats), calls, _ = _run("generate_pool", 0, dict(max_new_tokens=5, slots=2, min_new_tokens=[], return_info=True))
    assert calls == [] and tuple(out.shape) == (0, 5) and tuple(stats["finish_reason"].shape) == (0,)
    _refused("generate_pool", 0, dict(max_new_tokens=5, slots=2, temperature=[0.9]), "temperature has 1 values for 0 requests")


def test_first_end_takes_the_requests_minimum():
    from tcavt_amd.stopping import StopRules

    rules = StopRules(100, stop_token_ids=[5], min_new_tokens=[0, 2, 3])
    assert not rules.empty and [rules.min_new(r) for r in range(3)] == [0, 2, 3] and rules.min_new_tokens == 0
    assert StopRules(100, min_new_tokens=[0, 0]).empty
    assert rules.first_end([9, 5, 7], 7, request=0) == (2, 2)
    assert rules.first_end([9, 8, 7, 5], 7, request=1) == (3, 1)  # the request's own EOS, past its minimum
    assert rules.first_end([9, 8, 7, 5], None, request=1) == (4, 2)  # ... which another request does not have
    with pytest.raises(ValueError, match="banned before its minimum 3"):
        rules.first_end([9, 5, 7], 7, request=2)  # a token the sampler cannot have emitted
    rules.check_bannable(2, None)  # (the stop set is there to ban)
    with pytest.raises(ValueError, match="nothing to ban"):
        StopRules(100).check_bannable(2, None)
    StopRules(100).check_bannable(2, 7)
    StopRules(100).check_bannable(0, None)
