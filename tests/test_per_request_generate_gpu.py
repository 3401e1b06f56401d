"""Per-request sampling parameters through the whole stack, on the tiny generation fixture (3 requests): in a call with mixed
parameters request r gets exactly the tokens, finish_reason, n_generated and log-probabilities that row r gets in the call where
ALL requests use its parameters p_r -- whatever the slots, the schedule, the admission width's rows, eager or hipGraph, the poll
interval and the partners' parameters.  (The decode step's logits do not depend on the row count at this model's shape, as
DESIGN.md states for the pool; for generate_pool the comparison is made at the same admit_group.)

  request 0   greedy, repetition_penalty 1.0, no_repeat_ngram_size 0
  request 1   sampled, T 0.7, top_k 5, seed 5
  request 2   sampled, T 1.3, top_p 0.55, seed 6, repetition_penalty 1.2, no_repeat_ngram_size 3
"""
import numpy as np
import pytest
import torch

from tests.util import load_generation_case

pytestmark = pytest.mark.gpu

PAD, N, EOS = 7, 12, 268
KEYS = ("do_sample", "temperature", "top_k", "top_p", "repetition_penalty", "no_repeat_ngram_size", "seed")
P = [dict(do_sample=False, temperature=0.9, top_k=40, top_p=0.9, repetition_penalty=1.0, no_repeat_ngram_size=0, seed=0),
     dict(do_sample=True, temperature=0.7, top_k=5, top_p=0.9, repetition_penalty=1.2, no_repeat_ngram_size=3, seed=5),
     dict(do_sample=True, temperature=1.3, top_k=40, top_p=0.55, repetition_penalty=1.2, no_repeat_ngram_size=3, seed=6)]
MIXED = {k: [p[k] for p in P] for k in KEYS}
_MODEL, _UNIFORM = {}, {}


def _setup(dev):
    """The fixture model, built once for the module."""
    if "m" not in _MODEL:
        from tcavt_amd import model

        fx, cfg, weights, t = load_generation_case()
        m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights, device=dev).eval()
        _MODEL.update(m=m, fx=fx, cfg=cfg, g={k: v.to(dev) for k, v in t.items()})
    return _MODEL


def _pool(M, **kw):
    g = M["g"]
    res = M["m"].mllm.generate_pool(g["vision_emb"], g["input_ids"], g["attention_mask"], pad_token_id=PAD, **kw)
    torch.cuda.synchronize()
    M["m"].mllm.check_flags()
    return (res[0].cpu(), res[1]) if isinstance(res, tuple) else res.cpu()


def _batch(M, **kw):
    g = M["g"]
    res = M["m"].mllm.generate_batch(g["vision_emb"], None, input_ids=g["input_ids"], attention_mask=g["attention_mask"], pad_token_id=PAD, **kw)
    torch.cuda.synchronize()
    M["m"].mllm.check_flags()
    return (res[0].cpu(), res[1]) if isinstance(res, tuple) else res.cpu()


def _uniform_pool(M, r, budgets, G, **kw):
    """The call where every request uses p_r (2 slots, eager, polled every step): computed once per setting, never changed."""
    key = ("pool", r, tuple(budgets), G, tuple(sorted(kw.items())))
    if key not in _UNIFORM:
        _UNIFORM[key] = _pool(M, max_new_tokens=list(budgets), slots=2, admit_group=G, use_graph=False, **P[r], **kw)
    return _UNIFORM[key]


@pytest.mark.parametrize("G", [1, 2], ids=["admit1", "admit2"])
@pytest.mark.parametrize("budgets", [(12, 12, 12), (3, 12, 12)], ids=["even", "refill"])
def test_pool_rows_equal_the_uniform_calls(gpu, budgets, G):
    M = _setup(gpu["device"])
    want = torch.stack([_uniform_pool(M, r, budgets, G)[r] for r in range(3)])
    assert not torch.equal(want[1], want[2]) and ((want >= 0) & (want < M["cfg"].llama.vocab)).all()
    assert (want[0, budgets[0]:] == PAD).all()
    for slots in (2, 3):
        for use_graph in (False, True):
            for poll_every in (1, 3):
                out = _pool(M, max_new_tokens=list(budgets), slots=slots, admit_group=G, use_graph=use_graph, poll_every=poll_every, **MIXED)
                assert torch.equal(out, want), (slots, use_graph, poll_every)
    # the table's forms are interchangeable: tuples and 1-D tensors
    as_tensors = dict(MIXED, temperature=torch.tensor(MIXED["temperature"]), seed=torch.tensor(MIXED["seed"]), top_k=tuple(MIXED["top_k"]))
    assert torch.equal(_pool(M, max_new_tokens=list(budgets), slots=2, admit_group=G, **as_tensors), want)


def test_pool_with_the_fp8_cache(gpu):
    M = _setup(gpu["device"])
    want = torch.stack([_uniform_pool(M, r, (3, 12, 12), 1, kv_cache="fp8")[r] for r in range(3)])
    out = _pool(M, max_new_tokens=[3, 12, 12], slots=2, kv_cache="fp8", **MIXED)
    assert torch.equal(out, want)


def test_pool_records_and_logprobs_equal_the_uniform_calls(gpu):
    M = _setup(gpu["device"])
    kw = dict(return_info=True, return_logprobs=True, stop_token_ids=[5])
    uni = [_uniform_pool(M, r, (3, 12, 12), 2, **{k: (tuple(v) if isinstance(v, list) else v) for k, v in kw.items()}) for r in range(3)]
    out, stats = _pool(M, max_new_tokens=[3, 12, 12], slots=3, admit_group=2, stop_token_ids=[5], return_info=True, return_logprobs=True, **MIXED)
    for r in range(3):
        o, s = uni[r]
        assert torch.equal(out[r], o[r]), r
        for key in ("finish_reason", "n_generated", "token_logprobs", "sum_logprob", "n_scored"):
            assert torch.equal(stats[key][r], s[key][r]), (key, r)
    assert stats["n_generated"].tolist()[0] == 3 and (stats["finish_reason"] != 0).all()


def test_a_request_ends_on_its_own_eos_only(gpu):
    """Request 0 with EOS 268 reproduces the fixture's greedy row and ends after three tokens; its neighbours have no EOS and run
    on -- request 1 even past a 268 of its own, if it draws one."""
    M = _setup(gpu["device"])
    ref = M["fx"]["greedy_tokens"]
    assert int(ref[0, 2]) == EOS and EOS not in ref[0, :2].tolist()
    plain = _pool(M, max_new_tokens=N, slots=2, **MIXED)
    for G in (1, 2):
        out, stats = _pool(M, max_new_tokens=N, slots=2, admit_group=G, eos_token_id=[EOS, None, None], return_info=True, **MIXED)
        assert np.array_equal(out[0, :3].numpy(), ref[0, :3]) and (out[0, 3:] == PAD).all()
        assert stats["finish_reason"].tolist() == [1, 4, 4] and stats["n_generated"].tolist() == [3, N, N]
        if G == 1:
            assert torch.equal(out[1:], plain[1:])
    # the EOS moved to request 1: request 0 runs through its 268
    out, stats = _pool(M, max_new_tokens=N, slots=2, eos_token_id=[None, EOS, None], return_info=True, **MIXED)
    assert np.array_equal(out[0].numpy(), ref[0, :N]) and stats["finish_reason"].tolist()[0] == 4
    # per-request minimum: with min_new_tokens = 5 for request 0 the EOS is banned at step 2 and the row runs on
    out, stats = _pool(M, max_new_tokens=N, slots=2, eos_token_id=[EOS, None, None], min_new_tokens=[5, 0, 0], return_info=True, **MIXED)
    assert np.array_equal(out[0, :2].numpy(), ref[0, :2]) and EOS not in out[0, :5].tolist()
    assert stats["n_generated"].tolist()[0] >= 5 and torch.equal(out[1:], plain[1:])


@pytest.mark.parametrize("share_prefix", [False, True], ids=["own-cache", "share-prefix"])
@pytest.mark.parametrize("n", [1, 2])
def test_batch_rows_equal_the_uniform_calls(gpu, n, share_prefix):
    """generate_batch: one value per prompt; with num_return_sequences = n prompt b's value serves its rows b * n .. b * n + n - 1."""
    M = _setup(gpu["device"])
    kw = dict(max_new_tokens=N, num_return_sequences=n, share_prefix=share_prefix)
    uni = [_batch(M, use_graph=False, **kw, **P[b]) for b in range(3)]
    want = torch.cat([uni[b][b * n:(b + 1) * n] for b in range(3)])
    for use_graph in (False, True):
        assert torch.equal(_batch(M, use_graph=use_graph, **kw, **MIXED), want), use_graph
    if n == 2:
        assert torch.equal(want[0], want[1]) and not torch.equal(want[2], want[3])  # greedy twins; sampled rows on their own Philox rows
    out, info = _batch(M, poll_every=2, return_info=True, return_logprobs=True, eos_token_id=[EOS, None, None], **kw, **MIXED)
    assert torch.equal(out[n:], want[n:]) and info["n_generated"].tolist() == [3] * n + [N] * (2 * n)
    o0, i0 = _batch(M, return_info=True, return_logprobs=True, eos_token_id=EOS, **kw, **P[0])
    assert torch.equal(out[:n], o0[:n]) and torch.equal(info["token_logprobs"][:n], i0["token_logprobs"][:n])


def test_scalars_after_lists_are_the_call_of_before(gpu):
    M = _setup(gpu["device"])
    kw = dict(max_new_tokens=[3, 12, 12], slots=2, do_sample=True, seed=5)
    before_pool, before_batch = _pool(M, **kw), _batch(M, max_new_tokens=N, seed=5)
    _pool(M, max_new_tokens=[3, 12, 12], slots=2, **MIXED)
    _batch(M, max_new_tokens=N, **MIXED)
    assert torch.equal(_pool(M, **kw), before_pool) and torch.equal(_batch(M, max_new_tokens=N, seed=5), before_batch)
