"""generate_batch(prompt_lookup_num_tokens=k) end to end on the tiny generation model (tests/golden/tiny_generation.npz's case): the
tokens are those of the call without the argument.

- Greedy ids with k = 3 and k = 7, eager and graph, equal the fixture's ids (the reference model's own continuation, which the plain
  call is held to): plain arg-max and the reference's processors (penalty 1.2, no-repeat-3-gram).
- Prompts built to repeat themselves (a 2- to 5-id pattern repeated over the 20 prompt positions; chosen on the CPU oracle for
  greedy margins >= 0.2 over the 24 tokens): tokens equal the plain call's, info["steps"] < N - 1, accepted > 0 for every row, and
  drafted / accepted / steps equal what the host loop of prompt_lookup_ref gives for those tokens (poll_every = 1).
- Drafts that never match (all prompt ids distinct, greedy under a repetition penalty of 100: no id ever repeats): nothing is
  drafted, the tokens equal the plain call's and steps equals the plain count N - 1.
- Sampled at the reference's defaults (temperature 0.9, top-k 40, top-p 0.9, penalty 1.2, no-repeat-3-gram) on three seeds: tokens
  equal the plain call's.  The comparator is the plain call itself: test_decode_step_multi_gpu.py measured a row's plain-step
  logits bit-independent of the row count (profiles/generate_prompt_lookup.txt), so the k + 1 times as many rows change nothing.
- decode_weights="fp8" and num_return_sequences=2 once each against their plain counterparts.
- Every refused combination raises ValueError.
"""
import pytest
import torch

import prompt_lookup_ref as R
from tests.util import load_generation_case

pytestmark = pytest.mark.gpu

PATTERNS = [[54, 155, 121, 307], [444, 31, 187, 244, 261], [481, 127]]
_cache = {}


def _setup(dev):
    from tcavt_amd import model

    if "m" not in _cache:
        fx, cfg, weights, t = load_generation_case()
        m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights, device=dev).eval()
        _cache["m"] = (fx, cfg, {k: v.to(dev) for k, v in t.items()}, m)
    return _cache["m"]


def _gen(m, g, ids=None, mask=None, **kw):
    ids = g["input_ids"] if ids is None else ids
    mask = g["attention_mask"] if mask is None else mask
    res = m.mllm.generate_batch(g["vision_emb"], None, input_ids=ids, attention_mask=mask, **kw)
    torch.cuda.synchronize()
    m.mllm.check_flags()
    return res


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("k", [3, 7])
def test_greedy_ids_equal_the_fixture(gpu, k, use_graph):
    fx, cfg, g, m = _setup(gpu["device"])
    N = fx["greedy_tokens"].shape[1]
    for pen, ng, want in ((1.0, 0, "greedy_tokens"), (1.2, 3, "greedy_proc_tokens")):
        out, info = _gen(m, g, max_new_tokens=N, do_sample=False, repetition_penalty=pen, no_repeat_ngram_size=ng, use_graph=use_graph,
                         prompt_lookup_num_tokens=k, return_info=True)
        assert out.dtype == torch.int64 and out.cpu().tolist() == fx[want].tolist(), (k, want, info)
        assert info["n_generated"].tolist() == [N] * 3 and info["finish_reason"].tolist() == [4] * 3
        assert 1 <= info["steps"] <= N - 1 and bool((info["accepted"] <= info["drafted"]).all())


def _simulate(prompt_ids, tokens, k, m_ngram):
    """the host loop on the tokens the call returned -> per row (steps, drafted, accepted)"""
    res = []
    for p, y in zip(prompt_ids, tokens):
        _, log = R.speculative(lambda h, s, y=y: y[s], p, len(y), lambda h, k_: R.draft(h, k_, m_ngram), k)
        res.append((len(log), sum(d for d, _, _ in log), sum(a for _, a, _ in log)))
    return res


@pytest.mark.parametrize("k", [3, 7])
def test_repeating_prompts_take_fewer_steps(gpu, k):
    dev = gpu["device"]
    fx, cfg, g, m = _setup(dev)
    N = 24
    ids = torch.tensor([(p * 20)[:20] for p in PATTERNS], dtype=torch.int64, device=dev)
    mask = torch.ones_like(ids)
    kw = dict(ids=ids, mask=mask, max_new_tokens=N, do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0)
    plain = _gen(m, g, **kw).cpu()
    out, info = _gen(m, g, prompt_lookup_num_tokens=k, poll_every=1, return_info=True, **kw)
    print(f"[prompt lookup] k={k}: steps {info['steps']} of {N - 1}, drafted {info['drafted'].tolist()}, accepted {info['accepted'].tolist()}")
    assert torch.equal(out.cpu(), plain)
    sim = _simulate(ids.tolist(), plain.tolist(), k, 2)
    assert info["drafted"].tolist() == [d for _, d, _ in sim] and info["accepted"].tolist() == [a for _, _, a in sim]
    assert info["steps"] == max(s for s, _, _ in sim)
    assert info["steps"] < N - 1 and bool((info["accepted"] > 0).all())


def test_drafts_that_never_match(gpu):
    dev = gpu["device"]
    fx, cfg, g, m = _setup(dev)
    N, k = 12, 3
    ids = (torch.arange(60, dtype=torch.int64, device=dev).view(3, 20) * 7 + 5) % 512
    mask = torch.ones_like(ids)
    kw = dict(ids=ids, mask=mask, max_new_tokens=N, do_sample=False, repetition_penalty=100.0, no_repeat_ngram_size=0)
    plain, pinfo = _gen(m, g, return_info=True, poll_every=1, **kw)
    for row, y in zip(ids.tolist(), plain.cpu().tolist()):
        assert len(set(row + y)) == len(row + y)  # from the plain call alone: no id repeats, so no n-gram can match
    out, info = _gen(m, g, prompt_lookup_num_tokens=k, poll_every=1, return_info=True, **kw)
    assert torch.equal(out, plain)
    assert info["drafted"].tolist() == [0, 0, 0] and info["accepted"].tolist() == [0, 0, 0]
    assert info["steps"] == pinfo["steps"] == N - 1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sampled_tokens_equal_the_plain_call(gpu, seed):
    dev = gpu["device"]
    fx, cfg, g, m = _setup(dev)
    N, k = 12, 3
    kw = dict(max_new_tokens=N, do_sample=True, seed=seed)  # (the reference's defaults: 0.9 / 40 / 0.9 / 1.2 / 3)
    plain = _gen(m, g, **kw).cpu()
    out, info = _gen(m, g, prompt_lookup_num_tokens=k, return_info=True, **kw)
    assert torch.equal(out.cpu(), plain), (seed, info)


def test_fp8_weights_and_return_sequences(gpu):
    dev = gpu["device"]
    fx, cfg, g, m = _setup(dev)
    N = 12
    kw = dict(max_new_tokens=N, do_sample=False, repetition_penalty=1.2, no_repeat_ngram_size=3, decode_weights="fp8")
    plain = _gen(m, g, **kw)
    out, info = _gen(m, g, prompt_lookup_num_tokens=3, return_info=True, **kw)
    assert torch.equal(out, plain), info
    kw = dict(max_new_tokens=N, do_sample=True, seed=11, num_return_sequences=2)
    plain = _gen(m, g, **kw)
    out, info = _gen(m, g, prompt_lookup_num_tokens=3, return_info=True, **kw)
    assert tuple(out.shape) == (6, N) and torch.equal(out, plain), info
    assert info["drafted"].shape == (6,) and not torch.equal(out[0], out[1])  # (the two continuations of a prompt do differ)


BAD = [dict(kv_cache="fp8"), dict(share_prefix=True), dict(num_beams=2, do_sample=False), dict(return_logprobs=True),
       dict(stop_sequences=[[1, 2]]), dict(num_return_sequences=3), dict(prompt_lookup_num_tokens=8), dict(prompt_lookup_num_tokens=0),
       dict(max_matching_ngram_size=9), dict(pad_token_id=512)]


def test_refused_combinations_raise(gpu):
    fx, cfg, g, m = _setup(gpu["device"])
    for kw in BAD:
        with pytest.raises(ValueError):
            _gen(m, g, **dict(dict(max_new_tokens=4, prompt_lookup_num_tokens=3), **kw))
