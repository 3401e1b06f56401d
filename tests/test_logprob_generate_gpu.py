"""return_logprobs through generate_batch and generate_pool on the tiny generation fixture: the tokens are those of the call
without the flag, bit for bit; at the three call sites (prefill logits, eager step, graph replay) the score equals the float64
reference on the very logits row the step produced, within the kernels' bar; every score is within twice the project's pinned
logits bar of the float64 log-softmax of the oracle's row (a log-softmax moves by at most twice the largest logit error);
sum_logprob is the fp32 running sum; n_scored equals n_generated; the ending token is scored and nothing after it; a pooled
request's three results do not depend on its slot, the number of slots or the order of the request list."""
import numpy as np
import pytest
import torch

from tests import logprob_ref as LR
from tests.util import load_generation_case

pytestmark = pytest.mark.gpu

_MODEL = {}
_ORACLE = {}
GREEDY = dict(do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0)
REQS = [0, 1, 2, 1, 0]  # the pool's request list: rows of the fixture


def _setup(dev):
    if "m" not in _MODEL:
        from tcavt_amd import model

        fx, cfg, weights, t = load_generation_case()
        m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights, device=dev).eval()
        _MODEL.update(m=m, fx=fx, cfg=cfg, weights=weights, t=t, g={k: v.to(dev) for k, v in t.items()})
    return _MODEL


def _batch(M, **kw):
    g = M["g"]
    res = M["m"].mllm.generate_batch(g["vision_emb"], None, input_ids=g["input_ids"], attention_mask=g["attention_mask"], **kw)
    torch.cuda.synchronize()
    return res


def _pool(M, order=REQS, **kw):
    g, idx = M["g"], torch.tensor(order)
    res = M["m"].mllm.generate_pool(g["vision_emb"][idx], g["input_ids"][idx], g["attention_mask"][idx], **kw)
    torch.cuda.synchronize()
    return res


def _oracle_row(M, b, prefix):
    """fp32 logits [V] of the oracle (fp16 contract) after fixture row b's prompt and the generated tokens ``prefix``."""
    key = (b, tuple(int(x) for x in prefix))
    if key not in _ORACLE:
        from oracle import generation as G

        w, cfg, t = M["weights"], M["cfg"], M["t"]
        seq = G.prefix_embeds(w, cfg, t["vision_emb"], t["input_ids"], "fp16", b, int(t["attention_mask"][b].sum()))
        for tok in prefix:
            seq = torch.cat([seq, G.token_embed(w, torch.as_tensor(tok), "fp16")[None, None]], dim=1)
        with torch.no_grad():
            _ORACLE[key] = G.next_logits(w, cfg, seq, "fp16").float().numpy()
    return _ORACLE[key]


def _check_against_oracle(M, rows, out, info, n_gen):
    """rows[i]: the fixture row behind result row i.  Every scored entry within 2 * 2e-3 * ||oracle logits||_2 of the float64
    log-softmax of the oracle's row; the rest exactly 0; sum_logprob the fp32 running sum; n_scored = n_gen."""
    tlp, tot, cnt = (info[k].numpy() for k in ("token_logprobs", "sum_logprob", "n_scored"))
    out = out.cpu().numpy()
    worst = 0.0
    for i, b in enumerate(rows):
        n = int(n_gen[i])
        assert cnt[i] == n
        run = np.float32(0.0)
        for k in range(n):
            ref_row = _oracle_row(M, b, out[i, :k])
            bound = 2 * 2e-3 * float(np.linalg.norm(ref_row.astype(np.float64)))
            err = abs(float(tlp[i, k]) - LR.ref_logprob(ref_row, out[i, k]))
            worst = max(worst, err / bound)
            assert err <= bound, (i, k, err, bound)
            assert tlp[i, k] <= 0
            run = np.float32(run + tlp[i, k])
        assert not tlp[i, n:].any()
        assert tot[i].tobytes() == run.tobytes()
    return worst


def test_tokens_are_those_of_the_call_without_the_flag(gpu):
    M = _setup(gpu["device"])
    cases = [dict(GREEDY, max_new_tokens=8), dict(GREEDY, max_new_tokens=8, use_graph=False),
             dict(do_sample=True, seed=5, max_new_tokens=8), dict(do_sample=True, seed=5, max_new_tokens=8, use_graph=False),
             dict(do_sample=True, seed=9, max_new_tokens=6, num_return_sequences=3),
             dict(do_sample=True, seed=9, max_new_tokens=6, num_return_sequences=3, share_prefix=True),
             dict(do_sample=False, max_new_tokens=6, stop_token_ids=[309], min_new_tokens=2, poll_every=2)]
    for kw in cases:
        plain = _batch(M, **kw).clone()
        out, info = _batch(M, return_logprobs=True, **kw)
        assert torch.equal(out, plain), kw
        rows = plain.shape[0]
        assert tuple(info["token_logprobs"].shape) == tuple(plain.shape) and info["token_logprobs"].dtype == torch.float32
        assert tuple(info["sum_logprob"].shape) == (rows,) and info["n_scored"].dtype == torch.int32
        assert bool((info["n_scored"] >= 1).all()) and bool((info["token_logprobs"] <= 0).all())
    for G in (1, 2):
        for kw in (dict(GREEDY), dict(do_sample=True, seed=5)):
            kw = dict(kw, max_new_tokens=[5, 2, 6, 1, 4], slots=3, admit_group=G)
            plain = _pool(M, **kw).clone()
            out, stats = _pool(M, return_logprobs=True, **kw)
            assert torch.equal(out, plain), (G, kw)
            assert stats["n_scored"].tolist() == [5, 2, 6, 1, 4]
    M["m"].mllm.check_flags()


@pytest.mark.parametrize("N", (1, 2, 4))
def test_score_equals_the_reference_on_the_steps_own_logits(gpu, N):
    """greedy, penalty 1.0, no ban: the selection leaves the logits row as the lm_head wrote it, so the workspace still holds
    the raw row of the last step -- N = 1 the prefill's, 2 the eager step's, 4 a graph replay's."""
    M = _setup(gpu["device"])
    out, info = _batch(M, max_new_tokens=N, return_logprobs=True, **GREEDY)
    B, V = out.shape[0], M["cfg"].llama.vocab
    logits = M["m"].mllm._ws.get("gen.logits", (B, V), torch.float32, gpu["device"]).cpu().numpy()
    worst = 0.0
    for b in range(B):
        tok = int(out[b, N - 1])
        assert tok == int(np.argmax(logits[b]))  # (the row is unmodified: the token is its plain arg-max)
        r = LR.ratio(info["token_logprobs"][b, N - 1].item(), LR.ref_logprob(logits[b], tok))
        worst = max(worst, r)
        assert r <= 1.0, (b, r)
    assert info["n_scored"].tolist() == [N] * B
    print(f"\n[logprob] call site N = {N}: worst {worst:.3f} of the bar")


def test_scores_match_the_oracle_on_the_growing_sequence(gpu):
    M = _setup(gpu["device"])
    (out, info) = _batch(M, max_new_tokens=7, return_logprobs=True, return_info=True, **GREEDY)
    assert np.array_equal(out.cpu().numpy(), M["fx"]["greedy_tokens"][:, :7])
    assert torch.equal(info["n_scored"], info["n_generated"]) and info["n_scored"].tolist() == [7, 7, 7]
    worst = _check_against_oracle(M, [0, 1, 2], out, info, info["n_generated"])
    print(f"\n[logprob] generate_batch against the oracle: worst {worst:.3f} of 2 * 2e-3 * ||logits||")
    # eager and graph give the same bits
    (out2, info2) = _batch(M, max_new_tokens=7, return_logprobs=True, use_graph=False, **GREEDY)
    for k in ("token_logprobs", "sum_logprob", "n_scored"):
        assert torch.equal(info[k], info2[k]), k


def test_ending_token_is_scored_and_nothing_after_it(gpu):
    M = _setup(gpu["device"])
    ref = _batch(M, max_new_tokens=10, **GREEDY).cpu()
    eos = int(ref[0, 2])
    first = [int((ref[b] == eos).nonzero()[0]) + 1 if bool((ref[b] == eos).any()) else 10 for b in range(3)]
    assert first[0] == 3
    full = _batch(M, max_new_tokens=10, return_logprobs=True, **GREEDY)[1]
    for use_graph in (True, False):
        out, info = _batch(M, max_new_tokens=10, eos_token_id=eos, pad_token_id=7, return_logprobs=True, return_info=True,
                           use_graph=use_graph, **GREEDY)
        assert info["n_scored"].tolist() == first == info["n_generated"].tolist()
        tlp = info["token_logprobs"]
        for b in range(3):
            assert bool((tlp[b, :first[b]] <= 0).all()) and not bool(tlp[b, first[b]:].any())
            assert torch.equal(tlp[b, :first[b]], full["token_logprobs"][b, :first[b]])  # the ending token included, same bits
        assert int(out[0, 2]) == eos and bool((out[0, 3:] == 7).all())


@pytest.mark.parametrize("G", (1, 2))
def test_pool_results_follow_the_request(gpu, G):
    M = _setup(gpu["device"])
    budgets = [7, 3, 7, 5, 2]
    kw = dict(GREEDY, admit_group=G, return_logprobs=True, return_info=True)
    out, stats = _pool(M, max_new_tokens=budgets, slots=2, **kw)
    assert stats["n_scored"].tolist() == budgets == stats["n_generated"].tolist()
    worst = _check_against_oracle(M, REQS, out, stats, stats["n_generated"])
    print(f"\n[logprob] generate_pool G = {G} against the oracle: worst {worst:.3f} of 2 * 2e-3 * ||logits||")
    out3, stats3 = _pool(M, max_new_tokens=budgets, slots=3, **kw)
    perm = [3, 0, 4, 2, 1]
    outp, statsp = _pool(M, order=[REQS[i] for i in perm], max_new_tokens=[budgets[i] for i in perm], slots=2, **kw)
    assert torch.equal(out3, out) and torch.equal(outp, out[torch.tensor(perm)])
    for k in ("token_logprobs", "sum_logprob", "n_scored"):
        assert torch.equal(stats3[k], stats[k]), ("slots", k)
        assert torch.equal(statsp[k], stats[k][torch.tensor(perm)]), ("order", k)
    # the sampling path too: Philox follows the request's row, so only the slot count is varied
    kw = dict(do_sample=True, seed=3, admit_group=G, return_logprobs=True)
    a, sa = _pool(M, max_new_tokens=budgets, slots=2, **kw)
    b, sb = _pool(M, max_new_tokens=budgets, slots=3, **kw)
    assert torch.equal(a, b)
    for k in ("token_logprobs", "sum_logprob", "n_scored"):
        assert torch.equal(sa[k], sb[k]), ("sampling", k)
    M["m"].mllm.check_flags()
