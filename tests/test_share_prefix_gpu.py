"""generate_batch(num_return_sequences=3, share_prefix=True) on the tiny generation fixture: the decode rows read their prompt's
cache in place (tcavt_attn_decode_shared through tcavt_llama_decode_step_shared) and own a suffix cache of N - 1 rows.  Greedy rows
against the reference model's continuation (tests/golden/tiny_generation.npz), sampling (seed, graph, first column), ending
rules, polling, what the call leaves in the workspace and for the next call.  The model and the call helper are those of
tests/test_nsamples_gpu.py."""
import numpy as np
import pytest
import torch

from tests.stop_util import cut_row
from test_nsamples_gpu import NSEQ, SEED, _batch, _setup

pytestmark = pytest.mark.gpu
SHARED = dict(num_return_sequences=NSEQ, share_prefix=True)


@pytest.mark.parametrize("use_graph", [False, True])
def test_greedy_rows_are_the_reference_continuation_three_times(gpu, use_graph):
    M = _setup(gpu["device"])
    fx = M["fx"]
    N = fx["greedy_tokens"].shape[1]
    kw = dict(max_new_tokens=N, do_sample=False, use_graph=use_graph)
    out = _batch(M, repetition_penalty=1.0, no_repeat_ngram_size=0, **kw, **SHARED).cpu().numpy()
    assert out.dtype == np.int64 and out.shape == (3 * NSEQ, N)
    assert np.array_equal(out, np.repeat(fx["greedy_tokens"], NSEQ, axis=0))
    out2 = _batch(M, repetition_penalty=1.2, no_repeat_ngram_size=3, **kw, **SHARED).cpu().numpy()
    assert np.array_equal(out2, np.repeat(fx["greedy_proc_tokens"], NSEQ, axis=0))
    # n = 1 is legal: the prompts' own rows on the shared path
    one = _batch(M, repetition_penalty=1.0, no_repeat_ngram_size=0, share_prefix=True, **kw).cpu().numpy()
    assert np.array_equal(one, fx["greedy_tokens"])


def test_sampling_is_a_function_of_the_seed_and_starts_from_the_prefill_logits(gpu):
    M = _setup(gpu["device"])
    vocab, N = M["cfg"].llama.vocab, 10
    kw = dict(max_new_tokens=N, do_sample=True, **SHARED)
    a = _batch(M, seed=SEED, **kw).cpu()
    b = _batch(M, seed=SEED, **kw).cpu()
    e = _batch(M, seed=SEED, use_graph=False, **kw).cpu()
    c = _batch(M, seed=SEED + 1, **kw).cpu()
    assert tuple(a.shape) == (3 * NSEQ, N) and bool(((a >= 0) & (a < vocab)).all())
    assert torch.equal(a, b) and torch.equal(a, e) and not torch.equal(a, c)  # two runs equal, eager == graph, another seed differs
    unshared = _batch(M, max_new_tokens=N, do_sample=True, seed=SEED, num_return_sequences=NSEQ).cpu()
    assert torch.equal(a[:, 0], unshared[:, 0])  # the first token comes from the prefill's logits and Philox row r on both paths
    print("rows equal to the unshared call's:", int((a == unshared).all(1).sum()), "of", 3 * NSEQ)


def test_rules_cut_the_unruled_run_and_polling_returns_the_same_tokens(gpu):
    from tests.test_stop_rules_gpu import PAD, _rules_from

    M = _setup(gpu["device"])
    vocab, N = M["cfg"].llama.vocab, 16
    kw = dict(max_new_tokens=N, do_sample=True, seed=SEED, pad_token_id=PAD, **SHARED)
    plain = _batch(M, **kw).cpu()
    rows = plain.tolist()
    rules = _rules_from(rows, vocab, 0, 5, 4, 7)  # row 0's step-5 token as a stop token, row 4's steps 7 .. 9 as a sequence
    want = [cut_row(rules, r, None, PAD) for r in rows]
    reasons = [w[2] for w in want]
    assert 2 in reasons and 3 in reasons, reasons  # (a condition on the input: both rules fire somewhere)
    rk = dict(stop_token_ids=rules.stop_token_ids, stop_sequences=rules.stop_sequences, return_info=True)
    for use_graph, poll in ((True, None), (True, 2), (False, 2)):
        out, info = _batch(M, use_graph=use_graph, poll_every=poll, **kw, **rk)
        assert out.cpu().tolist() == [w[0] for w in want], (use_graph, poll)
        assert info["finish_reason"].shape == info["n_generated"].shape == (3 * NSEQ,)
        assert info["finish_reason"].tolist() == reasons and info["n_generated"].tolist() == [w[1] for w in want]
    assert torch.equal(_batch(M, poll_every=2, **kw).cpu(), plain)  # unruled: polled == unpolled


def test_the_prompt_cache_is_the_prefills_and_the_suffix_cache_has_n_minus_one_rows(gpu):
    dev = gpu["device"]
    M = _setup(dev)
    mm, ll, t = M["m"].mllm, M["cfg"].llama, M["t"]
    Lt, N = t["input_ids"].shape[1], 4
    L, w = 16 + Lt, ll.n_kv_heads * ll.head_dim
    st = mm.llama_wrapper.storage
    src = lambda nm: mm._ws.get(f"gen.src.{nm}", (ll.layers, 3, L, w), st, dev).view(torch.int16).cpu().clone()
    _batch(M, max_new_tokens=N, num_return_sequences=NSEQ, do_sample=True, seed=SEED)
    want = {nm: src(nm) for nm in ("kc", "vc")}
    for nm in ("kc", "vc"):  # a value the shared call has to overwrite, so that equality below is the call's doing
        mm._ws.get(f"gen.src.{nm}", (ll.layers, 3, L, w), st, dev).fill_(7.0)
    _batch(M, max_new_tokens=N, do_sample=True, seed=SEED, **SHARED)
    for nm in ("kc", "vc"):
        got = src(nm)
        for b in range(3):  # the prompt's valid rows (the rows behind them are the prefill's pad rows, which nothing reads)
            kvl = 16 + int(t["attention_mask"][b].sum())
            assert bool(want[nm][:, b, :kvl].any()), nm
            assert torch.equal(got[:, b, :kvl], want[nm][:, b, :kvl]), f"gen.src.{nm} of prompt {b} differs from the unshared call's prefill"
    for nm in ("gen.sfx.kc", "gen.sfx.vc"):  # (the workspace is keyed by name, shape and type)
        assert (nm, (ll.layers, 3 * NSEQ, N - 1, w), st) in mm._ws._bufs


def test_a_shared_call_leaves_nothing_behind(gpu):
    M = _setup(gpu["device"])
    fx = M["fx"]
    N = fx["greedy_tokens"].shape[1]
    greedy = dict(max_new_tokens=N, do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0)
    _batch(M, max_new_tokens=N, do_sample=True, seed=3, **SHARED)
    assert np.array_equal(_batch(M, **greedy).cpu().numpy(), fx["greedy_tokens"])
    # FP8 weights at B * n = 9 rows: bit-reproducible, flags clean (_batch checks them)
    w8 = dict(max_new_tokens=N, do_sample=True, seed=3, decode_weights="fp8", **SHARED)
    x = _batch(M, **w8).cpu()
    y = _batch(M, **w8).cpu()
    assert tuple(x.shape) == (3 * NSEQ, N) and torch.equal(x, y)
