"""top_logprobs through generate_batch and generate_pool on the tiny generation fixture: what return_logprobs returns is unchanged
bit for bit; under plain greedy decoding the first entry of every list is the emitted token with the bits of token_logprobs;
every list is sorted by (log-probability descending, id ascending) and every entry lies within the project's pinned per-step bar
(2 * 2e-3 * ||logits||_2, as in tests/test_beam_generate_gpu.py) of the oracle's float64 log-softmax after the same prefix;
positions a request never generated hold -1 / -inf; eager and graph agree; a pooled request gets the bits generate_batch gives it;
with a constraint the lists stay those of the raw row.  The model, the oracle rows and the helpers are those of
tests/test_logprob_generate_gpu.py (computed once, shared)."""
import numpy as np
import pytest
import torch

from tests import topk_ref as TR
from tests.test_logprob_generate_gpu import GREEDY, REQS, _batch, _oracle_row, _pool, _setup

pytestmark = pytest.mark.gpu

K = 5
KEYS = ("token_logprobs", "sum_logprob", "n_scored")
TOP = ("top_token_ids", "top_token_logprobs")


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


def _check_lists(M, rows, out, info, n_gen, k, oracle=True):
    """rows[i]: the fixture row behind result row i.  Generated positions: valid distinct ids, sorted lists, every entry within the
    bar of the oracle; the rest -1 / -inf.  -> worst error in units of the bar."""
    ids, lps = info["top_token_ids"].numpy(), info["top_token_logprobs"].numpy()
    out = out.cpu().numpy()
    V = M["cfg"].llama.vocab
    assert ids.dtype == np.int64 and lps.dtype == np.float32 and ids.shape == lps.shape == out.shape + (k,)
    worst = 0.0
    for i, b in enumerate(rows):
        n = int(n_gen[i])
        assert bool((ids[i, n:] == -1).all()) and bool(np.isneginf(lps[i, n:]).all()), f"row {i}: written after its end"
        for s in range(n):
            assert bool(((ids[i, s] >= 0) & (ids[i, s] < V)).all()) and len(set(ids[i, s].tolist())) == k
            assert TR.is_sorted(ids[i, s], lps[i, s]), (i, s, ids[i, s], lps[i, s])
            assert bool((lps[i, s] <= 0).all())
            if not oracle:
                continue
            ref_row = _oracle_row(M, b, out[i, :s])
            x64 = ref_row.astype(np.float64)
            lse = x64.max() + np.log(np.exp(x64 - x64.max()).sum())
            bound = 2 * 2e-3 * float(np.linalg.norm(x64))
            for j in range(k):
                err = abs(float(lps[i, s, j]) - float(x64[ids[i, s, j]] - lse))
                print(f"[top_logprobs] row {i} step {s} entry {j}: id {ids[i, s, j]} err {err:.3e} bound {bound:.3e}")
                worst = max(worst, err / bound)
                assert err <= bound, (i, s, j, err, bound)
    return worst


def test_what_return_logprobs_returns_is_unchanged(gpu):
    M = _setup(gpu["device"])
    cases = [dict(GREEDY, max_new_tokens=6), dict(do_sample=True, seed=5, max_new_tokens=6),
             dict(do_sample=True, seed=9, max_new_tokens=5, num_return_sequences=2, share_prefix=True)]
    for kw in cases:
        out0, info0 = _batch(M, return_logprobs=True, **kw)
        out0 = out0.clone()
        out1, info1 = _batch(M, return_logprobs=True, top_logprobs=K, **kw)
        assert torch.equal(out1, out0), kw
        for key in KEYS:
            assert _same(info1[key], info0[key]), (kw, key)
        assert all(t not in info0 for t in TOP)
        rows, N = out0.shape
        assert tuple(info1["top_token_ids"].shape) == (rows, N, K) and info1["top_token_ids"].dtype == torch.int64
        assert tuple(info1["top_token_logprobs"].shape) == (rows, N, K) and info1["top_token_logprobs"].dtype == torch.float32
        n = kw.get("num_return_sequences", 1)
        _check_lists(M, [b for b in range(3) for _ in range(n)], out1, info1, info1["n_scored"], K, oracle=False)
        # the emitted token's entry, wherever it is listed, has the bits of token_logprobs
        ids, lps, tlp = info1["top_token_ids"], info1["top_token_logprobs"], info1["token_logprobs"]
        hit = ids == out1.cpu()[..., None]
        assert bool(hit.any())
        assert torch.equal(lps[hit].view(torch.int32), tlp[..., None].expand_as(lps)[hit].view(torch.int32))
    M["m"].mllm.check_flags()


def test_greedy_lists_lead_with_the_emitted_token_and_match_the_oracle(gpu):
    M = _setup(gpu["device"])
    out, info = _batch(M, max_new_tokens=7, return_logprobs=True, return_info=True, top_logprobs=K, **GREEDY)
    assert np.array_equal(out.cpu().numpy(), M["fx"]["greedy_tokens"][:, :7])
    assert info["n_generated"].tolist() == [7, 7, 7]
    assert torch.equal(info["top_token_ids"][..., 0], out.cpu())
    assert torch.equal(info["top_token_logprobs"][..., 0].view(torch.int32), info["token_logprobs"].view(torch.int32))
    worst = _check_lists(M, [0, 1, 2], out, info, info["n_generated"], K)
    print(f"\n[top_logprobs] generate_batch against the oracle: worst {worst:.3f} of 2 * 2e-3 * ||logits||")
    # eager and graph give the same bits; k = 1 and k = 20 are prefixes / extensions of the same order
    out2, info2 = _batch(M, max_new_tokens=7, return_logprobs=True, top_logprobs=K, use_graph=False, **GREEDY)
    for key in KEYS + TOP:
        assert _same(info2[key], info[key]), key
    for k in (1, 20):
        _, ik = _batch(M, max_new_tokens=7, return_logprobs=True, top_logprobs=k, **GREEDY)
        m = min(k, K)
        assert torch.equal(ik["top_token_ids"][..., :m], info["top_token_ids"][..., :m])
        assert _same(ik["top_token_logprobs"][..., :m].contiguous(), info["top_token_logprobs"][..., :m].contiguous())
        _check_lists(M, [0, 1, 2], out, ik, [7, 7, 7], k, oracle=False)


def test_positions_beyond_the_end_keep_the_initial_values(gpu):
    M = _setup(gpu["device"])
    ref = _batch(M, max_new_tokens=10, **GREEDY).cpu()
    eos = int(ref[0, 2])  # an id of the fixture's own continuation: row 0 ends with its third token
    first = [int((ref[b] == eos).nonzero()[0]) + 1 if bool((ref[b] == eos).any()) else 10 for b in range(3)]
    assert first[0] == 3
    _, full = _batch(M, max_new_tokens=10, return_logprobs=True, top_logprobs=K, **GREEDY)
    for use_graph in (True, False):
        out, info = _batch(M, max_new_tokens=10, eos_token_id=eos, pad_token_id=7, return_logprobs=True, return_info=True,
                           top_logprobs=K, use_graph=use_graph, **GREEDY)
        assert info["n_generated"].tolist() == first == info["n_scored"].tolist()
        _check_lists(M, [0, 1, 2], out, info, first, K, oracle=False)
        for b in range(3):  # the ending token's position included: the bits of the run that does not end
            for key in TOP:
                assert _same(info[key][b, :first[b]].contiguous(), full[key][b, :first[b]].contiguous()), (b, key)


@pytest.mark.parametrize("G", (1, 2))
def test_pool_returns_per_request_the_bits_of_generate_batch(gpu, G):
    M = _setup(gpu["device"])
    budgets = [7, 3, 7, 5, 2]
    out_b, info_b = _batch(M, max_new_tokens=7, return_logprobs=True, top_logprobs=K, **GREEDY)
    out_b = out_b.cpu().clone()
    out, stats = _pool(M, max_new_tokens=budgets, slots=2, admit_group=G, return_logprobs=True, return_info=True, top_logprobs=K, **GREEDY)
    assert stats["n_generated"].tolist() == budgets == stats["n_scored"].tolist()
    _check_lists(M, REQS, out, stats, budgets, K, oracle=False)
    for r, (b, n) in enumerate(zip(REQS, budgets)):
        assert torch.equal(out[r, :n].cpu(), out_b[b, :n]), (r, b)
        for key, key_b in zip(TOP + ("token_logprobs",), TOP + ("token_logprobs",)):
            got, exp = stats[key][r, :n].contiguous(), info_b[key_b][b, :n].contiguous()
            diff = (got.double() - exp.double()).abs().max().item() if got.dtype.is_floating_point else int((got != exp).sum())
            print(f"[top_logprobs] pool G = {G} request {r} (row {b}) {key}: max difference to generate_batch {diff}")
            assert _same(got, exp), (G, r, key)
    # ... and independent of the slot count
    out3, stats3 = _pool(M, max_new_tokens=budgets, slots=3, admit_group=G, return_logprobs=True, top_logprobs=K, **GREEDY)
    for key in KEYS + TOP:
        assert _same(stats3[key], stats[key]), ("slots", key)
    M["m"].mllm.check_flags()


def test_with_a_constraint_the_lists_are_those_of_the_raw_row(gpu):
    from tcavt_amd.constraint import TokenConstraint

    M = _setup(gpu["device"])
    V = M["cfg"].llama.vocab
    out0, info0 = _batch(M, max_new_tokens=3, return_logprobs=True, top_logprobs=K, **GREEDY)
    raw_best = info0["top_token_ids"][:, 0, 0].tolist()
    allowed = sorted(set(range(V)) - set(raw_best))[:50]  # every row's raw arg-max is banned
    con = TokenConstraint.from_allowed_tokens(V, allowed)
    for use_graph in (True, False):
        out, info = _batch(M, max_new_tokens=3, return_logprobs=True, top_logprobs=K, constraint=con, use_graph=use_graph, **GREEDY)
        assert bool(torch.isin(out.cpu(), torch.tensor(allowed)).all())
        for key in TOP:  # step 0 has the same prefix: the same raw row, the same list
            assert _same(info[key][:, 0].contiguous(), info0[key][:, 0].contiguous()), key
        assert info["top_token_ids"][:, 0, 0].tolist() == raw_best  # a banned id leads the list
        assert all(int(out[b, 0]) != raw_best[b] for b in range(3))
        _check_lists(M, [0, 1, 2], out, info, [3, 3, 3], K, oracle=False)
    outp, statsp = _pool(M, order=[0, 1, 2], max_new_tokens=3, slots=2, return_logprobs=True, top_logprobs=K, constraint=con, **GREEDY)
    assert statsp["top_token_ids"][:, 0, 0].tolist() == raw_best
    M["m"].mllm.check_flags()


def test_flags_are_clean_and_a_default_call_is_the_fixtures(gpu):
    M = _setup(gpu["device"])
    g, fx = M["g"], M["fx"]
    _batch(M, max_new_tokens=4, return_logprobs=True, top_logprobs=20, do_sample=True, seed=3)
    M["m"].mllm.check_flags()
    N = fx["greedy_tokens"].shape[1]
    out = M["m"].mllm.generate_batch(g["vision_emb"], None, max_new_tokens=N, input_ids=g["input_ids"], attention_mask=g["attention_mask"],
                                     **GREEDY)
    torch.cuda.synchronize()
    M["m"].mllm.check_flags()
    assert torch.is_tensor(out) and np.array_equal(out.cpu().numpy(), fx["greedy_tokens"])


def test_illegal_calls_raise_before_any_launch(gpu):
    M = _setup(gpu["device"])
    ws = M["m"].mllm._ws
    n_bufs = len(ws._bufs)
    with pytest.raises(ValueError, match="top_logprobs needs return_logprobs=True"):
        _batch(M, max_new_tokens=3, top_logprobs=5, **GREEDY)
    with pytest.raises(ValueError, match="top_logprobs needs return_logprobs=True"):
        _pool(M, max_new_tokens=3, slots=2, top_logprobs=5, **GREEDY)
    for bad in (0, 21, True, 2.5):
        with pytest.raises(ValueError, match="top_logprobs must be None or an int"):
            _batch(M, max_new_tokens=3, return_logprobs=True, top_logprobs=bad, **GREEDY)
        with pytest.raises(ValueError, match="top_logprobs must be None or an int"):
            _pool(M, max_new_tokens=3, slots=2, return_logprobs=True, top_logprobs=bad, **GREEDY)
    with pytest.raises(ValueError, match="num_beams > 1"):
        _batch(M, max_new_tokens=3, return_logprobs=True, top_logprobs=5, num_beams=2, **GREEDY)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        _batch(M, max_new_tokens=3, return_logprobs=True, top_logprobs=5, prompt_lookup_num_tokens=2, **GREEDY)
    assert len(ws._bufs) == n_bufs  # nothing was requested, so nothing was launched
