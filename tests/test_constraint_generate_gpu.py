"""Constrained decoding through the whole stack, on the tiny generation fixture (3 requests, repeated where a pool needs 12):
(a) a constraint that allows everything changes no token; (b) a trie of three choices of different lengths makes every row one
of the choices, then EOS, then pads; (c) in a pool whose requests follow two different forms (a union, per-request start states)
every request walks its own automaton and gets the tokens generate_batch gives it alone with its form -- the pool's
schedule-independence, now including the state reset at refill; (d) what the entries refuse.  (a) - (c) eager and as a hipGraph."""
import pytest
import torch

from tests.util import load_generation_case

pytestmark = pytest.mark.gpu

PAD, EOS, N = 7, 5, 8
CHOICES = ([11, 12], [20, 21, 22, 23], [30])
OTHER = ([40, 41, 42], [43])
GREEDY = dict(do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0)
SAMPLED = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.9, repetition_penalty=1.2, no_repeat_ngram_size=0, seed=11)
_MODEL = {}


def _setup(dev):
    """The fixture model, built once for the module."""
    if "m" not in _MODEL:
        from tcavt_amd import model
        from tcavt_amd.constraint import TokenConstraint

        fx, cfg, weights, t = load_generation_case()
        m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights, device=dev).eval()
        V = cfg.llama.vocab
        A, B = TokenConstraint.from_sequences(V, CHOICES, EOS), TokenConstraint.from_sequences(V, OTHER, EOS)
        U, starts = TokenConstraint.union([A, B])
        _MODEL.update(m=m, cfg=cfg, g={k: v.to(dev) for k, v in t.items()}, V=V, A=A, B=B, U=U, starts=starts, free=TokenConstraint.free(V))
    return _MODEL


def _done(M, res):
    torch.cuda.synchronize()
    M["m"].mllm.check_flags()
    return (res[0].cpu(), res[1]) if isinstance(res, tuple) else res.cpu()


def _batch(M, rows=slice(None), **kw):
    g = M["g"]
    return _done(M, M["m"].mllm.generate_batch(g["vision_emb"][rows], None, input_ids=g["input_ids"][rows],
                                               attention_mask=g["attention_mask"][rows], pad_token_id=PAD, **kw))


def _pool(M, times=1, **kw):
    g = M["g"]
    vis, ids, mask = (g[k].repeat(times, *[1] * (g[k].dim() - 1)) for k in ("vision_emb", "input_ids", "attention_mask"))
    return _done(M, M["m"].mllm.generate_pool(vis, ids, mask, pad_token_id=PAD, **kw))


def _is_a_choice(row, choices):
    row = row.tolist()
    return any(row == list(c) + [EOS] + [PAD] * (len(row) - len(c) - 1) for c in choices)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("how", ["greedy", "sampled"])
def test_a_free_constraint_changes_no_token(gpu, how, use_graph):
    M = _setup(gpu["device"])
    kw = dict(GREEDY if how == "greedy" else SAMPLED, use_graph=use_graph)
    assert torch.equal(_batch(M, max_new_tokens=N, constraint=M["free"], **kw), _batch(M, max_new_tokens=N, **kw))
    out, info = _batch(M, max_new_tokens=N, constraint=M["free"], return_info=True, return_logprobs=True, **kw)
    want, winfo = _batch(M, max_new_tokens=N, return_info=True, return_logprobs=True, **kw)
    assert torch.equal(out, want) and torch.equal(info["token_logprobs"], winfo["token_logprobs"])
    assert info["constraint_state"].tolist() == [0, 0, 0]
    for G in (1, 2):
        pkw = dict(kw, max_new_tokens=[3, N, N], slots=2, admit_group=G)
        assert torch.equal(_pool(M, constraint=M["free"], **pkw), _pool(M, **pkw)), G


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("how", ["greedy", "sampled"])
def test_a_trie_of_choices_is_all_a_row_can_say(gpu, how, use_graph):
    M = _setup(gpu["device"])
    A = M["A"]
    kw = dict(GREEDY if how == "greedy" else SAMPLED, use_graph=use_graph, max_new_tokens=N, constraint=A, eos_token_id=EOS, return_info=True)
    for extra in (dict(), dict(kv_cache="fp8"), dict(num_return_sequences=4), dict(num_return_sequences=4, share_prefix=True),
                  dict(return_logprobs=True, poll_every=2)):
        out, info = _batch(M, **kw, **extra)
        n = extra.get("num_return_sequences", 1)
        assert tuple(out.shape) == (3 * n, N)
        for r in range(3 * n):
            assert _is_a_choice(out[r], CHOICES), (extra, r, out[r].tolist())
            k = int(info["n_generated"][r])
            assert A.walk(out[r, :k].tolist()) == (A.n_states - 1, k)
        assert (info["finish_reason"] == 1).all() and (info["constraint_state"] == A.n_states - 1).all(), extra
        if "return_logprobs" in extra:  # the scores are those of the raw row: finite, and as many as tokens
            assert torch.equal(info["n_scored"], info["n_generated"]) and torch.isfinite(info["sum_logprob"]).all()


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("G", [1, 4], ids=["admit1", "admit4"])
def test_pool_requests_follow_their_own_forms(gpu, G, use_graph):
    M = _setup(gpu["device"])
    U, starts, forms = M["U"], M["starts"], (M["A"], M["B"])
    R = 12
    form_of = [(r // 3 + r % 3) % 2 for r in range(R)]  # request r is fixture row r % 3; both forms meet every fixture row
    kw = dict(GREEDY, eos_token_id=EOS, return_info=True)
    out, stats = _pool(M, times=4, max_new_tokens=N, slots=4, admit_group=G, use_graph=use_graph, constraint=U,
                       constraint_start=[starts[f] for f in form_of], **kw)
    alone = {}
    for r in range(R):
        f, k = form_of[r], int(stats["n_generated"][r])
        assert _is_a_choice(out[r], (CHOICES, OTHER)[f]), (r, out[r].tolist())
        state, n_ok = U.walk(out[r, :k].tolist(), start=starts[f])
        assert n_ok == k and state == int(stats["constraint_state"][r]) == starts[f] + forms[f].n_states - 1
        if (r % 3, f) not in alone:
            alone[r % 3, f] = _batch(M, rows=slice(r % 3, r % 3 + 1), max_new_tokens=N, use_graph=False, constraint=forms[f], **kw)[0][0]
        assert torch.equal(out[r], alone[r % 3, f]), (r, f)
    assert (stats["finish_reason"] == 1).all() and len(stats["admitted"]) == R


def test_refusals_come_before_any_launch(gpu):
    M = _setup(gpu["device"])
    from tcavt_amd.constraint import TokenConstraint

    A, m = M["A"], M["m"].mllm
    n_bufs = len(m._ws._bufs)
    ok = dict(GREEDY, max_new_tokens=N, constraint=A)
    for bad, match in ((dict(num_beams=2), "num_beams > 1"), (dict(prompt_lookup_num_tokens=2), "prompt_lookup_num_tokens"),
                       (dict(no_repeat_ngram_size=3), "pass 0"), (dict(no_repeat_ngram_size=[0, 2, 0]), "pass 0"),
                       (dict(min_new_tokens=1, eos_token_id=EOS), "min_new_tokens = 0"),
                       (dict(min_new_tokens=[0, 0, 4], eos_token_id=EOS), "min_new_tokens = 0"),
                       (dict(constraint=TokenConstraint.free(M["V"] + 1)), "vocabulary"), (dict(constraint="json"), "TokenConstraint"),
                       (dict(constraint_start=A.n_states), "start state"), (dict(constraint_start=[0, 0]), "2 values for 3 requests"),
                       (dict(constraint_start=[0, -1, 0]), r"constraint_start\[1\]"), (dict(constraint=None, constraint_start=0), "needs a constraint")):
        with pytest.raises(ValueError, match=match):
            _batch(M, **dict(ok, **bad))
        if not {"num_beams", "prompt_lookup_num_tokens"} & set(bad):
            with pytest.raises(ValueError, match=match):
                _pool(M, slots=2, **dict(ok, **bad))
    with pytest.raises(ValueError, match="pass 0"):  # the reference's default of 3 is refused too
        _batch(M, max_new_tokens=N, constraint=A)
    assert len(m._ws._bufs) == n_bufs
