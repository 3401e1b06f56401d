"""constraint.TokenConstraint on the host -- no GPU: the builders, walk / allowed (the host statement of the rule the kernels are
held to), union's state ranges, every validation error, the refusals of the generate entries (through the stub library
tests/generation_stub.py: nothing is called, no workspace buffer requested), and the condition under which
tests/test_constraint_sampler_gpu.py may use sampler_ref's decision rule: on its allowed sets the reference alone stays under
sampler_ref.UNDECIDED_CAP."""
import numpy as np
import pytest
import torch

import generation_stub as GS

from tests import constraint_ref as CR
from tests import sampler_ref as SR

from tcavt_amd import constraint as TC
from tcavt_amd.constraint import TokenConstraint

V = 100
I32 = torch.int32


# ---- builders and the rule
def test_allowed_and_suppressed_tokens_are_complements():
    ids = [3, 4, 99, 0]
    A, S = TokenConstraint.from_allowed_tokens(V, ids), TokenConstraint.from_suppressed_tokens(V, ids)
    assert A.n_states == S.n_states == 1 and A.start == S.start == 0
    assert A.allowed(0) == sorted(ids) and S.allowed(0) == [t for t in range(V) if t not in ids]
    assert A.walk([3, 3, 99, 0]) == (0, 4) and A.walk([3, 5, 3]) == (0, 1) and S.walk([5, 6, 3]) == (0, 2)
    assert A.next(0, 3) == 0 and A.next(0, 5) == -1 and A.next(0, V) == -1 and A.next(0, -1) == -1
    F = TokenConstraint.free(V)
    assert F.allowed(0) == list(range(V)) and F.walk(list(range(V))) == (0, V)


def test_from_sequences_is_a_trie_with_a_looping_terminal_state():
    seqs, end = [[11, 12], [20, 21, 22, 23], [30], [11, 12, 13]], 5
    C = TokenConstraint.from_sequences(V, seqs, end)
    term = C.n_states - 1
    assert C.n_states == 1 + 3 + 4 + 1 + 1 and C.start == 0  # root, 11-12-13, 20-21-22-23, 30, terminal
    assert C.allowed(0) == [11, 20, 30] and C.allowed(term) == [end] and C.next(term, end) == term
    for s in seqs:
        assert C.walk(s + [end]) == (term, len(s) + 1) and C.walk(s + [end, end, end]) == (term, len(s) + 3)
        assert C.walk(s + [end, s[0]])[1] == len(s) + 1  # nothing but the end token behind the end token
    state, n = C.walk([11, 12])
    assert n == 2 and C.allowed(state) == [end, 13]  # a choice that is a prefix of another: end it, or go on
    assert C.walk([20, 21, end])[1] == 2 and C.walk([12])[1] == 0 and C.walk([]) == (0, 0)
    # every string of allowed tokens ends in the terminal state after one of the sequences
    outs = set()

    def grow(state, toks):
        if state == term:
            outs.add(tuple(toks[:-1]))
            return
        for t in C.allowed(state):
            grow(C.next(state, t), toks + [t])

    grow(0, [])
    assert outs == {tuple(s) for s in seqs}


def test_union_keeps_the_members_apart():
    A = TokenConstraint.from_sequences(V, [[11, 12], [30]], 5)
    B = TokenConstraint.from_allowed_tokens(V, [1, 2, 11])
    C = TokenConstraint.from_sequences(V, [[11, 40, 41]], 6)
    U, starts = TokenConstraint.union([A, B, C])
    assert U.n_states == A.n_states + B.n_states + C.n_states and U.start == starts[0]
    assert starts == [0, A.n_states, A.n_states + B.n_states]
    for M, base in zip((A, B, C), starts):
        for s in range(M.n_states):
            assert U.allowed(base + s) == M.allowed(s)
            for t in M.allowed(s):
                assert U.next(base + s, t) == base + M.next(s, t)  # a member never leaves its own state range
    assert U.walk([11, 12, 5], start=starts[0]) == (starts[0] + A.n_states - 1, 3)
    assert U.walk([11, 12, 5], start=starts[1]) == (starts[1], 1)
    assert U.walk([11, 40, 41, 6, 6], start=starts[2]) == (starts[2] + C.n_states - 1, 5)
    assert U.n_classes <= 10  # distinct tuples of member classes, not their product


def test_starts_are_request_major():
    C = TokenConstraint.from_sequences(V, [[11, 12], [30]], 5)
    assert C.starts("w", None, 3).tolist() == [0, 0, 0] and C.starts("w", 2, 2).tolist() == [2, 2]
    for v in ([1, 0, 2], (1, 0, 2), torch.tensor([1, 0, 2])):
        s = C.starts("w", v, 3, repeat=2)
        assert s.dtype == I32 and s.tolist() == [1, 1, 0, 0, 2, 2]
    assert C.starts("w", torch.tensor(1), 2).tolist() == [1, 1]
    for bad, match in (([0, 1], "2 values for 3 requests"), ([0, C.n_states, 0], r"constraint_start\[1\]"), ([0, 0, -1], r"constraint_start\[2\]"),
                       ([0, 1.5, 0], r"constraint_start\[1\]"), ([0, True, 0], r"constraint_start\[1\]"), (C.n_states, "start state"),
                       (-1, "start state"), (torch.zeros(3, 1, dtype=I32), "2-D tensor")):
        with pytest.raises(ValueError, match=match):
            C.starts("w", bad, 3)


# ---- validation
def test_every_validation_error():
    cls, tr = torch.zeros(V, dtype=I32), torch.zeros(1, 1, dtype=I32)
    for args, match in (((torch.zeros(V, 2, dtype=I32), tr), "token_class must be a non-empty 1-D"), ((torch.zeros(0, dtype=I32), tr), "non-empty 1-D"),
                        ((cls, torch.zeros(3, dtype=I32)), "trans must be a 2-D"), ((cls, torch.zeros(0, 1, dtype=I32)), "trans must be a 2-D"),
                        ((cls.long(), tr), "token_class must be int32"), ((cls, tr.long()), "trans must be int32"),
                        ((cls, tr.float()), "trans must be int32"),
                        ((torch.full((V,), 1, dtype=I32), tr), r"token_class holds 1, outside \[0, n_classes = 1\)"),
                        ((torch.full((V,), -1, dtype=I32), tr), r"token_class holds -1"),
                        ((cls, torch.full((1, 1), 1, dtype=I32)), r"trans holds 1, outside \[-1, n_states = 1\)"),
                        ((cls, torch.full((1, 1), -2, dtype=I32)), "trans holds -2"),
                        ((cls, torch.zeros(TC.MAX_STATES + 1, 1, dtype=I32)), "4097 states, at most 4096"),
                        ((cls, torch.zeros(1, TC.MAX_CLASSES + 1, dtype=I32)), "4097 classes, at most 4096")):
        with pytest.raises(ValueError, match=match):
            TokenConstraint(*args)
    TokenConstraint(cls, torch.zeros(TC.MAX_STATES, 1, dtype=I32))  # the bound itself is legal
    with pytest.raises(ValueError, match="start state"):
        TokenConstraint(cls, tr, start=1)


def test_an_empty_state_is_named():
    cls = torch.zeros(V, dtype=I32)
    cls[7] = 1
    with pytest.raises(ValueError, match="state 1 allows no token"):
        TokenConstraint(cls, torch.tensor([[1, 0, -1], [-1, -1, -1]], dtype=I32))
    with pytest.raises(ValueError, match="state 2 allows no token"):  # its only class holds no token
        TokenConstraint(cls, torch.tensor([[1, 2, -1], [0, 0, -1], [-1, -1, 0]], dtype=I32))
    with pytest.raises(ValueError, match="state 0 allows no token"):
        TokenConstraint.from_allowed_tokens(V, [])
    with pytest.raises(ValueError, match="state 0 allows no token"):
        TokenConstraint.from_suppressed_tokens(V, range(V))


def test_builders_refuse_ids_outside_the_vocabulary():
    for make in (lambda ids: TokenConstraint.from_allowed_tokens(V, ids), lambda ids: TokenConstraint.from_suppressed_tokens(V, ids),
                 lambda ids: TokenConstraint.from_sequences(V, [[1, 2], ids], 5), lambda ids: TokenConstraint.from_sequences(V, [[1]], ids[-1])):
        for bad in ([3, V], [3, -1], [3, 1.5], [3, True]):
            with pytest.raises(ValueError, match="outside"):
                make(bad)
    with pytest.raises(ValueError, match="vocab must be >= 1"):
        TokenConstraint.from_allowed_tokens(0, [])
    for seqs in ([], [[1], []]):
        with pytest.raises(ValueError, match="at least one"):
            TokenConstraint.from_sequences(V, seqs, 5)
    with pytest.raises(ValueError, match="end_token 5 occurs inside"):
        TokenConstraint.from_sequences(V, [[1, 5, 2]], 5)
    with pytest.raises(ValueError, match="at most 4096"):
        TokenConstraint.from_sequences(5000, [list(range(1, 4200))], 0)
    with pytest.raises(ValueError, match="at least one"):
        TokenConstraint.union([])
    with pytest.raises(ValueError, match="vocabularies differ"):
        TokenConstraint.union([TokenConstraint.free(V), TokenConstraint.free(V + 1)])
    big = TokenConstraint(torch.zeros(V, dtype=I32), torch.zeros(3000, 1, dtype=I32))
    with pytest.raises(ValueError, match="6000 states"):
        TokenConstraint.union([big, big])


# ---- the generate entries refuse before anything is called
def _refusals(cfg):
    Vm = cfg.llama.vocab
    A = TokenConstraint.from_sequences(Vm, [[11, 12], [30]], 5)
    ok = dict(max_new_tokens=4, no_repeat_ngram_size=0, constraint=A)
    both = [(dict(no_repeat_ngram_size=3), "pass 0"), (dict(no_repeat_ngram_size=[0, 0, 1]), "pass 0"),
            (dict(no_repeat_ngram_size=torch.tensor([0, 2, 0])), "pass 0"), (dict(min_new_tokens=2, eos_token_id=5), "min_new_tokens = 0"),
            (dict(min_new_tokens=[0, 1, 0], eos_token_id=5), "min_new_tokens = 0"), (dict(constraint=TokenConstraint.free(Vm + 3)), "vocabulary has"),
            (dict(constraint=object()), "TokenConstraint or None"), (dict(constraint_start=A.n_states), "start state"),
            (dict(constraint_start=[0, 1]), "constraint_start has 2 values for 3 requests"), (dict(constraint_start=[0, 99, 0]), r"constraint_start\[1\] = 99"),
            (dict(constraint=None, constraint_start=1), "constraint_start needs a constraint")]
    batch_only = [(dict(num_beams=2, do_sample=False), "not built for num_beams > 1"), (dict(prompt_lookup_num_tokens=3), "not built for prompt_lookup_num_tokens")]
    return ok, both, batch_only


def test_the_entries_refuse_before_any_call():
    with GS.stubbed() as stub:
        cfg, m = GS.tiny_model()
        vis, ids, mask = GS._requests(cfg, 3)
        ok, both, batch_only = _refusals(cfg)
        for bad, match in both + batch_only:
            with pytest.raises(ValueError, match="generate_batch: .*" + match):
                m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, **dict(ok, **bad))
        for bad, match in both:
            with pytest.raises(ValueError, match="generate_pool: .*" + match):
                m.mllm.generate_pool(vis, ids, mask, slots=2, **dict(ok, **bad))
        with pytest.raises(ValueError, match="pass 0"):  # the reference's default of 3
            m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, max_new_tokens=4, constraint=ok["constraint"])
        with pytest.raises(ValueError, match="pass 0"):
            m.mllm.generate_pool(vis, ids, mask, max_new_tokens=4, slots=2, constraint=ok["constraint"])
        assert stub.calls == [] and not m.mllm._ws._bufs
        m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, **ok)  # and the legal call goes through
        assert any(c[0] == "tcavt_constraint_build" for c in stub.calls)


def test_the_flag_is_reported_as_a_runtime_error():
    with GS.stubbed():
        cfg, m = GS.tiny_model()
        vis, ids, mask = GS._requests(cfg, 3)
        A = TokenConstraint.from_sequences(cfg.llama.vocab, [[11, 12], [30]], 5)
        m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, max_new_tokens=3, no_repeat_ngram_size=0, constraint=A)
        m.mllm.check_flags()
        m.mllm._constraint_flag.fill_(1)  # what tcavt_constraint_advance leaves behind a token outside the state
        with pytest.raises(RuntimeError, match="does not allow"):
            m.mllm.check_flags()
        m.mllm.check_flags()  # read once: the flag is cleared
        m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, max_new_tokens=3)
        assert m.mllm._constraint_flag is None


def test_a_beam_call_drops_the_flags_of_the_call_before():
    with GS.stubbed():
        cfg, m = GS.tiny_model()
        vis, ids, mask = GS._requests(cfg, 3)
        A = TokenConstraint.from_sequences(cfg.llama.vocab, [[11, 12], [30]], 5)
        m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, max_new_tokens=3, no_repeat_ngram_size=0, constraint=A,
                              temperature=[0.9, 0.8, 0.7])
        assert m.mllm._constraint_flag is not None and m.mllm._request_flag is not None
        m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, max_new_tokens=3, num_beams=2, do_sample=False)
        assert m.mllm._constraint_flag is None and m.mllm._request_flag is None


# ---- the condition of the GPU sampler test
def test_the_reference_alone_decides_the_sampler_tests_cases():
    scores, hist, hl = CR.sampler_inputs()
    C = CR.cycle_constraint(CR.V)
    R = scores.shape[0]
    assert all(np.isfinite(CR.masked(C, s, scores[r])).any() for s in range(3) for r in range(R))  # no row is ever left empty
    tally = SR.Tally("reference alone")
    for params in CR.SETS:
        chain = CR.Chain(C, scores, hist, hl, CR.CAP, params, np.arange(R) % 3, tally)
        for t in range(CR.STEPS):
            chain.step(t)
    assert tally.n == len(CR.SETS) * CR.STEPS * R and tally.share <= SR.UNDECIDED_CAP, tally.report()
