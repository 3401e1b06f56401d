"""tests/constraint_ref.py -- mask by TokenConstraint.allowed, then sampler_ref.process_logits, then the arg-max -- against HF's own
results: every case of tests/golden/tiny_constraint.npz (made by tests/golden/make_golden_constraint.py from transformers'
generate(prefix_allowed_tokens_fn=..., do_sample=False) on a tiny float64 Llama) is replayed from the recorded logits rows alone
and must reproduce HF's tokens exactly.  Needs neither transformers nor a GPU."""
import os

import numpy as np
import pytest
import torch

from tests import constraint_ref as CR

from tcavt_amd.constraint import TokenConstraint

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_constraint.npz")
PAD, N_CASES = 0, 11


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _case(g, c):
    N, pen, eos, start, n_gen = g["cases"][c]
    C = TokenConstraint(torch.from_numpy(g[f"c{c}_token_class"]), torch.from_numpy(g[f"c{c}_trans"]))
    return C, int(N), float(pen), int(eos), int(start), int(n_gen)


def test_fixture_covers_the_argument_space(golden):
    cases = [_case(golden, c) for c in range(N_CASES)]
    assert len(golden["cases"]) == N_CASES >= 10
    assert {c[2] for c in cases} == {1.0, 1.2}
    ended = [bool((golden[f"c{i}_sequences"] == c[3]).any()) for i, c in enumerate(cases)]
    assert 3 <= sum(ended) <= N_CASES - 3  # an EOS inside the form ends the row; one outside it never appears
    assert {c[0].n_states for c in cases} >= {1, 9}  # allowed / suppressed sets (one state) and tries
    assert any(c[4] != 0 for c in cases)  # a union member that does not start in state 0
    assert os.path.getsize(GOLDEN) < 100 * 1024


@pytest.mark.parametrize("c", range(N_CASES))
def test_replay_repeats_hf(golden, c):
    C, N, pen, eos, start, n_gen = _case(golden, c)
    prompt, want, rows = golden[f"c{c}_prompt"].tolist(), golden[f"c{c}_sequences"], golden[f"c{c}_rows"]
    assert rows.shape == (n_gen, C.vocab)
    state, got = start, []
    for i in range(N):
        tok = CR.greedy(C, state, rows[i], prompt + got, pen)  # (HF's penalty sees the prompt and the tokens so far)
        assert tok in C.allowed(state)
        got.append(tok)
        state = C.next(state, tok)
        if tok == eos:
            break
    assert len(got) == n_gen
    assert got + [PAD] * (N - len(got)) == want.tolist()
    assert C.walk(got, start=start) == (state, n_gen)
