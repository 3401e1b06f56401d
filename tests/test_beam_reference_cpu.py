"""tests/beam_ref.py, the float64 restatement of the beam search the kernels run, against HF's own results: for every case of
tests/golden/tiny_beam.npz (made by tests/golden/make_golden_beam.py from transformers' generate(num_beams=n, do_sample=False) on a
tiny float64 Llama) the search is replayed from the recorded logits rows alone.  Pass mark: sequences equal, sequences_scores within
1e-9 relative (float64 against float64).  Needs neither transformers nor a GPU."""
import os

import numpy as np
import pytest

import beam_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_beam.npz")
PAD = 0


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _cases(g):
    return [(int(n), int(N), float(lp), bool(early), float(pen), int(ng), int(eos)) for n, N, lp, early, pen, ng, eos, _ in g["cases"]]


def test_fixture_covers_the_argument_space(golden):
    cases = _cases(golden)
    assert len(cases) >= 12
    assert {c[0] for c in cases} == {2, 3, 4} and {c[1] for c in cases} == {6, 8, 10} and {c[2] for c in cases} == {0.5, 1.0, 2.0}
    assert {c[3] for c in cases} == {False, True} and {c[4] for c in cases} == {1.0, 1.2} and {c[5] for c in cases} == {0, 2, 3}
    reached = sum(bool((golden[f"c{i}_sequences"] == c[6]).any()) for i, c in enumerate(cases))
    assert 2 * reached >= len(cases)  # EOS ends a hypothesis in at least half of the cases
    assert os.path.getsize(GOLDEN) < 200 * 1024


@pytest.mark.parametrize("c", range(12))
def test_restatement_repeats_hf(golden, c):
    n, N, lp, early, pen, ng, eos = _cases(golden)[c]
    table = {tuple(int(t) for t in pre if t >= 0): row for pre, row in zip(golden[f"c{c}_prefixes"], golden[f"c{c}_rows"])}
    got = beam_ref.search(lambda prefix: table[prefix], golden[f"c{c}_prompt"], n, N, eos, pen, ng, lp, early, pad=PAD)
    assert np.array_equal(got["sequences"], golden[f"c{c}_sequences"])
    want = golden[f"c{c}_scores"]
    assert got["scores"].shape == want.shape
    assert np.all(np.abs(got["scores"] - want) <= 1e-9 * np.abs(want)), (got["scores"], want)
    assert len(got["trace"]) == got["steps"] and all(len(k) == 2 * n for k in got["trace"])  # the K candidates of every step
