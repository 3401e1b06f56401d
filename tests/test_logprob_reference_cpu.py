"""The float64 reference of the generated tokens' log-probabilities, its bar, and generation.rank_continuations -- no GPU.

First the bar itself: an fp32 numpy restatement of exactly the kernels' summation shape (tests/logprob_ref.py) stays well inside
|got - ref| <= 1e-5 + 2^-22 |ref|, so the bar admits the arithmetic alone; a fully serial fp32 sum over a slice is worse.  Then
the planted cases of the GPU kernel test against the reference: each faulty reading misses the bar by a wide margin."""
import numpy as np
import pytest
import torch

import logprob_ref as R
import sampler_ref
from tcavt_amd import generation


def _tokens(x):
    g = np.random.default_rng(x.size)
    return [int(np.argmax(x)), int(np.argmin(x)), int(g.integers(x.size)), int(np.argsort(x)[x.size // 2])]


@pytest.mark.parametrize("V", R.VOCABS)
def test_bar_admits_the_fp32_restatement_of_the_summation_shape(V):
    worst = 0.0
    for sigma in R.SIGMAS:
        x = R.random_row(V, sigma)
        for t in _tokens(x):
            worst = max(worst, R.ratio(R.restate_fp32(x, t), R.ref_logprob(x, t)))
    print(f"V = {V}: fp32 restatement at {worst:.3f} of the bar")
    assert worst <= 0.3


def test_serial_slice_sum_is_worse_than_the_tree():
    V, tree, serial = 262144, 0.0, 0.0
    for sigma in (1.0, 4.0):
        x = R.random_row(V, sigma)
        t = int(np.argmax(x))
        ref = R.ref_logprob(x, t)
        tree, serial = max(tree, R.ratio(R.restate_fp32(x, t), ref)), max(serial, R.ratio(R.serial_fp32(x, t), ref))
    print(f"tree {tree:.3f}, serial {serial:.3f} of the bar")
    assert serial > tree


def test_slices_cover_the_row_once():
    for V in R.VOCABS + (1, 3, 4, 5, 63, 64, 65, 300000):
        b = R.slice_bounds(V)
        assert b[0][0] == 0 and b[-1][1] == V and all(lo <= hi for lo, hi in b)
        assert all(b[g][1] == b[g + 1][0] for g in range(15))


@pytest.mark.parametrize("V", (48, 1003, 128256))
def test_planted_single_element_discriminates(V):
    for p in R.planted_positions(V):
        x = R.planted_single(V, p)
        ref = R.ref_logprob(x, p)
        assert R.ratio(R.restate_fp32(x, p), ref) <= 1.0
        dropped = (0.0 - (-40.0)) - np.log(V - 1.0)  # the planted element missing from the normaliser
        assert abs(dropped - ref) >= 25.0 and R.ratio(dropped, ref) > 1e5


@pytest.mark.parametrize("V", (1000, 128256))
def test_planted_processor_cases_discriminate(V):
    for c in R.planted_cases(V):
        x, _ = sampler_ref.process_logits(c["scores"], c["hist"], c["penalty"], c["ngram"])
        if c["min_new"] > 0:
            x[c["eos"]] = -np.inf
        assert int(np.argmax(x)) == c["token"], c["name"]  # the selection chooses it after the processors
        ref = R.ref_logprob(c["scores"], c["token"])
        assert R.ratio(R.restate_fp32(c["scores"], c["token"]), ref) <= 1.0, c["name"]
        assert abs(c["wrong"] - ref) >= 1.0 and R.ratio(c["wrong"], ref) > 1e4, c["name"]


def test_rank_continuations_order_ties_and_length_penalty():
    s = torch.tensor([-6.0, -2.0, -4.0, -3.0, -3.0, -1.0], dtype=torch.float32)
    k = torch.tensor([3, 1, 4, 3, 3, 1], dtype=torch.int32)
    r = generation.rank_continuations(s, k, 3)
    assert r.dtype == torch.int64 and r.shape == (2, 3)
    assert r.tolist() == [[2, 0, 1], [0, 1, 2]]  # means -2, -2, -1 | -1, -1, -1: ties to the lower index
    assert generation.rank_continuations(s, k, 3, length_penalty=0.0).tolist() == [[1, 2, 0], [2, 0, 1]]  # plain sums
    assert generation.rank_continuations(s, k, 3, length_penalty=2.0).tolist() == [[2, 0, 1], [0, 1, 2]]
    assert generation.rank_continuations(s, k, 1).tolist() == [[0]] * 6
    with pytest.raises(ValueError):
        generation.rank_continuations(s, k, 4)
