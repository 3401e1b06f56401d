"""The float64 reference alone over the exact cases of tests/test_sampler_per_request_gpu.py (tests/per_request_cases.py): the
share of UNDECIDED cases of every GPU test must be at most sampler_ref.UNDECIDED_CAP (2 %).  The cap is a condition on the inputs,
not a tolerance on the kernel: the inputs are chosen so that the reference alone meets it.  Also: the cases do what their
docstring says (greedy rows among sampled ones, every top_k, a seed above 2^32, a permutation that is not the identity)."""
import numpy as np
import pytest

from tests import per_request_cases as PC
from tests import sampler_ref as SR


@pytest.mark.parametrize("form", PC.FORMS)
@pytest.mark.parametrize("V", PC.VOCABS)
def test_undecided_share_of_the_reference_alone(V, form):
    n = undecided = 0
    for j in PC.calls(V):
        for _, entry, *_, choice in PC.choices(V, form, j):
            if PC.FIN0[entry]:
                continue
            n += 1
            undecided += not choice.decided
    print(f"\n[per_request] V={V} {form}: {n} cases, {undecided} undecided ({100.0 * undecided / n:.2f} %)")
    assert n >= 24 and undecided <= SR.UNDECIDED_CAP * n, (V, form, n, undecided)


def test_the_cases_mix_what_they_should():
    assert not np.array_equal(PC.OUT_ROW, np.arange(PC.N_ROWS)) and len(set(PC.OUT_ROW.tolist())) == PC.N_ROWS
    assert PC.OUT_ROW.max() < PC.N_REQ and len(set(PC.STEPS.tolist())) > 1 and (PC.SLOT_OF_ROW == -1).sum() == 1
    for V in PC.VOCABS:
        for form in PC.FORMS:
            seen_k, seeds, greedy_next_to_sampled = set(), set(), False
            for j in PC.calls(V):
                prm = PC.request_params(j)
                used = [prm[req] for _, _, req, _ in PC.placement(form, j)]
                seen_k |= {q["k"] for q in used if q["do_sample"]}
                seeds |= {q["seed"] for q in used if q["do_sample"]}
                modes = {q["do_sample"] for q in used}
                greedy_next_to_sampled |= modes == {0, 1}
                assert len({(q["T"], q["k"], q["p"], q["rep"], q["ngram"], q["do_sample"], q["seed"]) for q in used}) > 1
            assert seen_k == {1, 5, 40, 256} and any(s >= 1 << 32 for s in seeds) and greedy_next_to_sampled, (V, form)
