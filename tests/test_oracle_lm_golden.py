"""Pins the oracle's LM loss (oracle.forward.lm_head_and_loss) to tests/golden/tiny_lm_loss.npz: `outputs.loss` of the
reference's own LlamaWithCrossAttnPEFT.forward(..., labels=fused_labels), captured by tests/golden/make_golden_lm.py.
fp32 both sides, on the fixture's own final hidden states; measured 9e-8 relative at worst."""
import os

import numpy as np
import pytest
import torch

from tests.util import GOLDEN, load_case

LM_CASES = [("tiny_6_12_lora_ragged", "tiny_6_12_lora_ragged"), ("tiny_18_30_nolora_ragged", "tiny_18_30_nolora_ragged"),
            ("tiny_6_30_lora_full", "tiny_6_30_lora_full"), ("tiny_6_12_lora_ragged_answers", "tiny_6_12_lora_ragged")]


def load_lm():
    return dict(np.load(os.path.join(GOLDEN, "tiny_lm_loss.npz"), allow_pickle=False))


def test_fixture_holds_the_four_cases():
    lm = load_lm()
    assert [str(c) for c in lm["cases"]] == [c for c, _ in LM_CASES]
    assert all(v.dtype != object for v in lm.values())
    _, _, fx = load_case("tiny_6_12_lora_ragged")
    lab, mask = lm["tiny_6_12_lora_ragged_answers.labels"], fx["attention_mask"]
    for b in range(lab.shape[0]):  # the first ceil(len / 2) labels of every row are -100, the rest are the case's own
        n = int(mask[b].sum())
        assert (lab[b, : -(-n // 2)] == -100).all() and (lab[b, -(-n // 2):] == fx["labels"][b, -(-n // 2):]).all()


@pytest.mark.parametrize("case,base", LM_CASES)
def test_oracle_lm_loss_matches_reference_fixture(case, base):
    from oracle import forward as O

    cfg, weights, fx = load_case(base)
    lm = load_lm()
    labels = torch.from_numpy(lm[case + ".labels"])
    if case == base:
        assert torch.equal(labels, torch.from_numpy(fx["labels"]))
    fused = torch.cat([torch.full((labels.shape[0], cfg.q_num_query_tokens), -100, dtype=labels.dtype), labels], 1)
    with torch.no_grad():
        loss = O.lm_head_and_loss(O.as_torch(weights), torch.from_numpy(fx["exp_final_hidden"]), fused)
    ref = float(lm[case + ".loss"])
    assert int(lm[case + ".n"]) == int((fused[:, 1:] != -100).sum())
    assert abs(loss.item() - ref) <= 1e-5 * abs(ref), (loss.item(), ref)
