"""Host-side rules of the autograd bridge (autograd.py): which requires-grad states activate it, and the argument checks of
the seeded loss gradient that need no GPU."""
import pytest
import torch

from tests.util import load_case


def _model(case="tiny_6_12_lora_ragged"):
    from tcavt_amd import model

    cfg, weights, _ = load_case(case)
    return model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights)


def _freeze(m):
    for p in m.mllm.parameters():
        p.requires_grad_(False)


def test_activation_rule():
    from tcavt_amd import autograd as A

    m = _model()
    assert A.trainable_set(m) is None  # default: every parameter requires grad
    _freeze(m)
    assert A.trainable_set(m) == A.S0
    with torch.no_grad():
        assert A.trainable_set(m) is None
    lora = [p for n, p in m.mllm.named_parameters() if ".lora_" in n]
    assert len(lora) > 0
    for p in lora:
        p.requires_grad_(True)
    assert A.trainable_set(m) == A.S1
    lora[0].requires_grad_(False)
    assert A.trainable_set(m) is None  # part of the adapters: not a supported set
    lora[0].requires_grad_(True)
    m.mllm.llama_wrapper.llama_model.model.layers[0].self_attn.k_proj.weight.requires_grad_(True)
    assert A.trainable_set(m) is None  # a Llama base weight
    _freeze(m)
    m.mllm.qformer.query_tokens.requires_grad_(True)
    assert A.trainable_set(m) is None  # the Q-Former (modify_train.py's whole set): out of scope
    _freeze(m)
    for p in list(m.ltsf.parameters()) + list(m.lane_polygon_encoder.parameters()):
        p.requires_grad_(False)
    assert A.trainable_set(m) is None  # nothing trains
    m.ltsf.decoder.out_proj.weight.requires_grad_(True)
    assert A.trainable_set(m) == A.S0
    m.driven_by_trainer = True
    assert A.trainable_set(m) is None


def test_activation_without_lora_adapters():
    from tcavt_amd import autograd as A

    m = _model("tiny_18_30_nolora_ragged")
    _freeze(m)
    assert A.trainable_set(m) == A.S0


def test_shared_flags_per_set():
    from tcavt_amd import training

    m = _model()
    s0 = {(type(o).__name__, a): v for o, a, v in training.backward_flags(m, False)}
    s1 = {(type(o).__name__, a): v for o, a, v in training.backward_flags(m, True)}
    assert s0[("TransformerLTSF", "save_for_backward")] and s0[("LanePolygonEncoder", "save_for_backward")]
    assert ("LlamaWithCrossAttnPEFT", "save_for_backward") not in s0 and s1[("LlamaWithCrossAttnPEFT", "save_for_backward")]
    assert s1[("TransformerLTSF", "absorb_kv")] is False and s0[("LlamaMultiModal", "skip_f32_hidden")] is True
    assert s1[("LlamaMultiModal", "skip_f32_hidden")] is False and s1[("MultiModalTrajectoryModel", "pipeline_decoder")] is False


def test_mse_grad_seeded_refuses_two_absent_seeds():
    from tcavt_amd import capi, ops

    g = torch.zeros(2, 2, 3)
    with pytest.raises(capi.TcavtError):
        ops.mse_grad_seeded(g, g, torch.zeros(2, 4), g, 2, 3)
