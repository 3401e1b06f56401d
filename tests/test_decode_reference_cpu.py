"""The float64 reference of one decode step (oracle/decode.py) against the oracle it restates: the per-layer K / V of
oracle.forward.llama_decoder on a prefix are the cache, the next token is fed, and the logits must equal
oracle.generation.next_logits on the whole sequence to float64 round-off (fp32 contract: no rounding point rounds, both
sides run in float64).  tests/test_decode_step_gpu.py measures tcavt_llama_decode_step with this reference."""
import dataclasses

import pytest
import torch


def _cfg(use_lora=True):
    from tcavt_amd import config

    return dataclasses.replace(config.tiny(use_lora=use_lora),
                               llama=config.LlamaShape(hidden=256, inter=512, layers=2, n_q_heads=8, n_kv_heads=2, vocab=512))


@pytest.mark.parametrize("use_lora", [True, False], ids=["lora", "nolora"])
def test_decode_step_equals_next_logits_on_the_whole_sequence(use_lora):
    from oracle import decode as D
    from oracle import forward as O
    from oracle import generation as G
    from tcavt_amd.weights import make_weights

    cfg = _cfg(use_lora)
    ll = cfg.llama
    W = {k: v.double() for k, v in O.as_torch(make_weights(cfg, 5)).items()}
    if use_lora:  # (make_weights may leave lora_B at its zero initialisation: give the adapters something to do)
        g = torch.Generator().manual_seed(1)
        for k in W:
            if ".lora_B." in k:
                W[k] = W[k] + 0.05 * torch.randn(W[k].shape, generator=g, dtype=torch.float64)
    Wp = D.prepare(W, cfg, "fp32")
    g = torch.Generator().manual_seed(2)
    lens = [1, 7, 70]  # tokens in the whole sequence: the fed token alone (empty cache), a short and a longer prefix
    ids = [torch.randint(0, ll.vocab, (n,), generator=g) for n in lens]
    lmax = max(lens)
    kc = [torch.full((len(lens), lmax, ll.n_kv_heads, ll.head_dim), float("nan"), dtype=torch.float64) for _ in range(ll.layers)]
    vc = [t.clone() for t in kc]
    want = []
    with torch.no_grad():
        for b, t in enumerate(ids):
            seq = D.token_embeds(Wp, t)[None]  # [1, n, H]
            want.append(G.next_logits(W, cfg, seq, "fp32"))
            if len(t) > 1:
                kv = []
                O.llama_decoder(W, cfg, seq[:, :-1], torch.ones(1, len(t) - 1, dtype=torch.int64), O._rounder("fp32"), collect_kv=kv)
                assert len(kv) == ll.layers
                for li, (k, v) in enumerate(kv):
                    kc[li][b, : len(t) - 1], vc[li][b, : len(t) - 1] = k[0], v[0]
        pos = torch.tensor([n - 1 for n in lens])
        emb = D.token_embeds(Wp, torch.stack([t[-1] for t in ids]))
        logits, new_kv = D.decode_step(Wp, cfg, emb, pos, kc, vc, "fp32")
    assert logits.dtype == torch.float64 and tuple(logits.shape) == (len(lens), ll.vocab) and len(new_kv) == ll.layers
    for b in range(len(lens)):
        assert want[b].dtype == torch.float64
        e = ((logits[b] - want[b]).norm() / want[b].norm()).item()
        assert e < 1e-12, (b, e)
    # the appended rows are what the whole-sequence pass attends at the last position
    with torch.no_grad():
        kv = []
        O.llama_decoder(W, cfg, D.token_embeds(Wp, ids[2])[None], torch.ones(1, lens[2], dtype=torch.int64), O._rounder("fp32"), collect_kv=kv)
    for li, (k, v) in enumerate(kv):
        assert (new_kv[li][0][2] - k[0, -1]).abs().max().item() < 1e-12 and (new_kv[li][1][2] - v[0, -1]).abs().max().item() < 1e-12


def test_rounding_points_round_to_the_storage_type():
    """in the fp16 contract the reference's stored values are fp16 values (carried as float64)"""
    from oracle import decode as D
    from oracle import forward as O
    from tcavt_amd.weights import make_weights

    cfg = _cfg()
    ll = cfg.llama
    W = O.as_torch(make_weights(cfg, 5))
    Wp = D.prepare(W, cfg, "fp16")
    for k, v in Wp["layers"][0].items():
        assert v.dtype == torch.float64 and torch.equal(v.to(torch.float16).double(), v), k
    assert torch.equal(Wp["g_final"], W[O.LLAMA + "norm.weight"].double())  # the gains stay fp32
    # fp8 map: only the frozen matrices and the lm_head's table change
    W8 = D.prepare(W, cfg, "fp16", weight_map=lambda t: t * 0)
    assert not W8["layers"][0]["wq"].any() and not W8["head"].any() and torch.equal(W8["table"], Wp["table"])
    assert torch.equal(W8["layers"][0]["aq"], Wp["layers"][0]["aq"])
    pos = torch.tensor([0, 3])
    kc = [torch.randn(2, 4, ll.n_kv_heads, ll.head_dim).half().double() for _ in range(ll.layers)]
    with torch.no_grad():
        logits, new_kv = D.decode_step(Wp, cfg, D.token_embeds(Wp, torch.tensor([5, 9])), pos, kc, kc, "fp16")
    assert torch.isfinite(logits).all()
    for k, v in new_kv:
        assert torch.equal(k.to(torch.float16).double(), k) and torch.equal(v.to(torch.float16).double(), v)
