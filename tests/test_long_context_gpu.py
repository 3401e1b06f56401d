"""Stage 1 at its own sequence length: the decoder beyond 544 rows (streaming attention forward, chunked backward under the
higher cap) through every entry point that reaches it, against the CPU oracle.

Model: config.tiny() with 8 query / 2 key-value heads (hidden 256, 2 layers, vocab 512, LoRA r 8), fp16 storage.  (hidden 256,
not 128: tcavt_llama_stack_forward takes hidden sizes that are multiples of 256.)

1. dispatch: through tcavt_llama_stack_forward with a tape, L = 544 is the resident kernel's bits and L = 545 the streaming
   kernel's; L = 2049 is refused.
2. final_hidden at B = 2, Lt = 1024 (L = 1040, lengths [1024, 700]) against oracle.forward.mllm_forward: the bar form of
   test_model_parity_gpu.py (1.5 x the contract's own error against fp32 + 1e-3).
3. lm_forward / lm_evaluate on that batch: loss at LOSS_BAR_ORACLE of test_lm_loss_model_gpu.py, the two losses bit-equal, pred
   = the oracle's arg-max wherever the oracle's top-two gap exceeds twice the logit bar (2e-3 of the row's norm, the
   decode-logit bar); that set is computed from the oracle alone and covers >= 95 % of the labelled rows.
4. LoRA gradients through the layers (the recipe of test_lora_grads_through_the_layers_at_320) at L = 640 (M = 1280: the stage
   call) and L = 1040 (M = 2080: the composition), ragged, with and without LoRA dropout: < 7.5e-3 per tensor; stage call
   against composition within 2e-4 at 640; the tiled fallback (TCAVT_ATTN_BWD_NO_STREAM) within e <= 1.5 e_tiled + 1e-4.
5. MllmTrainer at L = 640: the first backward's flat gradient against the oracle's autograd at GRAD_NORM_BAR / GRAD_COS_BAR of
   test_lm_loss_model_gpu.py; two steps, finite loss, no skipped update.
6. generation: prompt Lt = 600 (lengths [600, 570]), 8 greedy tokens, eager and graph ids equal, every step's logits against
   the oracle decoder on the growing sequence at 2e-3, ids = the oracle's arg-max; the oracle's own top-two gap is asserted first.
7. the trajectory model at L = 560 (ids) and at L = 545 through the tokenizer branch raises before anything is launched; the
   message names 544.
"""
import dataclasses
import math

import numpy as np
import pytest
import torch

from tests.util import rel_err

pytestmark = pytest.mark.gpu

F16 = torch.float16
LOGIT_BAR = 2e-3          # the decode-logit bar of test_generation_gpu.py (relative to the row's norm)
SEED_W, SEED_LM, SEED_GEN = 5, 31, 7
_cache = {}


def _cfg():
    from tcavt_amd import config

    return dataclasses.replace(config.tiny(), llama=config.LlamaShape(hidden=256, inter=512, layers=2, n_q_heads=8, n_kv_heads=2, vocab=512))


def _weights(cfg):
    from tcavt_amd.weights import make_weights

    if "w" not in _cache:
        _cache["w"] = make_weights(cfg, SEED_W)
    return _cache["w"]


def _model(cfg, weights, dev):
    from tcavt_amd import model

    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights, device=dev).eval()
    m.set_storage(F16)
    return m


def _batch(cfg, lens, Lt, seed):
    """make_batch with the given text lengths (right padding: ids 0, mask 0, labels -100) -> dict of CPU tensors"""
    from tcavt_amd import synth

    b = synth.make_batch(cfg, len(lens), text_len=Lt, seed=seed, ragged=False)
    for i, n in enumerate(lens):
        b["input_ids"][i, n:] = 0
        b["attention_mask"][i, n:] = 0
        b["labels"][i, n:] = -100
    return {k: torch.from_numpy(np.asarray(v)) for k, v in b.items()}


def _oracle_lm(cfg, weights, t):
    """the oracle on the fp16 contract, from the CPU alone: final hidden states (fp16 and fp32 contract), the loss and the
    logits of the rows that predict a label (float64 on the 16-bit operands the kernels read)"""
    from oracle import forward as O

    if "lm" in _cache:
        return _cache["lm"]
    W = O.as_torch(weights)
    Nq = cfg.q_num_query_tokens
    with torch.no_grad():
        f16 = O.mllm_forward(W, cfg, t["vision_emb"], t["input_ids"], t["attention_mask"], "fp16")
        f32 = O.mllm_forward(W, cfg, t["vision_emb"], t["input_ids"], t["attention_mask"], "fp32")
        table = W["mllm.llama_wrapper.llama_model.lm_head.weight"].to(F16).double()
        labels = t["labels"]
        fused = torch.cat([torch.full((labels.shape[0], Nq), -100, dtype=labels.dtype), labels], 1)
        h = f16.to(F16).double()
        loss = float(O.lm_head_and_loss({"mllm.llama_wrapper.llama_model.lm_head.weight": table}, h, fused))
        logits = h[:, Nq - 1:-1] @ table.T  # [B, Lt, V]: row Nq + j - 1 predicts labels[:, j]
    _cache["lm"] = (f16, f32, loss, logits)
    return _cache["lm"]


def _qualifying(logits, labels):
    """rows whose oracle top-two gap exceeds twice the logit bar, among the labelled ones; the oracle's arg-max"""
    top = torch.topk(logits, 2, dim=-1)
    gap = top.values[..., 0] - top.values[..., 1]
    lab = labels != -100
    return lab & (gap > 2 * LOGIT_BAR * logits.norm(dim=-1)), lab, top.indices[..., 0]


def _lm_case():
    cfg = _cfg()
    return cfg, _weights(cfg), _batch(cfg, [1024, 700], 1024, SEED_LM)


def test_dispatch_is_what_it_claims(gpu):
    from tcavt_amd import capi, ops, training

    dev = gpu["device"]
    cfg = _cfg()
    ll = cfg.llama
    m = _model(cfg, _weights(cfg), dev)
    training.Trainer(m, lora_trainable=True)  # (sets the flags that make the decoder keep its tape)
    lw = m.mllm.llama_wrapper
    nq, nkv, B = ll.n_q_heads, ll.n_kv_heads, 2
    g = torch.Generator().manual_seed(3)
    for L, entry in ((544, ops.attn_causal_gqa), (545, ops.attn_causal_gqa_stream)):
        embeds = (torch.randn(B, L, ll.hidden, generator=g) * 0.5).to(dev)
        mask = torch.ones(B, L, dtype=torch.int64, device=dev)
        mask[1, L - 45:] = 0
        with torch.no_grad():
            lw(embeds, mask)
        assert len(lw.tape.layers) == ll.layers
        for li, sv in enumerate(lw.tape.layers):
            out = torch.full_like(sv.att, float("nan"))
            lse = torch.full_like(sv.lse, float("nan"))
            entry(sv.qkv, out, lw.tape.kv_len, B, L, nq, nkv, 0.125, lse=lse)
            torch.cuda.synchronize()
            assert torch.equal(out, sv.att) and torch.equal(lse, sv.lse), (L, li)
    # L = 2049 through the wrapper: refused before anything is launched (the buffers its first launches write keep a sentinel)
    embeds = torch.ones(1, 2049, ll.hidden, device=dev)
    h16, part = lw.norm_inputs(2049, dev)
    h16.fill_(-3.0)
    part.fill_(-3.0)
    torch.cuda.synchronize()
    with pytest.raises(capi.TcavtError, match="L=2049"):
        lw(embeds, torch.ones(1, 2049, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    h16_after, part_after = lw.norm_inputs(2049, dev)
    assert h16_after.data_ptr() == h16.data_ptr() and bool((h16 == -3.0).all()) and bool((part == -3.0).all()), "the refused call launched"
    # ... and by the C entry itself when the stack is called directly
    with pytest.raises(capi.TcavtError, match="llama_stack_forward: L=2049"):
        lw.decoder_stack(None if lw.stream16 else torch.zeros(2049, ll.hidden, device=dev), torch.full((1,), 2049, dtype=torch.int32, device=dev),
                         1, 2049, out_f32=torch.empty(2049, ll.hidden, device=dev))
    # the MLLM's own entry refuses it before anything is launched
    t = _batch(cfg, [2040], 2040, 1)
    with pytest.raises(ValueError, match="2048"):
        m.mllm(t["vision_emb"].to(dev), None, input_ids=t["input_ids"].to(dev), attention_mask=t["attention_mask"].to(dev))


def test_final_hidden_lm_forward_and_lm_evaluate_at_1040(gpu):
    from test_lm_loss_model_gpu import LOSS_BAR_ORACLE

    dev = gpu["device"]
    cfg, weights, t = _lm_case()
    Nq = cfg.q_num_query_tokens
    f16, f32, loss_o, logits = _oracle_lm(cfg, weights, t)
    qual, lab, amax = _qualifying(logits, t["labels"])
    frac = float(qual.sum()) / float(lab.sum())
    print(f"[long context lm] oracle alone: {int(qual.sum())} of {int(lab.sum())} labelled rows have a top-two gap above twice the logit bar ({frac:.3f})")
    assert frac >= 0.95
    m = _model(cfg, weights, dev)
    g = {k: v.to(dev) for k, v in t.items()}
    with torch.no_grad():
        out = m.mllm.lm_forward(g["vision_emb"], None, g["input_ids"], g["attention_mask"], g["labels"])
        ev = m.mllm.lm_evaluate(g["vision_emb"], None, g["input_ids"], g["attention_mask"], g["labels"])
        torch.cuda.synchronize()
        m.mllm.check_flags()
    assert tuple(out.final_hidden.shape) == (2, 1040, cfg.llama.hidden) and int(out.n_tokens) == int(lab.sum())
    e, o = rel_err(out.final_hidden.float().cpu(), f16), rel_err(f16, f32)
    e_loss = abs(float(out.loss) - loss_o) / abs(loss_o)
    print(f"[long context lm] final_hidden vs fp16-oracle {e:.2e} (the contract's own error vs fp32 {o:.2e}); loss {float(out.loss):.6f} "
          f"vs oracle {loss_o:.6f} (rel {e_loss:.2e})")
    assert e <= 1.5 * o + 1e-3
    assert e_loss < LOSS_BAR_ORACLE["fp16"]
    assert torch.equal(ev.loss, out.loss) and int(ev.n_tokens) == int(out.n_tokens)
    pred = ev.pred.cpu()
    assert tuple(pred.shape) == tuple(t["labels"].shape)
    assert torch.equal(pred[qual], amax[qual]), f"{int((pred[qual] != amax[qual]).sum())} of {int(qual.sum())} qualifying rows differ"
    assert bool((pred[~lab] == -1).all())


@pytest.mark.parametrize("lora_drop", [False, True])
@pytest.mark.parametrize("L,lens", [(640, [640, 411]), (1040, [1040, 700])])
def test_lora_grads_through_the_layers(gpu, monkeypatch, L, lens, lora_drop):
    from oracle import forward as O
    from tcavt_amd import model, ops, training

    dev = gpu["device"]
    cfg = _cfg()
    weights = _weights(cfg)
    ll = cfg.llama
    B, H = 2, ll.hidden
    g = torch.Generator().manual_seed(11)
    embeds = torch.randn(B, L, H, generator=g) * 0.5
    mask = torch.zeros(B, L, dtype=torch.int64)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    G = torch.randn(B, L, H, generator=g).to(torch.bfloat16)
    W = {k: torch.from_numpy(v).clone() for k, v in weights.items()}
    keys = [k for k in W if ".lora_A." in k or ".lora_B." in k]
    assert len(keys) == 4 * ll.layers
    for k in keys:
        W[k].requires_grad_(True)
    seed = 0xD0C
    drop = O.DropTape(seed, cfg.lora_dropout, first_site=(2 << 16) + 1) if lora_drop else O._ident
    out = O.llama_decoder(W, cfg, embeds, mask, O._rounder("fp16"), drop=drop)
    (out * G.float()).sum().backward()

    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights, device=dev).eval()
    tr = training.Trainer(m, lora_trainable=True)
    lw = m.mllm.llama_wrapper
    calls, stage = [], []
    real, real_stage = ops.attn_bwd_stream, tr.lbw._stage_call
    monkeypatch.setattr(ops, "attn_bwd_stream", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(tr.lbw, "_stage_call", lambda *a, **k: (stage.append(1), real_stage(*a, **k))[1])

    def run():
        with torch.no_grad():
            lw.dctx = model.DropoutCtx(seed).sub(2) if lora_drop else None
            lw(embeds.to(dev), mask.to(dev))
            lw.dctx = None
            tr.lbw.run(G.reshape(B * L, H).contiguous().to(dev))
        torch.cuda.synchronize()
        got = {k: tr.book.g[k].detach().cpu().clone() for k in keys}
        return got, {k: rel_err(got[k], W[k].grad) for k in keys}

    g_def, e_def = run()
    if (B * L) % 256 == 0:  # the one-call decoder backward; then the Python composition of the same kernels
        assert stage == [1] and calls == []
        monkeypatch.setenv("TCAVT_PY_LLM_BACKWARD", "1")
        g_py, e_py = run()
        assert stage == [1] and len(calls) == ll.layers
        for k in keys:
            assert rel_err(g_def[k], g_py[k]) < 2e-4, k  # (atomics' summation order in the weight gradients)
    else:
        assert stage == [] and len(calls) == ll.layers, "M % 256 != 0: the composition, over the stream form"
        e_py = e_def
    n = len(calls)
    monkeypatch.setenv("TCAVT_ATTN_BWD_NO_STREAM", "1")
    _, e_tiled = run()
    assert len(calls) == n and stage == ([1] if (B * L) % 256 == 0 else [])
    print(f"[lora grads L={L} lora_dropout={lora_drop}] worst relative error: default {max(e_def.values()):.2e}, composition "
          f"{max(e_py.values()):.2e}, tiled {max(e_tiled.values()):.2e}")
    for k in keys:
        assert W[k].grad.abs().max() > 0, k
        assert e_def[k] < 7.5e-3 and e_py[k] < 7.5e-3, (k, e_def[k], e_py[k])
        assert e_py[k] < 1.5 * e_tiled[k] + 1e-4, (k, e_py[k], e_tiled[k])


def test_mllm_trainer_at_640(gpu):
    from oracle import forward as O
    from test_lm_loss_model_gpu import GRAD_COS_BAR, GRAD_NORM_BAR
    from tcavt_amd import training

    dev = gpu["device"]
    cfg = _cfg()
    weights = _weights(cfg)
    Nq = cfg.q_num_query_tokens
    t = _batch(cfg, [624, 500], 624, 9)
    W = O.as_torch(weights)
    keys = sorted(k for k in W if ".lora_A." in k or ".lora_B." in k)
    for k in keys:
        W[k].requires_grad_(True)
    final = O.mllm_forward(W, cfg, t["vision_emb"], t["input_ids"], t["attention_mask"], "fp16")
    table = W["mllm.llama_wrapper.llama_model.lm_head.weight"].detach().to(F16).double()
    fused = torch.cat([torch.full((2, Nq), -100, dtype=torch.int64), t["labels"]], 1)
    loss_o = O.lm_head_and_loss({"mllm.llama_wrapper.llama_model.lm_head.weight": table}, final.to(F16).double(), fused)
    loss_o.backward()

    m = _model(cfg, weights, dev)
    tr = training.MllmTrainer(m)
    g = {k: v.to(dev) for k, v in t.items()}
    args = (g["vision_emb"], g["input_ids"], g["attention_mask"], g["labels"])
    loss = tr.forward_backward(*args)
    torch.cuda.synchronize()
    tr.check_flags()
    assert set(tr.book.g) == set(keys)
    got = torch.cat([tr.book.g[k].detach().cpu().double().reshape(-1) for k in keys])
    ref = torch.cat([W[k].grad.double().reshape(-1) for k in keys])
    norm_dev = abs(float(got.norm()) - float(ref.norm())) / float(ref.norm())
    cos = float(got @ ref / (got.norm() * ref.norm()))
    print(f"[mllm trainer L=640] loss {float(loss):.6f} vs oracle {float(loss_o):.6f}; flat adapter gradient: norm deviation {norm_dev:.2e}, "
          f"1 - cosine {1 - cos:.2e}, relative error {rel_err(got, ref):.2e}")
    assert norm_dev < GRAD_NORM_BAR["fp16"] and 1 - cos < GRAD_COS_BAR["fp16"]
    losses = [float(tr.step(*args)) for _ in range(2)]
    torch.cuda.synchronize()
    tr.check_flags()
    assert all(math.isfinite(v) for v in losses) and tr.optimizer_counters() == (2, 0), (losses, tr.optimizer_counters())


def _gen_case():
    cfg = _cfg()
    return cfg, _weights(cfg), _batch(cfg, [600, 570], 600, SEED_GEN)


def test_generation_from_a_600_token_prompt(gpu):
    from oracle import generation as G

    dev = gpu["device"]
    cfg, weights, t = _gen_case()
    N, B = 8, 2
    m = _model(cfg, weights, dev)
    g = {k: v.to(dev) for k, v in t.items()}

    def gen(n, use_graph):
        out = m.mllm.generate_batch(g["vision_emb"], None, max_new_tokens=n, input_ids=g["input_ids"], attention_mask=g["attention_mask"],
                                    do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0, use_graph=use_graph)
        torch.cuda.synchronize()
        logits = m.mllm._ws.get("gen.logits", (B, cfg.llama.vocab), torch.float32, dev).cpu().clone()
        return out.cpu(), logits

    ids, _ = gen(N, False)
    ids_graph, _ = gen(N, True)
    m.mllm.check_flags()
    assert torch.equal(ids, ids_graph)
    step_logits = []
    for n in range(1, N + 1):  # the logits buffer holds the last step's: one run per step
        out_n, lg = gen(n, False)
        assert torch.equal(out_n, ids[:, :n])
        step_logits.append(lg)
    for b in range(B):
        n_text = int(t["attention_mask"][b].sum())
        seq = G.prefix_embeds(weights, cfg, t["vision_emb"], t["input_ids"], "fp16", b, n_text)
        for i in range(N):
            with torch.no_grad():
                ref = G.next_logits(weights, cfg, seq, "fp16")
            top = torch.topk(ref, 2)
            gap = float(top.values[0] - top.values[1])
            assert gap > 2 * LOGIT_BAR * float(ref.norm()), f"the oracle's own top-two gap at sample {b} step {i} is too small: {gap}"
            e = rel_err(step_logits[i][b], ref)
            print(f"[generation L={16 + n_text}] sample {b} step {i}: logits rel {e:.2e}, oracle gap {gap:.3f} (needs {2 * LOGIT_BAR * float(ref.norm()):.3f})")
            assert e < LOGIT_BAR, (b, i, e)
            assert int(top.indices[0]) == int(ids[b, i]), (b, i)
            seq = torch.cat([seq, G.token_embed(weights, ids[b, i], "fp16")[None, None]], dim=1)


def test_trajectory_model_refuses_560_before_any_launch(gpu):
    dev = gpu["device"]
    cfg = _cfg()
    m = _model(cfg, _weights(cfg), dev)
    small = {k: v.to(dev) for k, v in _batch(cfg, [40, 33], 40, 2).items()}
    long = {k: v.to(dev) for k, v in _batch(cfg, [544, 500], 544, 2).items()}

    def call(g):
        with torch.no_grad():
            return m(g["traj_emb"], g["vision_emb"], None, g["lane_polygon"], g["lane_polygon_len"], y=g["target_traj"],
                     norm_stat=g["norm_stat"], input_ids=g["input_ids"], attention_mask=g["attention_mask"], labels=g["labels"])

    call(small)
    torch.cuda.synchronize()
    ws = m.mllm._ws
    kv = ws.get("mm.kvlen", (2,), torch.int32, dev)
    kv.fill_(-7)
    n_before = m._n_forward
    with pytest.raises(ValueError, match="544") as ei:
        call(long)
    torch.cuda.synchronize()
    assert "lm_forward" in str(ei.value)
    assert bool((kv == -7).all()) and m._n_forward == n_before, "the refused call reached the MLLM pass"
    # the tokenizer branch (context_str alone): tokenised on the host first, so the same refusal comes before any launch
    from tcavt_amd import synth

    m.mllm.tokenizer = synth.SyntheticTokenizer(cfg.llama.vocab)

    def call_text(texts):
        g = small
        with torch.no_grad():
            return m(g["traj_emb"], g["vision_emb"], texts, g["lane_polygon"], g["lane_polygon_len"], y=g["target_traj"],
                     norm_stat=g["norm_stat"])

    with pytest.raises(ValueError, match="544"):
        call_text([" ".join(["car"] * 529), "a short one"])  # 16 + 529 = 545 rows
    torch.cuda.synchronize()
    assert bool((kv == -7).all()) and m._n_forward == n_before, "the refused tokenizer-branch call reached the MLLM pass"
    loss_t, dec_t = call_text([" ".join(["car"] * 528), "a short one"])  # 544 rows: runs
    torch.cuda.synchronize()
    assert torch.isfinite(loss_t).all() and torch.isfinite(dec_t).all() and m._n_forward == n_before + 1
    loss, dec = call({k: (v[:, :528] if k in ("input_ids", "attention_mask", "labels") else v) for k, v in long.items()})  # L = 544 still runs
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(dec).all()
