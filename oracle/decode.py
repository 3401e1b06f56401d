"""CPU ORACLE of ONE decode step over a KV cache (tcavt_llama_decode_step) -- TEST INFRASTRUCTURE ONLY.

oracle/generation.py re-runs the whole decoder on the growing sequence; this is the same arithmetic for the last position
alone, over keys / values that were computed before: what the HIP decode step computes, at the rounding points of
oracle/forward.py's contract (w, xn, t, qkv, p, att, act, res, emb, fh), in the dtype of its inputs -- float64 in the tests,
where every rounding point rounds to the storage type and comes back as float64.

    Wp = prepare(W, cfg, r)                                  # the weights as the kernels read them (gains folded, rounded once)
    logits, kv = decode_step(Wp, cfg, embeds, pos, k_cache, v_cache, r)

tests/test_decode_reference_cpu.py pins it against oracle.generation.next_logits.
"""
import math

import torch
import torch.nn.functional as F

from . import forward as O

_STORAGE = {"fp16": torch.float16, "bf16": torch.bfloat16}


def caster(r, dtype=torch.float64):
    """rd(t, tag): t rounded to the storage type of rounding point `tag` of contract r, returned in `dtype`"""
    r = O._rounder(r)

    def rd(t, tag=None):
        m = r.mode(tag)
        return t.to(dtype) if m == "fp32" else t.to(_STORAGE[m]).to(dtype)

    return rd


def prepare(W, cfg, r, dtype=torch.float64, weight_map=None):
    """The decoder's weights as the decode step reads them: the RMSNorm gains folded into the projections that follow (product
    in the weights' own precision, rounded once at "w"), the tied table at "emb".  weight_map(t16) -> tensor (optional): a
    further transformation of the rounded frozen matrices (q|k|v, o, gate, up, down and the lm_head's copy of the table) --
    e.g. FP8 quantisation and back; the adapters and the table of the token lookup stay as rounded."""
    W = O.as_torch(W)
    r = O._rounder(r)
    ll = cfg.llama
    wm = weight_map if weight_map is not None else (lambda t: t)

    def w16(t):  # rounded to the storage type of "w", in that type (fp32 contract: as is)
        m = r.mode("w")
        return t if m == "fp32" else t.to(_STORAGE[m])

    layers = []
    for li in range(ll.layers):
        P = f"{O.LLAMA}layers.{li}."
        g1, g2 = W[P + "input_layernorm.weight"], W[P + "post_attention_layernorm.weight"]
        d = {"wq": wm(w16(W[P + "self_attn.q_proj.weight"] * g1)), "wk": wm(w16(W[P + "self_attn.k_proj.weight"] * g1)),
             "wv": wm(w16(W[P + "self_attn.v_proj.weight"] * g1)), "wo": wm(w16(W[P + "self_attn.o_proj.weight"])),
             "wg": wm(w16(W[P + "mlp.gate_proj.weight"] * g2)), "wu": wm(w16(W[P + "mlp.up_proj.weight"] * g2)),
             "wd": wm(w16(W[P + "mlp.down_proj.weight"]))}
        if cfg.use_lora:
            d.update(aq=w16(W[P + "self_attn.q_proj.lora_A.weight"] * g1), av=w16(W[P + "self_attn.v_proj.lora_A.weight"] * g1),
                     bq=w16(W[P + "self_attn.q_proj.lora_B.weight"]), bv=w16(W[P + "self_attn.v_proj.lora_B.weight"]))
        layers.append({k: v.to(dtype) for k, v in d.items()})
    m = r.mode("emb")
    table = W[O.LLAMA + "embed_tokens.weight"]
    table16 = table if m == "fp32" else table.to(_STORAGE[m])
    return dict(layers=layers, g_final=W[O.LLAMA + "norm.weight"].to(dtype), table=table16.to(dtype), head=wm(table16).to(dtype),
                txt=W["mllm.text_modality_embedding"].reshape(-1).to(dtype))


def token_embeds(Wp, tok):
    """[B, H]: embed_tokens(id) + text_modality_embedding (generated tokens are text tokens)"""
    return Wp["table"][tok] + Wp["txt"]


def decode_step(Wp, cfg, embeds, pos, k_cache, v_cache, r):
    """embeds [B, H]: the new token's embedding; pos [B] (int64): its position = the number of keys in the cache;
    k_cache / v_cache: per layer [B, >= max(pos), nkv, hd], rows < pos[b] valid (values as stored).
    -> logits [B, V], [(k_new, v_new) per layer, each [B, nkv, hd]] (what the step appends at row pos[b])."""
    ll = cfg.llama
    r = O._rounder(r)
    dt = embeds.dtype
    rd = caster(r, dt)
    B, H = embeds.shape
    nq, nkv, hd = ll.n_q_heads, ll.n_kv_heads, ll.head_dim
    cos, sin = O.rope_tables(ll, int(pos.max()) + 1)
    cos, sin = cos[pos].to(dt)[:, None, :], sin[pos].to(dt)[:, None, :]  # [B, 1, hd / 2]: the sample's own position
    ss = r.stream_scale
    res = lambda x: rd(x * ss, "res") / ss

    def norm_parts(x):
        return rd(x * ss, "xn") / ss, torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + ll.rms_eps)

    def rot(t):
        t1, t2 = t[..., : hd // 2], t[..., hd // 2:]
        return torch.cat([t1 * cos - t2 * sin, t2 * cos + t1 * sin], dim=-1)

    h = res(embeds)
    new_kv = []
    for li, w in enumerate(Wp["layers"]):
        hb, rs = norm_parts(h)
        q, k, v = hb @ w["wq"].T, hb @ w["wk"].T, hb @ w["wv"].T
        if cfg.use_lora:
            s = O.lora_scale(cfg)
            tq = rd(ss * s * (hb @ w["aq"].T), "t") / ss
            tv = rd(ss * s * (hb @ w["av"].T), "t") / ss
            q = q + tq @ w["bq"].T
            v = v + tv @ w["bv"].T
        q = rd(rot((rs * q).view(B, nq, hd)), "qkv")
        k = rd(rot((rs * k).view(B, nkv, hd)), "qkv")
        v = rd((rs * v).view(B, nkv, hd), "qkv")
        new_kv.append((k, v))
        att = torch.zeros(B, nq, hd, dtype=dt)
        for b in range(B):
            n = int(pos[b])
            kb = torch.cat([k_cache[li][b, :n].to(dt), k[b][None]], 0).repeat_interleave(nq // nkv, dim=1)  # [n + 1, nq, hd]
            vb = torch.cat([v_cache[li][b, :n].to(dt), v[b][None]], 0).repeat_interleave(nq // nkv, dim=1)
            sc = torch.einsum("hd,jhd->hj", q[b], kb) / math.sqrt(hd)
            att[b] = torch.einsum("hj,jhd->hd", rd(torch.softmax(sc, dim=-1), "p"), vb)
        a = rd(att.reshape(B, nq * hd), "att")
        h = res(h + a @ w["wo"].T)
        hb2, rs2 = norm_parts(h)
        act = rd(F.silu(rs2 * (hb2 @ w["wg"].T)) * (rs2 * (hb2 @ w["wu"].T)), "act")
        h = res(h + act @ w["wd"].T)
    fh = O.rms_norm(h, Wp["g_final"], ll.rms_eps)
    return rd(fh, "fh") @ Wp["head"].T, new_kv
