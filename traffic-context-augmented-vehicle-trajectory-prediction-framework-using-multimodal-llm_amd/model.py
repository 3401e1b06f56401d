"""Host-side mirror of the reference's model classes over the gfx950 C ABI.

Same class names, constructor kwargs, ``forward()`` signatures and ``state_dict()`` key
layout as /root/reference/scripts/train.py:352-964 (no-LoRA key layout of
scripts/ablation_study_without_lora.py; LoRA adapters as ``...{q,v}_proj.lora_{A,B}.weight``),
so that train.py-style callers drop in.  Every module holds its parameters as fp32
``nn.Parameter``s on the GPU (torch = memory + streams) and computes exclusively through
``tcavt_amd.ops`` -> ``libtcavt_hip.so``; nothing here falls back to torch math.

Differences from the reference that are deliberate and documented in DESIGN.md:
  * ``from_pretrained`` fetches are replaced by an explicit ``LlamaShape`` (no network);
  * ``lm_head`` + cross-entropy of the reference's LLM call are not computed by the trajectory
    path (its caller keeps only ``hidden_states[-1]``, train.py:553).  The LM loss is opt-in:
    ``LlamaWithCrossAttnPEFT.forward(..., labels=...)`` and ``LlamaMultiModal.lm_forward`` fill
    ``outputs.loss`` from the fused kernel (csrc/lm_loss.hip); ``outputs.logits`` stays ``None``
    (the [B * L, V] logits are never stored);
  * the tokenizer branch of ``LlamaMultiModal.forward`` (train.py:556-575) runs when a tokenizer
    object is attached (``model.mllm.tokenizer``; none can be fetched offline) and raises
    ``NotImplementedError`` otherwise;
  * train-mode dropout draws its masks in-kernel from Philox (csrc/philox.hpp): same placement
    as the reference's dropout modules, not torch's random stream.
"""
import contextlib
import math
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import generation, ops, streams
from .config import LlamaShape, ModelConfig
from .layout import interleave_gate_up
from .rope import rope_tables


# --------------------------------------------------------------------------------------
# parameter holders (no compute; names reproduce the reference's state-dict keys)
# --------------------------------------------------------------------------------------
def _p(*shape):
    return nn.Parameter(torch.zeros(*shape, dtype=torch.float32))


class _Linear(nn.Module):
    def __init__(self, n_in, n_out, bias=True):
        super().__init__()
        self.weight = _p(n_out, n_in)
        if bias:
            self.bias = _p(n_out)
        else:
            self.register_parameter("bias", None)


class _Norm(nn.Module):
    def __init__(self, d, bias=True):
        super().__init__()
        self.weight = _p(d)
        if bias:
            self.bias = _p(d)


class _MHA(nn.Module):
    def __init__(self, e):
        super().__init__()
        self.in_proj_weight = _p(3 * e, e)
        self.in_proj_bias = _p(3 * e)
        self.out_proj = _Linear(e, e)


class _EncLayer(nn.Module):
    def __init__(self, d, ff, decoder=False):
        super().__init__()
        self.self_attn = _MHA(d)
        if decoder:
            self.multihead_attn = _MHA(d)
        self.linear1 = _Linear(d, ff)
        self.linear2 = _Linear(ff, d)
        self.norm1 = _Norm(d)
        self.norm2 = _Norm(d)
        if decoder:
            self.norm3 = _Norm(d)


class _LayerStack(nn.Module):
    def __init__(self, n, d, ff, decoder=False):
        super().__init__()
        self.layers = nn.ModuleList([_EncLayer(d, ff, decoder) for _ in range(n)])


class _Workspace:
    """Named scratch tensors, allocated once per (name, shape, dtype)."""

    def __init__(self):
        self._bufs = {}

    def get(self, name, shape, dtype, device, zero=False):
        """zero=True: zero-filled when first allocated (pad regions that kernels never write)."""
        key = (name, tuple(int(s) for s in shape), dtype)
        t = self._bufs.get(key)
        if t is None or t.device != device:
            t = (torch.zeros if zero else torch.empty)(key[1], dtype=dtype, device=device)
            self._bufs[key] = t
        return t


def _to16(t, dtype):
    """fp32 master -> packed 16-bit device copy in the module's storage type (fp16 by default, model.set_storage)."""
    return ops.cast16(t.detach().contiguous(), dtype=dtype)


XATTN_PAD = 64  # key counts of the head cross-attention are padded to a multiple of this
# Packed LoRA layout: a_cat [64, H] holds A_q in rows [0, r) and A_v in rows [LORA_V, LORA_V + r); b_ext [nqkv, 64] holds B_q in
# columns [0, r) of the q rows and B_v in columns [LORA_V, LORA_V + r) of the v rows; everything else is zero.  The two adapters
# sit in separate 16-column groups so that, with LoRA dropout on, each down-projection can be a GEMM of its own (N = 16) on its
# own dropped input -- PEFT gives every adapted Linear its own lora_dropout module (independent masks for q_proj and v_proj).
LORA_V = 16


class DropoutCtx:
    """Train-mode dropout bookkeeping for one forward pass: every dropout site of the reference
    (nn.Dropout / attention-weight dropout of nn.MultiheadAttention / LoRA dropout) gets its own site id,
    in call order, under one 64-bit seed; the kernels derive the mask from (seed, site, element index) with
    Philox4x32-10 (csrc/philox.hpp), so nothing is stored and a pass is reproducible from its seed."""

    def __init__(self, seed, first_site=0):
        self.seed, self.site = int(seed), int(first_site)

    def sub(self, block):
        """Site namespace of one module (block * 65536 + 1, ...): the numbering inside a module then does not depend
        on the order in which the modules are launched (side streams, Q-Former prefetch)."""
        return DropoutCtx(self.seed, first_site=block << 16)

    def spec(self, p):
        if p is None or p <= 0.0:
            return None
        self.site += 1
        return (float(p), self.seed, self.site)


def _spec(dctx, p):
    return dctx.spec(p) if dctx is not None else None


class _Prepared:
    """Mixin: lazily (re)build packed 16-bit device buffers derived from the parameters.

    `storage` is the 16-bit type of every GEMM operand the module keeps or produces: torch.float16 by default -- 11
    significant bits keep the whole model within 1e-3 of the fp32 reference (decoded 2.0e-4, ADE 7.7e-5, FDE 4.5e-4 at
    the full size against 2.6e-3 / 1.3e-3 / 7.4e-3 with bf16: profiles/r02_error_budget_full_size.json) at the same MFMA
    rate -- or torch.bfloat16 (the LoRA-trainable variant, whose backward kernels read bf16 tapes).  Accumulation,
    residual streams, norms, softmax and RoPE are fp32 either way."""
    storage = torch.float16

    def _invalidate(self):
        self._prep = None

    def _prepared(self):
        if getattr(self, "_prep", None) is None:
            with torch.no_grad():
                self._prep = self._prepare()
        return self._prep


# --------------------------------------------------------------------------------------
# generic post-LN transformer layers over the C ABI (nn.TransformerEncoder/DecoderLayer
# defaults: post-LN, ReLU, eval).  bf16=True: GEMMs in bf16 MFMA (Q-Former);
# bf16=False: everything fp32 (lane polygon encoder).
# --------------------------------------------------------------------------------------
def _prep_mha(m, bf16, split_kv=False, dt16=torch.float16):
    e = m.in_proj_weight.shape[1]
    cv = (lambda t: _to16(t, dt16)) if bf16 else (lambda t: t.detach().contiguous())
    d = SimpleNamespace(e=e, b_in=m.in_proj_bias.detach(), w_out=cv(m.out_proj.weight), b_out=m.out_proj.bias.detach())
    if split_kv:
        d.w_q, d.w_kv = cv(m.in_proj_weight[:e]), cv(m.in_proj_weight[e:])
        d.b_q, d.b_kv = m.in_proj_bias.detach()[:e].contiguous(), m.in_proj_bias.detach()[e:].contiguous()
    else:
        d.w_in = cv(m.in_proj_weight)
    return d


def _prep_layer(layer, bf16, decoder=False, dt16=torch.float16):
    cv = (lambda t: _to16(t, dt16)) if bf16 else (lambda t: t.detach().contiguous())
    d = SimpleNamespace(sa=_prep_mha(layer.self_attn, bf16, dt16=dt16), w1=cv(layer.linear1.weight), b1=layer.linear1.bias.detach(),
                        w2=cv(layer.linear2.weight), b2=layer.linear2.bias.detach(),
                        n1=layer.norm1, n2=layer.norm2)
    if decoder:
        d.ca = _prep_mha(layer.multihead_attn, bf16, split_kv=True, dt16=dt16)
        d.n3 = layer.norm3
    return d


class _TLayerRunner:
    """Runs post-LN layers on token matrices [M, D] (fp32 master copy x, bf16 shadow xb)."""

    def __init__(self, ws, bf16, nhead, tag, record=None, dctx=None, p_drop=0.0, dt16=torch.float16):
        self.ws, self.bf16, self.nhead, self.tag, self.dt16 = ws, bf16, nhead, tag, dt16
        self.dctx, self.p_drop = dctx, p_drop  # train-mode dropout of nn.Transformer*Layer (default 0.1)
        # training: `record` (a list) receives one dict of retained activations per encoder layer, and
        # `layer_tag` gives every layer its own buffers instead of recycling them
        self.record, self.layer_tag = record, ""
        self.specs = []  # dropout specs drawn by the layer being run, in call order (kept for the backward)

    def _draw(self):
        sp = _spec(self.dctx, self.p_drop)
        self.specs.append(sp)
        return sp

    def _gemm(self, a, w, **kw):
        if self.bf16:
            return ops.gemm_bf16(a, w, **kw)
        kw.pop("out_dtype", None)
        return ops.gemm_f32(a, w, **kw)

    def _buf(self, name, shape, dtype, dev):
        return self.ws.get(f"{self.tag}{self.layer_tag}.{name}", shape, dtype, dev)

    def self_attn(self, p, x, xb, B, L, key_len):
        """returns y = x + out_proj(MHA(x)) (fp32 [M, E])"""
        dev, E, M = x.device, p.e, x.shape[0]
        act_dt = self.dt16 if self.bf16 else torch.float32
        qkv = self._buf("qkv", (M, 3 * E), torch.float32, dev)
        self._gemm(xb if self.bf16 else x, p.w_in, out=qkv, bias=p.b_in, out_dtype=torch.float32)
        att = self._buf("att", (M, E), act_dt, dev)
        dh = E // self.nhead
        ops.mha(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], att, B, L, L, self.nhead, dh, 1.0 / math.sqrt(dh),
                key_len=key_len, ldq=3 * E, ldk=3 * E, ldv=3 * E, ldo=E, dropout=self._draw())
        y = self._buf("y", (M, E), torch.float32, dev)
        self._gemm(att, p.w_out, out=y, bias=p.b_out, residual=x, out_dtype=torch.float32,
                   dropout=self._draw())
        return y

    def cross_attn(self, p, x, xb, mem, memb, B, Lq, Lk):
        dev, E, M = x.device, p.e, x.shape[0]
        act_dt = self.dt16 if self.bf16 else torch.float32
        q = self._buf("cq", (M, E), torch.float32, dev)
        self._gemm(xb if self.bf16 else x, p.w_q, out=q, bias=p.b_q, out_dtype=torch.float32)
        kv = self._buf("ckv", (mem.shape[0], 2 * E), torch.float32, dev)
        self._gemm(memb if self.bf16 else mem, p.w_kv, out=kv, bias=p.b_kv, out_dtype=torch.float32)
        att = self._buf("catt", (M, E), act_dt, dev)  # (own buffers: a recording decoder layer keeps the self-attention's too)
        dh = E // self.nhead
        ops.mha(q, kv[:, :E], kv[:, E:], att, B, Lq, Lk, self.nhead, dh, 1.0 / math.sqrt(dh), ldq=E, ldk=2 * E,
                ldv=2 * E, ldo=E, dropout=self._draw())
        y = self._buf("cy", (M, E), torch.float32, dev)
        self._gemm(att, p.w_out, out=y, bias=p.b_out, residual=x, out_dtype=torch.float32,
                   dropout=self._draw())
        return y

    def norm(self, y, n, name):
        dev, (M, E) = y.device, y.shape
        x = self._buf(name, (M, E), torch.float32, dev)
        xb = self._buf(name + "b", (M, E), self.dt16, dev) if self.bf16 else None
        ops.layernorm(y, n.weight, n.bias, 1e-5, out_f32=x, out_bf16=xb)
        return x, xb

    def ffn(self, p, x, xb):
        dev, M = x.device, x.shape[0]
        ff = p.w1.shape[0]
        act_dt = self.dt16 if self.bf16 else torch.float32
        f = self._buf("ffh", (M, ff), act_dt, dev)
        self._gemm(xb if self.bf16 else x, p.w1, out=f, bias=p.b1, relu=True, out_dtype=act_dt,
                   dropout=self._draw())
        y = self._buf("y2", (M, x.shape[1]), torch.float32, dev)
        self._gemm(f, p.w2, out=y, bias=p.b2, residual=x, out_dtype=torch.float32, dropout=self._draw())
        return y

    def encoder_layer(self, p, x, xb, B, L, key_len=None, slot=0):
        y = self.self_attn(p.sa, x, xb, B, L, key_len)
        x1, x1b = self.norm(y, p.n1, f"x1_{slot}")
        y2 = self.ffn(p, x1, x1b)
        out = self.norm(y2, p.n2, f"x2_{slot}")
        specs, self.specs = self.specs, []
        if self.record is not None:
            M, E = x.shape
            dev = x.device
            self.record.append(dict(
                drop=specs,  # [attention weights, after out_proj, after ReLU, after linear2] or Nones
                x=x, xb=xb, y=y, x1=x1, x1b=x1b, y2=y2, qkv=self._buf("qkv", (M, 3 * E), torch.float32, dev),
                att=self._buf("att", (M, E), self.dt16 if self.bf16 else torch.float32, dev),
                f=self._buf("ffh", (M, p.w1.shape[0]), self.dt16 if self.bf16 else torch.float32, dev)))
        return out

    def run_stack(self, layers, x, xb, B, L, mem=None, memb=None, Lk=0, key_len=None, tag_fmt=None):
        """All `layers` (prepared encoder or decoder layers) in ONE C call (tcavt_tlayer_stack_forward, csrc/tlayers.hip): the
        launch sequence, buffers and dropout sites of encoder_layer / decoder_layer below, issued from C++.  Returns the last
        layer's (out, out16).  TCAVT_PY_TLAYERS=1 runs the per-layer Python composition instead (A/B, bit-identical)."""
        from . import capi

        decoder = mem is not None
        if os.environ.get("TCAVT_PY_TLAYERS", "0") == "1":
            for i, p in enumerate(layers):
                if self.record is not None and tag_fmt:
                    self.layer_tag = tag_fmt.format(i)
                x, xb = (self.decoder_layer(p, x, xb, mem, memb, B, L, Lk, slot=i & 1) if decoder else
                         self.encoder_layer(p, x, xb, B, L, key_len=key_len, slot=i & 1))
            return x, xb
        dev, (M, E) = x.device, x.shape
        a16 = self.dt16 if self.bf16 else torch.float32
        arr = (capi.TLayer * len(layers))()
        keep = [x, xb, mem, memb, key_len]
        first_site, recs = None, []
        x_in, xb_in = x, xb
        for i, p in enumerate(layers):
            if self.record is not None and tag_fmt:
                self.layer_tag = tag_fmt.format(i)
            slot = i & 1
            ff = p.w1.shape[0]
            n = "d" if decoder else "x"
            bufs = dict(qkv=self._buf("qkv", (M, 3 * E), torch.float32, dev), att=self._buf("att", (M, E), a16, dev),
                        y=self._buf("y", (M, E), torch.float32, dev), x1=self._buf(f"{n}1_{slot}", (M, E), torch.float32, dev),
                        ffh=self._buf("ffh", (M, ff), a16, dev), y2=self._buf("y2", (M, E), torch.float32, dev))
            last = f"d3_{slot}" if decoder else f"x2_{slot}"
            bufs["out"] = self._buf(last, (M, E), torch.float32, dev)
            if self.bf16:
                bufs["x1b"] = self._buf(f"{n}1_{slot}b", (M, E), self.dt16, dev)
                bufs["outb"] = self._buf(last + "b", (M, E), self.dt16, dev)
            if decoder:
                bufs.update(cq=self._buf("cq", (M, E), torch.float32, dev), ckv=self._buf("ckv", (mem.shape[0], 2 * E), torch.float32, dev),
                            catt=self._buf("catt", (M, E), a16, dev), cy=self._buf("cy", (M, E), torch.float32, dev),
                            x2=self._buf(f"d2_{slot}", (M, E), torch.float32, dev))
                if self.bf16:
                    bufs["x2b"] = self._buf(f"d2_{slot}b", (M, E), self.dt16, dev)
            w = dict(w_in=p.sa.w_in, b_in=p.sa.b_in, w_out=p.sa.w_out, b_out=p.sa.b_out, w1=p.w1, b1=p.b1, w2=p.w2, b2=p.b2,
                     n1_w=p.n1.weight, n1_b=p.n1.bias, n2_w=p.n2.weight, n2_b=p.n2.bias)
            if decoder:
                w.update(w_q=p.ca.w_q, b_q=p.ca.b_q, w_kv=p.ca.w_kv, b_kv=p.ca.b_kv, w_co=p.ca.w_out, b_co=p.ca.b_out,
                         n3_w=p.n3.weight, n3_b=p.n3.bias)
            for k_, t_ in list(bufs.items()) + list(w.items()):
                setattr(arr[i], k_, t_.data_ptr())
                keep.append(t_)
            specs = [self._draw() for _ in range(6 if decoder else 4)]  # the sites of this layer, in the kernels' call order
            self.specs = []
            if specs[0] is not None and first_site is None:
                first_site = specs[0]
            if self.record is not None:
                r = dict(drop=specs, x=x_in, xb=xb_in, y=bufs["y"], x1=bufs["x1"], x1b=bufs.get("x1b"), qkv=bufs["qkv"],
                         att=bufs["att"], f=bufs["ffh"])
                if decoder:
                    r.update(y2=bufs["cy"], x2=bufs["x2"], x2b=bufs.get("x2b"), y3=bufs["y2"], cq=bufs["cq"], ckv=bufs["ckv"],
                             catt=bufs["catt"])
                else:
                    r.update(y2=bufs["y2"])
                recs.append(r)
            x_in, xb_in = bufs["out"], bufs.get("outb")
        args = capi.TStackArgs()
        args.layers, args.n_layers = arr, len(layers)
        args.x, args.xb = x.data_ptr(), (xb.data_ptr() if xb is not None else None)
        if decoder:
            args.mem, args.memb = mem.data_ptr(), (memb.data_ptr() if memb is not None else None)
        args.key_len = key_len.data_ptr() if key_len is not None else None
        args.B, args.L, args.Lk, args.E, args.FF, args.nhead = B, L, Lk, E, layers[0].w1.shape[0], self.nhead
        args.dtype16 = (capi.F16 if self.dt16 == torch.float16 else capi.BF16) if self.bf16 else 0
        if first_site is not None:
            args.dropout_p, args.dropout_seed, args.first_site = first_site[0], first_site[1] & 0xFFFFFFFFFFFFFFFF, first_site[2]
        ops.tlayer_stack_forward(args)
        del keep
        if self.record is not None:
            self.record.extend(recs)
        return x_in, xb_in

    def decoder_layer(self, p, x, xb, mem, memb, B, Lq, Lk, slot=0):
        y = self.self_attn(p.sa, x, xb, B, Lq, None)
        x1, x1b = self.norm(y, p.n1, f"d1_{slot}")
        y2 = self.cross_attn(p.ca, x1, x1b, mem, memb, B, Lq, Lk)
        x2, x2b = self.norm(y2, p.n2, f"d2_{slot}")
        y3 = self.ffn(p, x2, x2b)
        specs, self.specs = self.specs, []
        out = self.norm(y3, p.n3, f"d3_{slot}")
        if self.record is not None:
            M, E = x.shape
            dev = x.device
            a16 = self.dt16 if self.bf16 else torch.float32
            self.record.append(dict(
                drop=specs,  # [self-attn weights, after its out_proj, cross-attn weights, after its out_proj, after ReLU, after linear2]
                x=x, xb=xb, y=y, x1=x1, x1b=x1b, y2=y2, x2=x2, x2b=x2b, y3=y3,
                qkv=self._buf("qkv", (M, 3 * E), torch.float32, dev), att=self._buf("att", (M, E), a16, dev),
                cq=self._buf("cq", (M, E), torch.float32, dev), ckv=self._buf("ckv", (mem.shape[0], 2 * E), torch.float32, dev),
                catt=self._buf("catt", (M, E), a16, dev), f=self._buf("ffh", (M, p.w1.shape[0]), a16, dev)))
        return out


# --------------------------------------------------------------------------------------
# LanePolygonEncoder (train.py:352-383) -- fp32 end to end (raw pixel inputs)
# --------------------------------------------------------------------------------------
class LanePolygonEncoder(nn.Module, _Prepared):
    def __init__(self, d_model=64, nhead=4, num_layers=2, max_points=64, dim_feedforward=2048):
        super().__init__()
        self.d_model, self.max_points, self.nhead = d_model, max_points, nhead
        self.input_proj = _Linear(2, d_model)
        self.encoder = _LayerStack(num_layers, d_model, dim_feedforward)
        self.pos_embedding = _p(1, max_points, d_model)
        self._ws = _Workspace()
        self._prep = None
        self.save_for_backward = False  # set by training.Trainer: keep per-layer activations
        self.saved = None
        self.dropout_p, self.dctx = 0.1, None  # nn.TransformerEncoderLayer default; dctx set per forward by the owner

    def _prepare(self):
        return [_prep_layer(l, bf16=False) for l in self.encoder.layers]

    def forward(self, polygon_batch, poly_len_list):
        B, P, _ = polygon_batch.shape
        dev, D = polygon_batch.device, self.d_model
        lens = poly_len_list if torch.is_tensor(poly_len_list) else torch.tensor(list(poly_len_list), dtype=torch.int32)
        lens = lens.to(device=dev, dtype=torch.int32).contiguous()
        keep = self.save_for_backward
        run = _TLayerRunner(self._ws, bf16=False, nhead=self.nhead, tag="poly", record=[] if keep else None,
                            dctx=self.dctx, p_drop=self.dropout_p)
        x = self._ws.get("poly.x0", (B * P, D), torch.float32, dev)
        polygon_batch = polygon_batch.contiguous()
        ops.poly_embed(polygon_batch, self.input_proj.weight, self.input_proj.bias,
                       self.pos_embedding[0, :P].contiguous(), x)
        x, _ = run.run_stack(self._prepared(), x, None, B, P, key_len=lens, tag_fmt=".L{}" if keep else None)
        emb = torch.empty((B, D), dtype=torch.float32, device=dev)
        ops.masked_mean(x, lens, emb, B, P, D)
        if keep:
            self.saved = SimpleNamespace(layers=run.record, lens=lens, polygon=polygon_batch, out=x, B=B, P=P)
        return emb


# --------------------------------------------------------------------------------------
# BlipQFormer (train.py:388-414) -- bf16 MFMA contractions, fp32 norms/softmax/residuals
# --------------------------------------------------------------------------------------
class BlipQFormer(nn.Module, _Prepared):
    def __init__(self, vision_dim=512, hidden_size=768, nhead=8, num_encoder_layers=4, num_decoder_layers=4,
                 num_query_tokens=16, dim_feedforward=2048):
        super().__init__()
        self.num_query_tokens, self.hidden_size, self.nhead = num_query_tokens, hidden_size, nhead
        self.vision_proj = _Linear(vision_dim, hidden_size)
        self.encoder = _LayerStack(num_encoder_layers, hidden_size, dim_feedforward)
        self.query_tokens = _p(num_query_tokens, hidden_size)
        self.decoder = _LayerStack(num_decoder_layers, hidden_size, dim_feedforward, decoder=True)
        self._ws = _Workspace()
        self._prep = None
        self.dropout_p, self.dctx = 0.1, None  # nn.Transformer*Layer default dropout
        self.save_for_backward = False  # training.Trainer(train_mllm_front=True): keep per-layer activations
        self.saved = None

    def _prepare(self):
        return SimpleNamespace(
            w_vp=_to16(self.vision_proj.weight, self.storage),
            enc=[_prep_layer(l, True, dt16=self.storage) for l in self.encoder.layers],
            dec=[_prep_layer(l, True, decoder=True, dt16=self.storage) for l in self.decoder.layers], q0={})

    def forward(self, vision_embs, return_bf16=False):
        B, Tv, Dv = vision_embs.shape
        dev, E, Nq = vision_embs.device, self.hidden_size, self.num_query_tokens
        P = self._prepared()
        keep = self.save_for_backward
        run = _TLayerRunner(self._ws, bf16=True, nhead=self.nhead, tag="qf", dctx=self.dctx, p_drop=self.dropout_p,
                            dt16=self.storage, record=[] if keep else None)
        vb = self._ws.get("qf.vb", (B * Tv, Dv), self.storage, dev)
        ops.cast16(vision_embs.contiguous().view(B * Tv, Dv), out=vb)
        x = self._ws.get("qf.x0", (B * Tv, E), torch.float32, dev)
        ops.gemm_bf16(vb, P.w_vp, out=x, bias=self.vision_proj.bias)
        xb = self._ws.get("qf.x0b", (B * Tv, E), self.storage, dev)
        ops.cast16(x, out=xb)
        x0, x0b = x, xb
        x, xb = run.run_stack(P.enc, x, xb, B, Tv, tag_fmt=".E{}" if keep else None)
        mem, memb = x, xb
        if B not in P.q0:  # learned queries broadcast over the batch (train.py:412); constant per B
            q = self.query_tokens.detach().unsqueeze(0).expand(B, -1, -1).reshape(B * Nq, E).contiguous()
            P.q0[B] = (q, ops.cast16(q, dtype=self.storage))
        q, qb = P.q0[B]
        q, qb = run.run_stack(P.dec, q, qb, B, Nq, mem=mem, memb=memb, Lk=Tv, tag_fmt=".D{}" if keep else None)
        if keep:
            ne = len(P.enc)
            self.saved = SimpleNamespace(enc=run.record[:ne], dec=run.record[ne:], vb=vb, x0=x0, x0b=x0b, mem=mem, memb=memb,
                                         out=q, outb=qb, B=B, Tv=Tv)
        out = q.view(B, Nq, E)
        return (out, qb) if return_bf16 else out


# --------------------------------------------------------------------------------------
# Llama decoder stack (HF LlamaForCausalLM layout) + LoRA on q_proj / v_proj
# --------------------------------------------------------------------------------------
class _LoraLinear(_Linear):
    def __init__(self, n_in, n_out, r):
        super().__init__(n_in, n_out, bias=False)
        if r:
            self.lora_A = _Linear(n_in, r, bias=False)
            self.lora_B = _Linear(r, n_out, bias=False)


class _LlamaAttn(nn.Module):
    def __init__(self, ll, r):
        super().__init__()
        H, hd = ll.hidden, ll.head_dim
        self.q_proj = _LoraLinear(H, ll.n_q_heads * hd, r)
        self.k_proj = _Linear(H, ll.n_kv_heads * hd, bias=False)
        self.v_proj = _LoraLinear(H, ll.n_kv_heads * hd, r)
        self.o_proj = _Linear(ll.n_q_heads * hd, H, bias=False)


class _LlamaMLP(nn.Module):
    def __init__(self, ll):
        super().__init__()
        self.gate_proj = _Linear(ll.hidden, ll.inter, bias=False)
        self.up_proj = _Linear(ll.hidden, ll.inter, bias=False)
        self.down_proj = _Linear(ll.inter, ll.hidden, bias=False)


class _LlamaLayer(nn.Module):
    def __init__(self, ll, r):
        super().__init__()
        self.self_attn = _LlamaAttn(ll, r)
        self.mlp = _LlamaMLP(ll)
        self.input_layernorm = _Norm(ll.hidden, bias=False)
        self.post_attention_layernorm = _Norm(ll.hidden, bias=False)


class _Embedding(nn.Module):
    def __init__(self, v, h):
        super().__init__()
        self.weight = _p(v, h)
        self.num_embeddings, self.embedding_dim = v, h


class _LlamaModel(nn.Module):
    def __init__(self, ll, r):
        super().__init__()
        self.embed_tokens = _Embedding(ll.vocab, ll.hidden)
        self.layers = nn.ModuleList([_LlamaLayer(ll, r) for _ in range(ll.layers)])
        self.norm = _Norm(ll.hidden, bias=False)


class _LlamaForCausalLM(nn.Module):
    def __init__(self, ll, r):
        super().__init__()
        self.model = _LlamaModel(ll, r)
        self.lm_head = _Linear(ll.hidden, ll.vocab, bias=False)
        self.lm_head.weight = self.model.embed_tokens.weight  # tied (public model card)
        self.config = SimpleNamespace(hidden_size=ll.hidden, vocab_size=ll.vocab, num_hidden_layers=ll.layers)

    def get_input_embeddings(self):
        return self.model.embed_tokens


class LlamaWithCrossAttnPEFT(nn.Module, _Prepared):
    """train.py:419-453.  ``base_model_name`` is kept for signature parity; the architecture
    comes from ``llama_shape`` (default Llama-3.2-1B) because nothing can be fetched here."""

    def __init__(self, base_model_name="meta-llama/Llama-3.2-1B", use_lora=True, lora_r=8, lora_alpha=32,
                 lora_dropout=0.1, llama_shape: LlamaShape = None):
        super().__init__()
        self.shape = llama_shape or LlamaShape()
        self.use_lora, self.lora_r, self.lora_alpha, self.lora_dropout = use_lora, lora_r, lora_alpha, lora_dropout
        self.llama_model = _LlamaForCausalLM(self.shape, lora_r if use_lora else 0)
        self.config = self.llama_model.config
        self.hidden_size = self.shape.hidden
        self.gemm_tile = 0
        self.timer = None  # optional ops.StackEvents: in-situ timing of the five big kernels of every layer (bench.py roofline leg)
        self.dctx = None   # DropoutCtx of the current forward (LoRA dropout on the adapter branch input)
        self._ws = _Workspace()
        self._prep = None
        self._rope = {}
        # LoRA-trainable variant (modify_scripts/modify_train.py:512-528; llm_backward.LoraBackward): when True the
        # decoder keeps, per layer, what the backward through the frozen layers needs (self.tape)
        self.save_for_backward = False
        self.tape = None
        self._prep_T = None
        # Scaled 16-bit image of the residual stream (tcavt_llama_stack_args.stream_scale): a power of two <= 1.  The 16-bit
        # stream (or the 16-bit copy of an fp32 stream) holds stream_scale * x, which moves the overflow limit of fp16 storage from
        # 65504 to 65504 / stream_scale at no cost in precision -- real checkpoints carry outlier channels far above the bulk
        # (MultiModalTrajectoryModel.set_storage("auto") picks it after a flagged first pass).  1.0: the plain contract.
        self.stream_scale = 1.0
        # fp16 operands with an fp32 residual stream (h != NULL in tcavt_llama_stack_args): the stream itself has no range limit,
        # its 16-bit copy is the only fp16 image (10 instead of 4 bytes per element through the residual epilogues)
        self.wide_stream = False
        # Opt-in MX8 MLP (mlp_weights, MultiModalTrajectoryModel.set_mlp_precision): "mx8" runs gate|up and down of every pass
        # without a tape on the block-scaled FP8 MFMA.  "fp16" (the default): the 16-bit kernels, bit for bit as before.
        self.mlp_precision = "fp16"
        self._prep_mx8 = None

    def set_stream_contract(self, stream_scale=1.0, wide_stream=False):
        """See stream_scale / wide_stream above.  Nothing is re-packed: with the stream's image at s x the whole q|k|v accumulator
        is s (x W^T + t B^T) -- the adapters' un-normalised t = lora_scale (s x) A^T simply stays at the stream's scale too --
        and the fused norm's row scale 1 / (s rms) takes the s out again."""
        self.stream_scale, self.wide_stream = float(stream_scale), bool(wide_stream)

    # ---- packed device-side weights -------------------------------------------------
    def _prepare(self):
        """16-bit packed copies for tcavt_llama_stack_forward.  The RMSNorm gains are FOLDED into the projections that
        follow them (fused RMSNorm: (x rs gamma) W^T == rs (x (W gamma)^T), csrc/stack.hip): W_qkv and the LoRA A
        matrices carry input_layernorm.weight, W_gateup carries post_attention_layernorm.weight; the product W * gamma
        is formed in fp32 and rounded once."""
        import ctypes

        from . import capi

        ll = self.shape
        nq, nkv, hd = ll.n_q_heads, ll.n_kv_heads, ll.head_dim
        layers = []
        to16 = lambda t: _to16(t, self.storage)
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        nL = len(self.llama_model.model.layers)
        a_all = b_all = g1_all = None
        carr = (capi.LlamaLayer * nL)()
        for li, lyr in enumerate(self.llama_model.model.layers):
            a = lyr.self_attn
            d = SimpleNamespace()
            d.g1, d.g2 = f32(lyr.input_layernorm.weight), f32(lyr.post_attention_layernorm.weight)
            d.w_qkv = to16(torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], dim=0).detach() * d.g1[None, :])
            if self.use_lora:
                r = self.lora_r
                if r > LORA_V:
                    raise ValueError(f"lora_r = {r}: the packed adapter layout holds ranks up to {LORA_V}")
                H = ll.hidden
                if a_all is None:
                    # all layers' packed adapters in two tensors, LAST layer first (the order of the trainer's flat
                    # parameter vector): refresh_lora() then re-packs every layer with a handful of strided copies
                    a_all = torch.zeros(nL, 64, H, dtype=self.storage, device=d.w_qkv.device)
                    b_all = torch.zeros(nL, (nq + 2 * nkv) * hd, 64, dtype=self.storage, device=d.w_qkv.device)
                    g1_all = torch.empty(nL, 1, H, dtype=torch.float32, device=d.w_qkv.device)
                d.a_cat, d.b_ext = a_all[nL - 1 - li], b_all[nL - 1 - li]
                g1_all[nL - 1 - li, 0].copy_(d.g1)
                d.a_cat[:r].copy_(a.q_proj.lora_A.weight.detach() * d.g1[None, :])
                d.a_cat[LORA_V:LORA_V + r].copy_(a.v_proj.lora_A.weight.detach() * d.g1[None, :])
                d.b_ext[: nq * hd, :r].copy_(a.q_proj.lora_B.weight.detach())
                d.b_ext[(nq + nkv) * hd:, LORA_V:LORA_V + r].copy_(a.v_proj.lora_B.weight.detach())
            d.w_o = to16(a.o_proj.weight)
            d.w_gu = to16(interleave_gate_up(lyr.mlp.gate_proj.weight.detach(), lyr.mlp.up_proj.weight.detach()) * d.g2[None, :])
            d.w_d = to16(lyr.mlp.down_proj.weight)
            c = carr[li]
            c.w_qkv, c.w_o, c.w_gu, c.w_d = d.w_qkv.data_ptr(), d.w_o.data_ptr(), d.w_gu.data_ptr(), d.w_d.data_ptr()
            if self.use_lora:
                c.a_cat, c.b_ext = d.a_cat.data_ptr(), d.b_ext.data_ptr()
            layers.append(d)
        return SimpleNamespace(layers=layers, g_final=f32(self.llama_model.model.norm.weight), carr=carr,
                               table=to16(self.llama_model.model.embed_tokens.weight), a_all=a_all, b_all=b_all,
                               g1_all=g1_all)

    def prepared_T(self):
        """Transposed 16-bit copies of the frozen weights: the `w` operands of the backward's dgrad GEMMs
        (g_in = g_out . W  ==  gemm_bf16(g_out, W^T stored [K_in, N_out])).  PLAIN weights, without the folded gains: the
        backward walks the un-fused graph (RMSNorm backward is its own kernel).  Built once; refresh_lora() keeps the
        adapter entries current."""
        if self._prep_T is None:
            P = self._prepared()
            ll = self.shape
            nq, nkv, hd, r = ll.n_q_heads, ll.n_kv_heads, ll.head_dim, self.lora_r
            to16 = lambda t: _to16(t, self.storage)
            tr = lambda w: to16(w.detach()).t().contiguous()
            nL = len(P.layers)
            at_all = bt_all = atq_all = atv_all = ap_all = None
            if self.use_lora:
                dev = P.a_all.device
                at_all = torch.zeros(nL, ll.hidden, 64, dtype=self.storage, device=dev)  # [layers (last first), H, 64]
                ap_all = torch.zeros(nL, 64, ll.hidden, dtype=self.storage, device=dev)  # plain a_cat (no folded gain)
                bt_all = P.b_all.transpose(1, 2).contiguous()                             # [layers (last first), 64, nqkv]
                # with LoRA dropout on, the two adapters' input gradients carry different masks: A_q^T and A_v^T alone
                # (the other adapter's columns zeroed), each the W operand of its own K = 64 product
                atq_all, atv_all = torch.zeros_like(at_all), torch.zeros_like(at_all)
            out = []
            for li, (d, lyr) in enumerate(zip(P.layers, self.llama_model.model.layers)):
                a = lyr.self_attn
                e = SimpleNamespace(w_qkv=tr(torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], dim=0)),
                                    w_o=tr(a.o_proj.weight), w_d=tr(lyr.mlp.down_proj.weight),
                                    w_gu=tr(interleave_gate_up(lyr.mlp.gate_proj.weight.detach(), lyr.mlp.up_proj.weight.detach())),
                                    a_cat=None, a_q=None, a_v=None, b_ext=None, a_plain=None)
                if self.use_lora:
                    k = nL - 1 - li
                    e.a_cat, e.a_q, e.a_v, e.b_ext, e.a_plain = at_all[k], atq_all[k], atv_all[k], bt_all[k], ap_all[k]
                out.append(e)
            self._prep_T = out
            self._prep_T_all = (at_all, bt_all, atq_all, atv_all, ap_all)
            if self.use_lora:
                self._refresh_lora_T()
        return self._prep_T

    def _refresh_lora_T(self, stacked=None):
        """The backward's adapter operands from the current parameters: plain A^T (no folded gain) and B^T."""
        at_all, bt_all, atq_all, atv_all, ap_all = self._prep_T_all
        P, r, nL = self._prepared(), self.lora_r, len(self._prepared().layers)
        if stacked is not None:  # all layers at once from the trainer's stacked views (last layer first, as ap_all is)
            ap_all[:, :r].copy_(stacked[0])
            ap_all[:, LORA_V:LORA_V + r].copy_(stacked[2])
        else:
            for li, lyr in enumerate(self.llama_model.model.layers):
                a, k = lyr.self_attn, nL - 1 - li
                ap_all[k, :r].copy_(a.q_proj.lora_A.weight.detach())
                ap_all[k, LORA_V:LORA_V + r].copy_(a.v_proj.lora_A.weight.detach())
        at_all.copy_(ap_all.transpose(1, 2))
        atq_all[:, :, :LORA_V].copy_(at_all[:, :, :LORA_V])
        atv_all[:, :, LORA_V:].copy_(at_all[:, :, LORA_V:])
        bt_all.copy_(P.b_all.transpose(1, 2))

    def _invalidate(self):
        self._prep_T = None
        self._prep_dec = None
        self._prep_dec8 = None
        self._prep_mx8 = None
        self._prep_tableT = None
        _Prepared._invalidate(self)

    # ---- LM loss on labels (opt-in: csrc/lm_loss.hip) ---------------------------------
    def table_T(self):
        """16-bit [H, V rounded up to 64] transpose of the tied table (zero beyond V): the LM loss backward's second
        operand.  A second copy of the table (525 MB at the Llama-3.2-1B shape), made on the first LM-loss backward and
        dropped with the packed weights it was made from, like the other transposed copies."""
        P = self._prepared()
        if getattr(self, "_prep_tableT", None) is None or self._prep_tableT[0] is not P:
            with torch.no_grad():
                self._prep_tableT = (P, ops.lm_table_t(P.table))
        return self._prep_tableT[1]

    def lm_loss(self, final16, labels, Nq, B, L, kv_len=None, flag=None):
        """Mean cross-entropy of the labelled rows (HF LlamaForCausalLM with ``labels``: row p predicts fused label p + 1,
        ignore_index -100, plain mean) from the 16-bit post-final-norm hidden states `final16` [>= B * L, H] and the tied
        16-bit table; labels int64 [B, L - Nq] (the image positions are unlabelled).  One fused pass: the logits are
        never stored.  Returns the state lm_loss_backward needs; .loss fp32 [1] and .count int32 [1] stay on the device
        (no host sync).  flag: int32 [1], set by the kernel on a label outside [0, V) or beyond kv_len."""
        P, ws, dev = self._prepared(), self._ws, final16.device
        V, H = P.table.shape
        wsb = ws.get("ll.lmloss.ws", (ops.lm_loss_workspace_bytes(B * L, V, H),), torch.uint8, dev)
        lse = ws.get("ll.lmloss.lse", (B * L,), torch.float32, dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        labels = labels.to(device=dev, dtype=torch.int64).contiguous()
        ops.lm_loss_forward(final16, P.table, labels, Nq, B, L, loss=loss, count=count, lse=lse, workspace=wsb, kv_len=kv_len,
                            flag=flag)
        return SimpleNamespace(loss=loss, count=count, lse=lse, h16=final16, labels=labels, Nq=Nq, B=B, L=L, kv_len=kv_len,
                               flag=flag, workspace=wsb)

    def lm_loss_backward(self, st, g_loss=None, out=None):
        """d loss / d (post-final-norm hidden states) as one bf16 [B * L, H] tensor -- what LoraBackward.run takes as
        g_final_a: (g_loss / N) (softmax(z) - onehot) table on labelled rows, zeros elsewhere.  g_loss: optional device
        fp32 [1] (absent: 1)."""
        P, dev = self._prepared(), st.h16.device
        H = P.table.shape[1]
        if out is None:
            out = self._ws.get("ll.lmloss.g_final", (st.B * st.L, H), torch.bfloat16, dev)
        return ops.lm_loss_backward(st.h16, P.table, self.table_T(), st.labels, st.Nq, st.B, st.L, lse=st.lse, count=st.count,
                                    g_out=out, workspace=st.workspace, g_loss=g_loss, kv_len=st.kv_len, flag=st.flag)

    def lm_eval(self, final16, labels, Nq, B, L, kv_len=None, flag=None):
        """Teacher-forced evaluation of the labelled rows in one fused pass (tcavt_lm_eval): the loss of lm_loss, bit for
        bit, plus the arg-max prediction of every labelled row and the per-sample sums -- the logits are never stored.
        Same arguments as lm_loss.  Returns fresh device tensors (no host sync): .loss fp32 [1], .count / .correct int32
        [1], .pred int32 [B * L] (-1 on unlabelled rows), .row_loss fp32 [B * L] (0 there), .sample_nll fp32 [B],
        .sample_tokens / .sample_correct int32 [B]."""
        P, ws, dev = self._prepared(), self._ws, final16.device
        V, H = P.table.shape
        wsb = ws.get("ll.lmeval.ws", (ops.lm_eval_workspace_bytes(B * L, V, H),), torch.uint8, dev)
        lse = ws.get("ll.lmloss.lse", (B * L,), torch.float32, dev)
        f32 = torch.empty(1 + B * L + B, dtype=torch.float32, device=dev)
        i32 = torch.empty(2 + B * L + 2 * B, dtype=torch.int32, device=dev)
        loss, row_loss, sample_nll = f32[:1], f32[1:1 + B * L], f32[1 + B * L:]
        count, correct, pred = i32[:1], i32[1:2], i32[2:2 + B * L]
        sample_tokens, sample_correct = i32[2 + B * L:2 + B * L + B], i32[2 + B * L + B:]
        labels = labels.to(device=dev, dtype=torch.int64).contiguous()
        ops.lm_eval(final16, P.table, labels, Nq, B, L, loss=loss, count=count, lse=lse, pred=pred, workspace=wsb,
                    row_loss=row_loss, correct=correct, sample_tokens=sample_tokens, sample_correct=sample_correct,
                    sample_nll=sample_nll, kv_len=kv_len, flag=flag)
        return SimpleNamespace(loss=loss, count=count, correct=correct, pred=pred, row_loss=row_loss, sample_nll=sample_nll,
                               sample_tokens=sample_tokens, sample_correct=sample_correct)

    def decode_weights(self, dtype="fp16"):
        """Fragment-major copies of the frozen projection weights and of the tied embedding table for the decode step of
        generate_batch (ops.pack_weight16; tcavt_decode_args.w_layout = W_FRAG16): one wave instruction of the weight stream
        then reads 1 KiB of consecutive bytes instead of 16 rows x 64 bytes -- 1.09 -> 0.91 ms per step at B = 8.  A second
        copy of the decoder's weights (2.47 GB at the Llama-3.2-1B shape), made on the first generation call and dropped with
        the packed weights it was made from; the adapters' small matrices are shared with the prefill's layer array.  Returns
        None (row-major weights) when a shape has no skinny form.

        dtype="fp8": the same copies as e4m3 codes with one power-of-two scale per row (ops.pack_weight8, quant.py; W_FRAG8) --
        half the bytes per step and half the extra memory (1.24 GB).  Quantised from the prepared 16-bit matrices, the norm
        gains already folded in: what the fp16 copies hold.  One cache per dtype, both dropped with the prepared weights."""
        from . import capi

        if dtype not in ("fp16", "fp8"):
            raise ValueError(f"decode_weights: dtype must be 'fp16' or 'fp8', got {dtype!r}")
        P = self._prepared()
        slot = "_prep_dec" if dtype == "fp16" else "_prep_dec8"
        pack = ops.pack_weight16 if dtype == "fp16" else ops.pack_weight8
        if getattr(self, slot, None) is not None and getattr(self, slot).of is P:
            return getattr(self, slot)
        ll = self.shape
        if ll.hidden % 256 or ll.inter % 256 or (ll.n_q_heads * ll.head_dim) % 256 or ll.vocab % 16:
            return None
        nL = len(P.layers)
        carr = (capi.LlamaLayer * nL)()
        keep = []
        with torch.no_grad():
            for li, d in enumerate(P.layers):
                ctypes_copy = P.carr[li]
                c = carr[li]
                for name, _ in capi.LlamaLayer._fields_:
                    setattr(c, name, getattr(ctypes_copy, name))
                pk = [pack(w) for w in (d.w_qkv, d.w_o, d.w_gu, d.w_d)]
                keep.append(pk)
                c.w_qkv, c.w_o, c.w_gu, c.w_d = (t.data_ptr() for t in pk)
            table = pack(P.table)
        setattr(self, slot, SimpleNamespace(of=P, carr=carr, table=table, keep=keep))
        return getattr(self, slot)

    def mlp_weights(self, dtype="mx8"):
        """MX8 images (ops.quant_mx8, quant.quantize_mx: e4m3 codes + one E8M0 scale per 32 elements along K) of the frozen gate|up
        and down matrices for the opt-in MX8 MLP, and a copy of the layer array that names them (tcavt_llama_layer.w_gu8 ...).
        Quantised from the prepared 16-bit matrices, the norm gain already folded in.  A second, 33/64-size copy of the MLP
        weights (0.83 GB at the Llama-3.2-1B shape), made on the first MX8 pass and dropped with the packed weights it was made
        from, like decode_weights."""
        from . import capi

        if dtype != "mx8":
            raise ValueError(f"mlp_weights: dtype must be 'mx8', got {dtype!r}")
        ll = self.shape
        if ll.hidden % 128 or ll.inter % 128:
            raise ValueError(f"mlp_weights: the MX8 MLP needs hidden and inter to be multiples of 128, got {ll.hidden} / {ll.inter}")
        P = self._prepared()
        if self._prep_mx8 is not None and self._prep_mx8.of is P:
            return self._prep_mx8
        carr = (capi.LlamaLayer * len(P.layers))()
        keep = []
        with torch.no_grad():
            for li, d in enumerate(P.layers):
                c = carr[li]
                for name, _ in capi.LlamaLayer._fields_:
                    setattr(c, name, getattr(P.carr[li], name))
                gu, d8 = ops.quant_mx8(d.w_gu), ops.quant_mx8(d.w_d)
                keep.append((gu, d8))
                c.w_gu8, c.w_gu8_scale, c.w_d8, c.w_d8_scale = gu[0].data_ptr(), gu[1].data_ptr(), d8[0].data_ptr(), d8[1].data_ptr()
        self._prep_mx8 = SimpleNamespace(of=P, carr=carr, keep=keep)
        return self._prep_mx8

    def refresh_lora(self, stacked=None):
        """Re-pack the adapter matrices (a_cat with the folded gain, b_ext, and the backward's transposes) from the
        lora_A / lora_B parameters after an optimizer step; the frozen base weights are left alone.  stacked = (A_q,
        B_q, A_v, B_v): views of ALL layers' parameters, last layer first ([layers, r, H] / [layers, out, r];
        training.Trainer builds them over its flat parameter vector) -- then the forward's re-pack is four strided
        copies instead of four per layer."""
        if not self.use_lora or self._prep is None:
            return
        ll, r = self.shape, self.lora_r
        nq, nkv, hd = ll.n_q_heads, ll.n_kv_heads, ll.head_dim
        P = self._prepared()
        if stacked is not None:
            aq, bq, av, bv = stacked
            P.a_all[:, :r].copy_(aq * P.g1_all)
            P.a_all[:, LORA_V:LORA_V + r].copy_(av * P.g1_all)
            P.b_all[:, : nq * hd, :r].copy_(bq)
            P.b_all[:, (nq + nkv) * hd:, LORA_V:LORA_V + r].copy_(bv)
        else:
            for li, lyr in enumerate(self.llama_model.model.layers):
                a, d = lyr.self_attn, P.layers[li]
                d.a_cat[:r].copy_(a.q_proj.lora_A.weight.detach() * d.g1[None, :])
                d.a_cat[LORA_V:LORA_V + r].copy_(a.v_proj.lora_A.weight.detach() * d.g1[None, :])
                d.b_ext[: nq * hd, :r].copy_(a.q_proj.lora_B.weight.detach())
                d.b_ext[(nq + nkv) * hd:, LORA_V:LORA_V + r].copy_(a.v_proj.lora_B.weight.detach())
        if self._prep_T is not None:
            self._refresh_lora_T(stacked)

    def _rope_tables(self, L, dev):
        key = (L, str(dev))
        if key not in self._rope:
            cos, sin = rope_tables(self.shape, L)
            self._rope[key] = (cos.to(dev), sin.to(dev))
        return self._rope[key]

    # ---- the hot loop -------------------------------------------------------------------
    def norm_inputs(self, M, dev):
        """(h16, part): the 16-bit copy of the residual stream and its rows' partial sums of squares [M, H / 64] -- what
        the fused RMSNorms read (written by tcavt_embed_fuse / ops.rownorm_prep for layer 0, by the residual epilogues
        afterwards)."""
        H = self.shape.hidden
        return (self._ws.get("ll.h16", (M, H), self.storage, dev), self._ws.get("ll.part", (M, H // 16), torch.float32, dev))

    @property
    def stream16(self):
        """16-bit residual stream (fp16 storage): no fp32 copy exists (tcavt_llama_stack_args.h == NULL).  Without a tape the
        stream lives in norm_inputs()[0] only and the residual epilogues add to it in place; with one (the LoRA-trainable
        variant) every epilogue writes the updated stream to its layer's own 16-bit buffer, which the backward reads --
        the forward arithmetic is the frozen path's either way.  bf16 storage (round 1's contract) keeps fp32 streams."""
        return self.storage == torch.float16 and not self.wide_stream

    def norm_npart(self, M):
        """Partials per row the first fused norm of a pass over M rows reads (what embed_fuse / rownorm_prep must write)."""
        return ops.norm_npart(M, self.shape.hidden, self.shape.inter)

    def decoder_stack(self, h, kv_len, B, L, out_f32=None, out_bf16=None, kv_cache=None, nonfinite_flag=None):
        """h: fp32 [B*L, H] residual stream (updated in place unless a tape is kept), or None with ``stream16`` (the stream
        is norm_inputs()[0]); norm_inputs() must have been filled; kv_len int32 [B].  One C call: tcavt_llama_stack_forward (csrc/stack.hip).  kv_cache = (k, v, lmax):
        16-bit [layers, B, lmax, nkv*64] tensors that receive the rotated keys / values (generation prefill); or the FP8 form
        (k_codes, k_scales, v_codes, v_scales, lmax): uint8 [layers, B, nkv, lmax, 64] codes and uint8 [layers, B, nkv, lmax, 2] scale
        bytes (quant.kv8_quantize of what the 16-bit form would hold; the stack's own output is the same either way)."""
        from . import capi

        ll, P, ws = self.shape, self._prepared(), self._ws
        dev, M, H = kv_len.device, B * L, ll.hidden
        if (h is None) != self.stream16:
            raise capi.TcavtError("decoder_stack: h must be None exactly when the 16-bit residual stream is in use (stream16)")
        nq, nkv, hd = ll.n_q_heads, ll.n_kv_heads, ll.head_dim
        nqkv = (nq + 2 * nkv) * hd
        if hd != 64:
            raise ValueError("the decoder kernels are built for head_dim 64")
        cos, sin = self._rope_tables(L, dev)
        h16, part = self.norm_inputs(M, dev)
        att = ws.get("ll.att", (M, nq * hd), self.storage, dev)
        act = ws.get("ll.act", (M, ll.inter), self.storage, dev)
        args = capi.LlamaStackArgs()
        keep = [cos, sin, h16, part, att, act, h, kv_len, out_f32, out_bf16]  # (tensors named by raw pointers below)
        dq = _spec(self.dctx, self.lora_dropout) if self.use_lora else None
        for _ in range(2 * ll.layers - 1 if dq is not None else 0):  # two sites per layer, numbered in layer order
            _spec(self.dctx, self.lora_dropout)
        tape = None
        carr = P.carr
        if self.save_for_backward:
            tape = self.tape = SimpleNamespace(layers=[], kv_len=kv_len, B=B, L=L, h_last=None)
            carr = (capi.LlamaLayer * ll.layers)()
            st_stream = self.storage if self.stream16 else torch.float32  # type of the per-layer residual streams
            h_in = h16 if self.stream16 else h  # (layer 0 reads the fused embeddings: the workspace's 16-bit stream / h)
            for li, d in enumerate(P.layers):
                # per-layer buffers instead of the shared ones: the residual stream is written to a new buffer by each
                # residual epilogue (no copies), q|k|v and the LoRA down-projection stay where the backward finds them
                dspec = None
                if dq is not None:
                    dspec = ((dq[0], dq[1], dq[2] + 2 * li), (dq[0], dq[1], dq[2] + 2 * li + 1))
                sv = SimpleNamespace(h_in=h_in, dspec=dspec,
                                     h_mid=ws.get(f"ll.sv.hmid{li}", (M, H), st_stream, dev),
                                     h_out=ws.get(f"ll.sv.hout{li}", (M, H), st_stream, dev),
                                     qkv_padded=ws.get(f"ll.sv.qkv{li}", (M + 64, nqkv), self.storage, dev, zero=True),
                                     gu=ws.get(f"ll.sv.gu{li}", (M, 2 * ll.inter), self.storage, dev),
                                     t=ws.get(f"ll.sv.t{li}", (M, 64), self.storage, dev, zero=True) if self.use_lora else None,
                                     # the attention's output and row log-sum-exp: one sweep over the keys in its backward
                                     att=ws.get(f"ll.sv.att{li}", (M, ll.n_q_heads * ll.head_dim), self.storage, dev),
                                     lse=ws.get(f"ll.sv.lse{li}", (B * ll.n_q_heads * L,), torch.float32, dev),
                                     # partial sums of squares of the layer's input stream: 1 / rms per token for the adapters'
                                     # weight gradients (the shared `part` is reused by the o_proj epilogue)
                                     part=ws.get(f"ll.sv.part{li}", (M, self.norm_npart(M)), torch.float32, dev))
                sv.qkv = sv.qkv_padded[:M]  # (the backward's score products read keys up to the next multiple of 64)
                tape.layers.append(sv)
                c, src = carr[li], P.carr[li]
                for f in ("w_qkv", "a_cat", "b_ext", "w_o", "w_gu", "w_d"):
                    setattr(c, f, getattr(src, f))
                c.tape_h_mid, c.tape_h_out = sv.h_mid.data_ptr(), sv.h_out.data_ptr()
                c.tape_qkv, c.tape_gu = sv.qkv_padded.data_ptr(), sv.gu.data_ptr()
                c.tape_att, c.tape_lse, c.tape_part = sv.att.data_ptr(), sv.lse.data_ptr(), sv.part.data_ptr()
                if self.use_lora:
                    c.tape_t = sv.t.data_ptr()
                h_in = sv.h_out
            tape.h_last = h_in
        else:
            qkv = ws.get("ll.qkv", (M, nqkv), self.storage, dev)
            args.qkv = qkv.data_ptr()
            keep.append(qkv)
        if self.mlp_precision == "mx8":  # opt-in MX8 MLP: no fallback -- what cannot run raises
            if self.save_for_backward:
                raise capi.TcavtError("decoder_stack: mlp_precision='mx8' cannot run with a tape (the LoRA-trainable backward reads "
                                      "16-bit pre-activations); set_mlp_precision('fp16') for training passes")
            if M <= 32:
                raise capi.TcavtError(f"decoder_stack: mlp_precision='mx8' needs more than 32 rows (B * L = {M})")
            carr = self.mlp_weights("mx8").carr
            kmax = max(H, ll.inter)
            mxc = ws.get("ll.mx8.codes", (M, kmax), torch.uint8, dev)
            mxs = ws.get("ll.mx8.scales", (M, kmax // 32), torch.uint8, dev)
            args.mx8_codes, args.mx8_scales = mxc.data_ptr(), mxs.data_ptr()
            keep += [mxc, mxs]
        if self.use_lora:
            t = ws.get("ll.lora_t", (M, 64), self.storage, dev, zero=True)
            args.t = t.data_ptr()
            keep.append(t)
            if dq is not None:  # (masks are applied inside tcavt_lora_down: no dropped copies of the stream)
                args.lora_dropout_p, args.dropout_seed, args.lora_first_site = dq[0], dq[1] & 0xFFFFFFFFFFFFFFFF, dq[2]
        args.layers = carr
        args.gamma_final, args.rope_cos, args.rope_sin = P.g_final.data_ptr(), cos.data_ptr(), sin.data_ptr()
        args.h = None if h is None else h.data_ptr()
        args.h16, args.part, args.kv_len = h16.data_ptr(), part.data_ptr(), kv_len.data_ptr()
        args.att, args.act = att.data_ptr(), act.data_ptr()
        if nonfinite_flag is not None:  # int32 [1]: 1 + 2 * layer (o_proj) / 2 + 2 * layer (down_proj) of the first non-finite epilogue
            if nonfinite_flag.dtype != torch.int32 or nonfinite_flag.numel() < 1:
                raise capi.TcavtError("decoder_stack.nonfinite_flag: int32 [1] required")
            args.nonfinite_flag = nonfinite_flag.data_ptr()
            keep.append(nonfinite_flag)
        for t_, nm, n_ in ((out_f32, "out_f32", M * H), (out_bf16, "out_bf16", M * H), (kv_len, "kv_len", B), (h, "h", M * H)):
            if t_ is not None and t_.numel() < n_:
                raise capi.TcavtError(f"decoder_stack.{nm}: buffer has {t_.numel()} elements, the stack needs {n_}")
        if out_f32 is not None:
            if out_f32.dtype != torch.float32:
                raise capi.TcavtError("decoder_stack.out_f32: fp32 required")
            args.out_f32 = out_f32.data_ptr()
        if out_bf16 is not None:
            if out_bf16.dtype != self.storage:
                raise capi.TcavtError(f"decoder_stack.out_bf16: {self.storage} required")
            args.out16 = out_bf16.data_ptr()
        if (h is not None and h.dtype != torch.float32) or kv_len.dtype != torch.int32:
            raise capi.TcavtError("decoder_stack: h fp32 and kv_len int32 required")
        if kv_cache is not None and len(kv_cache) == 5:
            kcod, ksc, vcod, vsc, lmax = kv_cache
            rows = ll.layers * B * nkv * lmax
            if any(t.dtype != torch.uint8 for t in (kcod, ksc, vcod, vsc)) or kcod.numel() < rows * 64 or vcod.numel() < rows * 64 or \
                    ksc.numel() < rows * 2 or vsc.numel() < rows * 2 or lmax < L:
                raise capi.TcavtError("decoder_stack.kv_cache: the FP8 form is four uint8 tensors, codes [layers, B, nkv, lmax, 64] and scale "
                                      "bytes [layers, B, nkv, lmax, 2] for keys and values, with lmax >= L")
            args.kv8_k_codes, args.kv8_k_scales = kcod.data_ptr(), ksc.data_ptr()
            args.kv8_v_codes, args.kv8_v_scales, args.kv_lmax = vcod.data_ptr(), vsc.data_ptr(), lmax
            keep += [kcod, ksc, vcod, vsc]
        elif kv_cache is not None:
            kc, vc, lmax = kv_cache
            need = ll.layers * B * lmax * nkv * hd
            if kc.dtype != self.storage or vc.dtype != self.storage or kc.numel() < need or vc.numel() < need or lmax < L:
                raise capi.TcavtError("decoder_stack.kv_cache: two 16-bit [layers, B, lmax, nkv*64] tensors with lmax >= L required")
            args.k_cache, args.v_cache, args.kv_lmax = kc.data_ptr(), vc.data_ptr(), lmax
        if self.timer is not None:
            args.events = self.timer.arr
        args.n_layers, args.B, args.L, args.H, args.I = ll.layers, B, L, H, ll.inter
        args.nq, args.nkv, args.dtype16 = nq, nkv, capi.F16 if self.storage == torch.float16 else capi.BF16
        args.gemm_tile = self.gemm_tile
        args.npart_in = self.norm_npart(M)
        args.rms_eps = ll.rms_eps
        args.lora_scale = (self.lora_alpha / self.lora_r) if self.use_lora else 0.0
        # few tokens (B * L <= 2048: 128 x 128 tiles of o / down leave CUs idle): workspace for the two-launch split K
        # (tcavt_llama_stack_args.splitk_ws; TCAVT_GEMM_NO_SPLITK2=1 switches it off in the library, A/B)
        if M <= 2048 and self.stream16 and dev.type == "cuda":
            skws = ws.get("ll.splitk", ((16 << 10) + 8 * 1024 * H * 4,), torch.uint8, dev, zero=True)
            args.splitk_ws, args.splitk_ws_bytes = skws.data_ptr(), skws.numel()
            keep.append(skws)
        if self.stream_scale != 1.0:
            if self.save_for_backward:
                raise capi.TcavtError("decoder_stack: the tape of the LoRA-trainable variant keeps the streams at scale 1 (stream_scale)")
            args.stream_scale = float(self.stream_scale)
        ops.llama_stack_forward(args)
        del keep

    def forward(self, inputs_embeds, attention_mask, labels=None, output_hidden_states=False):
        """HF-call-shaped entry (train.py:445-453).  ``hidden_states[-1]`` is produced; with ``labels`` (the FUSED labels
        [B, L], -100 on the image positions: train.py:536-552) ``.loss`` is the LM loss as a device fp32 scalar, from the
        fused lm_head + cross-entropy kernel (no host sync beyond the one this call already has).  ``.logits`` stays
        ``None``: the [B * L, V] logits are never stored."""
        B, L, H = inputs_embeds.shape
        dev = inputs_embeds.device
        if L > ops.ATTN_STREAM_MAX_L:  # (before anything is launched; tcavt_llama_stack_forward refuses it as well)
            from . import capi

            raise capi.TcavtError(f"LlamaWithCrossAttnPEFT: L={L} exceeds the decoder attention's limit of {ops.ATTN_STREAM_MAX_L}")
        if self.stream16:
            h = None
            ops.rownorm_prep(inputs_embeds.reshape(B * L, H).float().contiguous(), *self.norm_inputs(B * L, dev),
                             npart=self.norm_npart(B * L), rounded_sums=True, stream_scale=self.stream_scale)
        else:
            h = self._ws.get("ll.h", (B * L, H), torch.float32, dev)
            h.copy_(inputs_embeds.reshape(B * L, H))
            ops.rownorm_prep(h, *self.norm_inputs(B * L, dev), npart=self.norm_npart(B * L), stream_scale=self.stream_scale)
        kv_len = torch.empty(B, dtype=torch.int32, device=dev)
        flag = torch.zeros(2 if labels is not None else 1, dtype=torch.int32, device=dev)
        ops.mask_to_kvlen(attention_mask.to(torch.int64).contiguous(), 0, kv_len, flag[0:1])
        out = torch.empty((B * L, H), dtype=torch.float32, device=dev)
        loss = None
        if labels is None:
            self.decoder_stack(h, kv_len, B, L, out_f32=out)
        else:
            if tuple(labels.shape) != (B, L):
                raise ValueError(f"labels must be the fused labels [B, L] = {(B, L)} (-100 on the image positions)")
            out16 = self._ws.get("ll.lmloss.h16", (B * L, H), self.storage, dev)
            self.decoder_stack(h, kv_len, B, L, out_f32=out, out_bf16=out16)
            self.lm_state = self.lm_loss(out16, labels, 0, B, L, kv_len=kv_len, flag=flag[1:2])
            loss = self.lm_state.loss.reshape(())
        f = flag.tolist()
        if f[0]:
            raise ValueError("attention_mask must be right-padded (a prefix of ones per row)")
        if len(f) > 1 and f[1]:
            raise ValueError("labels contain ids outside [0, vocab) other than -100, or a label at or beyond a sample's valid length")
        hs = (None,) * self.shape.layers + (out.view(B, L, H),)
        return SimpleNamespace(loss=loss, logits=None, hidden_states=hs if output_hidden_states else None,
                               last_hidden_state=out.view(B, L, H))


# --------------------------------------------------------------------------------------
# LlamaMultiModal (train.py:459-575)
# --------------------------------------------------------------------------------------
GENERATION_CUTOFF_MARKER = "No right-following vehicle."


def cut_generated_text(text, marker=GENERATION_CUTOFF_MARKER):
    """Post-processing of generate_batch (scripts/train.py:645-653): everything after the first occurrence of the marker
    sentence is dropped, the marker itself is kept."""
    k = text.find(marker)
    return text if k < 0 else text[:k + len(marker)]


class LlamaMultiModal(nn.Module, _Prepared):
    def __init__(self, base_model_name="meta-llama/Llama-3.2-1B", use_lora=True, lora_r=8, lora_alpha=32,
                 lora_dropout=0.1, vision_dim=512, q_hidden_size=768, q_nhead=8, q_enc_layers=4, q_dec_layers=4,
                 q_num_query_tokens=16, llama_shape: LlamaShape = None, dim_feedforward=2048):
        super().__init__()
        self.qformer = BlipQFormer(vision_dim, q_hidden_size, q_nhead, q_enc_layers, q_dec_layers,
                                   q_num_query_tokens, dim_feedforward)
        self.q_hidden_size = q_hidden_size
        self.llama_wrapper = LlamaWithCrossAttnPEFT(base_model_name, use_lora, lora_r, lora_alpha, lora_dropout,
                                                    llama_shape)
        self.llama_hidden_size = self.llama_wrapper.hidden_size
        # the reference uses nn.Identity when the sizes agree (train.py:492-495); they never do here
        self.skip_f32_hidden = False  # training.Trainer (frozen-MLLM variant): see forward
        self.q_proj = _Linear(q_hidden_size, self.llama_hidden_size)
        self.vision_modality_embedding = _p(1, 1, self.llama_hidden_size)
        self.text_modality_embedding = _p(1, 1, self.llama_hidden_size)
        self.tokenizer = None  # no tokenizer files offline (train.py:500)
        self._ws = _Workspace()
        self._prep = None
        self._pf_stream = self._pf = self._img_consumed = None

    def _image_tokens(self, vision_embs):
        """Q-Former + q_proj (train.py:519-521): image tokens [B*Nq, H] fp32, before the modality embedding."""
        P = self._prepared()
        B = vision_embs.shape[0]
        _, imgb = self.qformer(vision_embs, return_bf16=True)
        self._imgb = imgb  # (the q_proj backward's activation)
        img = self._ws.get("mm.img", (B * self.qformer.num_query_tokens, self.llama_hidden_size), torch.float32,
                           vision_embs.device)
        ops.gemm_bf16(imgb, P.w_qp, out=img, bias=self.q_proj.bias)
        return img

    @staticmethod
    def _pf_key(t):
        return (t.data_ptr(), tuple(t.shape), t._version)

    def prefetch(self, vision_embs, ready=None, dctx=None):
        """Software pipelining across calls (optional; results are identical with or without it).  The Q-Former and
        q_proj are frozen and depend on nothing but `vision_embs`, yet they are ~50 small launches that leave the chip
        idle in front of every decoder pass.  `prefetch(next_vision_embs)` enqueues them on a side stream as soon as
        the image tokens of the pass in flight have been consumed, so they run underneath that pass's decoder GEMMs;
        the next forward() on the same tensor picks the result up instead of recomputing it.
        Contract: `vision_embs` is complete when this is called, or `ready` is a torch.cuda.Event marking its
        completion (the side stream does not wait for the caller's stream, that would serialise it behind the pass
        in flight).  In train mode `dctx` carries the dropout seed / site namespace the next forward will use for the
        Q-Former (MultiModalTrajectoryModel.prefetch supplies it)."""
        if vision_embs.device.type != "cuda" or (self.training and dctx is None):
            return
        if self._pf_stream is None:
            self._pf_stream = streams.side_stream(vision_embs.device, 2)
        s = self._pf_stream
        if ready is not None:
            s.wait_event(ready)
        if self._img_consumed is not None:
            s.wait_event(self._img_consumed)  # workspaces / image tokens of the previous pass are free
        tag = None if dctx is None else (dctx.seed, dctx.site)  # masks are a function of (seed, first site)
        with torch.cuda.stream(s), torch.no_grad():
            self.qformer.dctx = dctx
            self._image_tokens(vision_embs)
            done = torch.cuda.Event()
            done.record(s)
        self._pf = (self._pf_key(vision_embs), done, vision_embs, tag)

    def _prepare(self):
        return SimpleNamespace(w_qp=_to16(self.q_proj.weight, self.storage),
                               vis=self.vision_modality_embedding.detach().reshape(-1).contiguous(),
                               txt=self.text_modality_embedding.detach().reshape(-1).contiguous())

    def forward(self, vision_embs, context_str, input_ids=None, attention_mask=None, labels=None, return_bf16=False,
                out_slot=0):
        """out_slot (0 / 1): which of two 16-bit output buffers receives the final hidden states -- the pipelined decoder
        (MultiModalTrajectoryModel.pipeline_decoder) alternates them, the head of pass i still reads one while pass i + 1
        writes the other."""
        if input_ids is None or attention_mask is None:
            input_ids, attention_mask = self.tokenize_context(context_str, vision_embs.device)
            labels = None
        B, Lt = input_ids.shape
        dev, H, ws = vision_embs.device, self.llama_hidden_size, self._ws
        P = self._prepared()
        LW = self.llama_wrapper
        Nq = self.qformer.num_query_tokens
        L = Nq + Lt
        if L > ops.ATTN_STREAM_MAX_L:  # (before anything is launched; the decoder stack refuses it as well)
            raise ValueError(f"LlamaMultiModal: {Nq} image tokens + {Lt} text tokens = {L} rows exceed the decoder attention's "
                             f"limit of {ops.ATTN_STREAM_MAX_L}")
        pf, self._pf = self._pf, None
        want = self.qformer.dctx  # (train mode) the masks this forward must use; a prefetch made for them carries the same
        if pf is not None and pf[0] == self._pf_key(vision_embs) and \
                pf[3] == (None if want is None else (want.seed, want.site)):
            torch.cuda.current_stream().wait_event(pf[1])  # prefetched on the side stream (see prefetch)
            img = ws.get("mm.img", (B * Nq, H), torch.float32, dev)
        else:
            if pf is not None:  # a prefetch for some other tensor is in flight in the same workspaces
                torch.cuda.current_stream().wait_stream(self._pf_stream)
            img = self._image_tokens(vision_embs)
        h = None if LW.stream16 else ws.get("mm.h", (B * L, H), torch.float32, dev)
        # error flags: the kernels only ever SET them, so they accumulate over forwards until check_flags() reads and
        # clears them (evaluate_model and Trainer.check_flags do; one host sync, off the hot path)
        flags = ws.get("mm.flags", (3,), torch.int32, dev, zero=True)
        h16, part = LW.norm_inputs(B * L, dev)
        ops.embed_fuse(LW._prepared().table, input_ids.contiguous(), img, P.vis, P.txt, h, flags[0:1], h16=h16, part=part,
                       npart=LW.norm_npart(B * L), stream_scale=LW.stream_scale)
        if dev.type == "cuda" and self._pf_stream is not None:
            self._img_consumed = torch.cuda.Event()
            self._img_consumed.record()
        kv_len = ws.get("mm.kvlen", (B,), torch.int32, dev)
        ops.mask_to_kvlen(attention_mask.to(torch.int64).contiguous(), Nq, kv_len, flags[1:2])
        # 16-bit copy for the head's cross-attention; XATTN_PAD zeroed tail rows let its GEMMs run on key counts padded to a
        # multiple of 64 (TransformerLTSF.forward)
        final_b = ws.get("mm.finalb" if not out_slot else "mm.finalb1", (B * L + XATTN_PAD, H), self.storage, dev, zero=True)
        if self.skip_f32_hidden and return_bf16 and LW.stream16:
            # the head reads the 16-bit copy only: skip the fp32 hidden_states[-1] (67 MB written by the final norm on the
            # decoder's critical path); the 16-bit tensor stands in for it (shape carrier)
            final = final_b[: B * L].view(B, L, H)
            LW.decoder_stack(h, kv_len, B, L, out_bf16=final_b, nonfinite_flag=flags[2:3])
        else:
            final = torch.empty((B, L, H), dtype=torch.float32, device=dev)
            LW.decoder_stack(h, kv_len, B, L, out_f32=final.view(B * L, H), out_bf16=final_b, nonfinite_flag=flags[2:3])
        self._last_flags = flags
        if return_bf16:
            return final, Nq, final_b
        return final, Nq

    def tokenize_context(self, context_str, device):
        """The tokenizer branch (train.py:556-575): context_str alone, tokenised with padding + truncation (host work only,
        nothing is launched) -> (input_ids, attention_mask) on `device`."""
        if self.tokenizer is None or context_str is None:
            raise NotImplementedError(
                "the tokenizer branch (train.py:556-575) needs a tokenizer that cannot be fetched offline: attach one "
                "(model.tokenizer = ...) or pass input_ids/attention_mask as custom_collate_fn produces them")
        enc = self.tokenizer(context_str, return_tensors="pt", padding=True, truncation=True)
        return enc["input_ids"].to(device), enc["attention_mask"].to(device)

    def lm_forward(self, vision_embs, context_str, input_ids=None, attention_mask=None, labels=None):
        """The MLLM pass with the LM loss on `labels` [B, Lt] (what train.py:536-552 hands to the LLM as fused labels: the
        image positions are unlabelled, the last image token predicts the first text label).  Opt-in: forward() keeps
        ignoring labels.  Returns .loss (device fp32 scalar; NaN when no row is labelled, as torch), .n_tokens (device
        int32 [1]: labelled rows), .final_hidden [B, L, H], .final_hidden_bf16 and .num_image_tokens; .state is what
        llama_wrapper.lm_loss_backward takes.  A bad label sets a device flag that check_flags() reports."""
        if labels is None:
            raise ValueError("lm_forward needs labels (the LM loss is defined on them)")
        final, Nq, final_b = self.forward(vision_embs, context_str, input_ids=input_ids, attention_mask=attention_mask,
                                          return_bf16=True)
        B, L = final.shape[0], final.shape[1]
        dev = final_b.device
        self._lm_flag = self._ws.get("mm.lmflag", (1,), torch.int32, dev, zero=True)
        st = self.llama_wrapper.lm_loss(final_b[: B * L], labels, Nq, B, L, kv_len=self._ws.get("mm.kvlen", (B,), torch.int32, dev),
                                        flag=self._lm_flag)
        return SimpleNamespace(loss=st.loss.reshape(()), n_tokens=st.count, final_hidden=final, final_hidden_bf16=final_b,
                               num_image_tokens=Nq, state=st)

    def lm_evaluate(self, vision_embs, context_str, input_ids=None, attention_mask=None, labels=None):
        """Teacher-forced evaluation of the MLLM pass on `labels` [B, Lt]: lm_forward's loss (the same bits) plus the
        model's predictions, from one fused pass that never stores the logits.  Returns .loss / .n_tokens / .n_correct
        (device scalars), .pred int64 [B, Lt] aligned with `labels` (pred[b, j] is the arg-max of the row that predicts
        labels[b, j], row Nq + j - 1; -1 where labels[b, j] == -100), .row_loss fp32 [B, Lt] in the same alignment,
        .sample_nll fp32 [B], .sample_tokens / .sample_correct int32 [B], .final_hidden and .num_image_tokens.  Runs in
        whatever mode the model is in and never keeps a decoder tape.  A bad label sets the flag check_flags() reports."""
        if labels is None:
            raise ValueError("lm_evaluate needs labels (the predictions are scored against them)")
        LW = self.llama_wrapper
        was_saving, LW.save_for_backward = LW.save_for_backward, False
        try:
            final, Nq, final_b = self.forward(vision_embs, context_str, input_ids=input_ids, attention_mask=attention_mask,
                                              return_bf16=True)
        finally:
            LW.save_for_backward = was_saving
        B, L = final.shape[0], final.shape[1]
        dev = final_b.device
        self._lm_flag = self._ws.get("mm.lmflag", (1,), torch.int32, dev, zero=True)
        st = LW.lm_eval(final_b[: B * L], labels, Nq, B, L, kv_len=self._ws.get("mm.kvlen", (B,), torch.int32, dev),
                        flag=self._lm_flag)
        # labels[b, j] is predicted by row Nq + j - 1 (Nq >= 1: the last image row predicts the first text label)
        pred = st.pred.view(B, L)[:, Nq - 1:L - 1].to(torch.int64)
        row_loss = st.row_loss.view(B, L)[:, Nq - 1:L - 1].contiguous()
        return SimpleNamespace(loss=st.loss.reshape(()), n_tokens=st.count, n_correct=st.correct, pred=pred, row_loss=row_loss,
                               sample_nll=st.sample_nll, sample_tokens=st.sample_tokens, sample_correct=st.sample_correct,
                               final_hidden=final, num_image_tokens=Nq)

    def check_flags(self):
        """Host-side check of the device error flags accumulated since the last check (one sync); clears them."""
        if getattr(self, "_lm_flag", None) is not None and self._lm_flag.item():
            self._lm_flag.zero_()
            raise ValueError("labels contain ids outside [0, vocab) other than -100, or a label at or beyond a sample's valid length")
        if getattr(self, "_pool_flag", None) is not None and self._pool_flag.item():
            self._pool_flag.zero_()
            raise ValueError("generate_pool: a grouped admission named a slot outside the pool (tcavt_slot_admit_group)")
        if getattr(self, "_last_flags", None) is None:
            return
        f = self._last_flags.tolist()
        self._last_flags.zero_()
        if f[0]:
            raise ValueError("input_ids contains ids outside [0, vocab)")
        if f[1]:
            raise ValueError("attention_mask must be right-padded (a prefix of ones per row)")
        if len(f) > 2 and f[2]:
            layer, site = (f[2] - 1) // 2, ("o_proj" if (f[2] - 1) % 2 == 0 else "down_proj")
            raise FloatingPointError(
                f"non-finite value in the decoder's residual stream, first seen in the {site} epilogue of layer {layer}: a 16-bit "
                f"operand left the range of {self.storage} (|x| > {torch.finfo(self.storage).max:g}) at or before that layer, or the "
                "inputs were not finite (DESIGN.md, precision contract)")

    def generate_batch(self, vision_embs_batch, context_str_list=None, max_new_tokens=50, input_ids=None,
                       attention_mask=None, do_sample=True, temperature=0.9, top_k=40, top_p=0.9, repetition_penalty=1.2,
                       no_repeat_ngram_size=3, eos_token_id=None, pad_token_id=0, seed=0, use_graph=True, decode_weights="fp16",
                       kv_cache="fp16", stop_token_ids=None, stop_sequences=None, min_new_tokens=0, return_info=False,
                       poll_every=None, num_return_sequences=1, share_prefix=False, return_logprobs=False):
        """Autoregressive text generation (train.py:577-654; scripts/check_generation.py:152-222) on the HIP path.

        Same leading arguments as the reference; the prompt arrives as ``input_ids`` / ``attention_mask`` (right padded,
        as custom_collate_fn produces them) because no tokenizer can be fetched offline -- with ``self.tokenizer`` set,
        ``context_str_list`` is tokenised as the reference does and the result is decoded to strings.  Sampling defaults
        are the reference's (train.py:628-642); ``do_sample=False`` is greedy and bit-reproducible.

        Semantics (DESIGN.md "text generation"): prefix = [16 image tokens | the prompt's valid tokens]; every generated
        token is embedded as a text token (embed_tokens(id) + text_modality_embedding) at the sample's next position.
        Prefill = the ordinary batched decoder pass writing a KV cache; then one tcavt_llama_decode_step +
        tcavt_sample_logits per token, all state on the device, the step replayed as a hipGraph (use_graph).
        decode_weights="fp8" (opt-in): the decode step streams the FP8 copies of the frozen weights
        (LlamaWithCrossAttnPEFT.decode_weights) -- half the bytes per token; the prefill, the activations and the KV cache
        stay 16-bit.  It needs the skinny path (B <= 32, a shape with a skinny form, no TCAVT_DECODE_ROWMAJOR=1) and raises
        where that cannot run: there is no fallback.
        kv_cache="fp8" (opt-in, independent of decode_weights): the KV cache is kept in the "KV8" format (quant.kv8_quantize: e4m3
        codes with one power-of-two scale per 32 elements of a head's row, head-major planes) -- 66 instead of 128 bytes per cached
        row and kv head.  The prefill itself is unchanged (its attention reads the 16-bit q|k|v; only the store into the cache
        quantises, tcavt_kv_store8), so the first generated token does not depend on the cache type; every decode step uses its
        own key / value at 16-bit precision, writes them quantised and sees every earlier row as code * 2^k (tcavt_attn_decode8).
        Any other value raises ValueError.
        Ending rules ("ending rules"; stopping.StopRules validates them and raises ValueError): a row also ends
        on a token of ``stop_token_ids`` (kept, like EOS) or when its last generated tokens equal one of ``stop_sequences`` (<= 16
        of 1 .. 8 ids; never matched across the end of the prompt); while fewer than ``min_new_tokens`` tokens are out, EOS and the
        stop tokens are banned (it needs one of the two).  With none of them set the sampler launches are those of a call without.
        ``poll_every`` = k >= 1: after every k replayed steps the finished flags are read back ([B] int32 to pinned memory, an event
        wait) and the loop ends once every row has: same tokens, fewer steps.  None: no host read, all max_new_tokens - 1 steps.
        ``return_info``: returns (out, info) -- info["finish_reason"] / info["n_generated"]: host int32 [B] (1 EOS, 2 stop token,
        3 stop sequence, 4 ran out at max_new_tokens), info["steps"]: decode steps run.
        ``num_return_sequences`` = n (an int >= 1; anything else raises ValueError): n continuations per prompt from ONE prefill
        ("n continuations per prompt").  The Q-Former, the embedding, the decoder stack and the lm_head run at
        B rows into a cache of the prompt's own 16 + Lt rows; one tcavt_kv_fanout launch copies every prompt's cache rows and first
        logits to its n decode rows and sets their state; token selection and the decode loop then run at B * n rows exactly as
        above (graph, poll_every, ending rules, return_info).  The result has B * n rows, row b * n + j being continuation j of
        prompt b -- the order of ``repeat_interleave(n)`` -- and the info arrays have length B * n.  Row b * n + j draws from Philox
        sample index b * n + j, the index the same row has in a call on the prompts repeated n times.  ``do_sample=False`` with
        n > 1 is allowed and yields n identical rows per prompt.  ``decode_weights="fp8"`` needs B * n <= 32.  n = 1, the default,
        is launch for launch the call without the argument.  generate_pool does not take it.
        ``share_prefix`` = True (opt-in; a bool, anything else raises ValueError; any n >= 1): the prompts' cache stays where the
        prefill wrote it (``gen.src.*``, B x (16 + Lt) rows, never written again) and every decode step reads it in place:
        tcavt_attn_decode_shared fetches a prompt row once per (prompt, kv head, 32 queries) for all n continuations, where the
        default reads n copies of it once per row and head.  One tcavt_state_fanout sets the rows' state and first logits (no
        cache copy), and the decode rows own a suffix cache of max_new_tokens - 1 rows (``gen.sfx.*``).  Row order, Philox rows,
        ending rules, poll_every, return_info, the graph and ``decode_weights`` are as above; the attention's summation order
        differs from the default's, so tokens can differ where two logits are within rounding of each other.  It needs the 16-bit
        cache: with ``kv_cache="fp8"`` it raises ValueError.  generate_pool does not take it.
        ``return_logprobs`` = True (opt-in; a bool, anything else raises ValueError): returns (out, info) and info gains the host
        tensors "token_logprobs" float32 [B * n, max_new_tokens], "sum_logprob" float32 [B * n] and "n_scored" int32 [B * n]
        ("log-probabilities").  token_logprobs[row, i] = log_softmax(raw)[out[row, i]] for every token the
        row emitted, the ending token included, where raw is the fp32 logits row as the lm_head wrote it -- before the repetition
        penalty, the bans, the temperature and top-k / top-p: the model's distribution, independent of the sampling arguments
        (HF: output_logits=True, log_softmax, gather).  Entries after a row's end are 0.0; sum_logprob is their fp32 sum in step
        order, n_scored their number.  Two small launches (tcavt_logprob_begin / _finish) bracket every token selection, in the
        captured step too; the tokens, the sampler entry chosen and every other launch are those of the call without the flag.
        generation.rank_continuations orders the n continuations of a prompt by it.
        Returns int64 [B * n, max_new_tokens] token ids (pad_token_id after a row's end), or a list of B * n strings in the same
        order with a tokenizer."""
        out, info = generation.generate_batch(
            self, vision_embs_batch, context_str_list, max_new_tokens, input_ids, attention_mask, do_sample, temperature, top_k,
            top_p, repetition_penalty, no_repeat_ngram_size, eos_token_id, pad_token_id, seed, use_graph, decode_weights, kv_cache,
            stop_token_ids, stop_sequences, min_new_tokens, return_info, poll_every, num_return_sequences, share_prefix,
            return_logprobs)
        res = self._generated_texts(out)
        return (res, info) if return_info or return_logprobs else res

    def _generated_texts(self, out):
        """Token ids as they are without a tokenizer; with one, the decoded strings, cut as the reference cuts them."""
        if self.tokenizer is None:
            return out
        return [cut_generated_text(self.tokenizer.decode(row, skip_special_tokens=True)) for row in out.tolist()]

    def generate_pool(self, vision_embs, input_ids, attention_mask, max_new_tokens=128, slots=8, poll_every=1, do_sample=True,
                      temperature=0.9, top_k=40, top_p=0.9, repetition_penalty=1.2, no_repeat_ngram_size=3, eos_token_id=None,
                      pad_token_id=0, seed=0, use_graph=True, decode_weights="fp16", kv_cache="fp16", admit_group=1,
                      stop_token_ids=None, stop_sequences=None, min_new_tokens=0, return_info=False, return_logprobs=False):
        """Text generation over a LIST of R requests on a fixed pool of ``slots`` decode slots ("slot
        pool"): request r is served exactly once, first in first out, and the moment a request ends (EOS, or its budget) the
        next one of the queue is prefilled into its slot -- no decode row computes pad tokens for longer than one poll interval.
        ``vision_embs`` [R, ...], ``input_ids`` / ``attention_mask`` [R, Lt] right padded; ``max_new_tokens``: an int, or one
        budget >= 1 per request.  Sampling arguments, ``decode_weights`` and ``kv_cache`` as in generate_batch (fp8 weights:
        slots <= 32).  Request r draws from Philox row r and writes output row r, and it is prefilled on its own (the ordinary
        decoder pass at B = 1, then tcavt_slot_admit), so its tokens do not depend on what else is running or on its slot.
        The decode loop is ``poll_every`` steps (tcavt_llama_decode_step at B = slots + tcavt_sample_logits_slots, one captured
        hipGraph with ``use_graph``), then one [slots] int32 copy of the finished flags to pinned host memory and an event wait,
        then the refills (poll_every = 1 measured best of 1 / 8 / 32, profiles/generate_pool.txt); the very first step runs eagerly and unpolled (the kernels' warm-up, then the capture).  A finished or idle slot is inert: it re-runs the step on the pad token at a frozen position.
        Returns int64 [R, max budget] (pad_token_id after each request's end), or strings with a tokenizer; check_flags()
        works afterwards as after generate_batch.  ``self.pool_stats`` of the last call: "steps" (decode steps run), "admitted" and
        "retired" [(request, slot, steps run by then)] -- retirement is seen at a poll, up to poll_every steps after the end.
        ``admit_group`` = G (1 <= G <= slots; anything else raises ValueError): G = 1, the default, is the path above.  G >= 2:
        requests are admitted in groups of up to G (pool.SlotScheduler.admission_groups: a group goes when min(G, waiting requests)
        slots are free) and EVERY admission is one decoder pass at exactly B = G rows -- Q-Former, embedding, stack,
        tcavt_slot_admit_group, lm_head, tcavt_sample_logits_rows -- a short group being filled with pad rows (the group's first
        request again, admitted nowhere).  M = G * L is then constant, so every kernel form is, and with ``use_graph`` the pass is
        captured after its first, eager run and replayed for every later group (only the staging buffers pool.pg.* change).
        Contract: for a FIXED G a request's tokens do not depend on the schedule, the slot, its row in the group, its partners or
        the pad rows; they may differ from its tokens at another G, admit_group = 1 included, because the kernel forms differ with
        M.  Measured on 256 requests (profiles/generate_pool_groups.txt): at 32 slots G = 2 / 4 / 8 serve the list in 1.22 / 1.02 /
        0.99 s against 1.57 s at G = 1 and 1.23 s for generate_batch; at 8 slots in 2.75 / 2.83 / 3.43 s against 2.95 s (G = 8 loses).
        Recommended: admit_group=4 (it wins at both sizes); G = 2 for small pools, G = 8 from 32 slots on.  The default stays 1.
        ``self.pool_stats["groups"]``: [(requests, slots, steps run by then)] per group pass, in row order (empty at G = 1).
        ``stop_token_ids``, ``stop_sequences``, ``min_new_tokens``: the ending rules of generate_batch, applied by all three sampler
        uses (the decode loop, the G = 1 admission, the grouped admission); a request may end on its first token, at admission.
        With none set the sampler launches are those of a call without.  With rules or ``return_info`` the stats gain
        "finish_reason" / "n_generated": host int32 [R] (1 EOS, 2 stop token, 3 stop sequence, 4 budget); ``return_info`` returns
        (out, stats).
        ``return_logprobs`` = True (a bool, anything else raises ValueError): returns (out, stats) and the stats gain the host tensors
        "token_logprobs" float32 [R, max budget], "sum_logprob" float32 [R] and "n_scored" int32 [R], as in generate_batch: the
        log-softmax of the raw logits row at every token request r emitted, 0.0 after its end.  The bracket sits around all three
        sampler uses, and a request's three results do not depend on its slot, the schedule or its partners (for a fixed G)."""
        out, stats = generation.generate_pool(
            self, vision_embs, input_ids, attention_mask, max_new_tokens, slots, poll_every, do_sample, temperature, top_k, top_p,
            repetition_penalty, no_repeat_ngram_size, eos_token_id, pad_token_id, seed, use_graph, decode_weights, kv_cache,
            admit_group, stop_token_ids, stop_sequences, min_new_tokens, return_info, return_logprobs)
        res = self._generated_texts(out)
        return (res, stats) if return_info or return_logprobs else res


# --------------------------------------------------------------------------------------
# LTSF blocks (train.py:659-842)
# --------------------------------------------------------------------------------------
class SelfAttentionBlock(nn.Module):
    def __init__(self, embed_dim, nhead=1, dropout_rate=0.1):
        super().__init__()
        self.embed_dim, self.nhead = embed_dim, nhead
        self.norm1 = _Norm(embed_dim)
        self.mha = _MHA(embed_dim)
        self.ffn = nn.ModuleList([_Linear(embed_dim, embed_dim * 4), nn.Identity(), nn.Identity(),
                                  _Linear(embed_dim * 4, embed_dim)])
        self.norm2 = _Norm(embed_dim)
        self._ws = _Workspace()
        self.dropout_p, self.dctx = dropout_rate, None

    def forward_tokens(self, tok, B, T):
        """tok fp32 [B*T, E] (batch-first tokens) -> [B*T, E].  Residuals start from the NORMED
        tensors exactly as train.py:677-684."""
        dev, E, ws = tok.device, self.embed_dim, self._ws
        M = B * T
        xn = ws.get("sab.xn", (M, E), torch.float32, dev)
        ops.layernorm(tok, self.norm1.weight, self.norm1.bias, 1e-5, out_f32=xn)
        qkv = ws.get("sab.qkv", (M, 3 * E), torch.float32, dev)
        ops.gemm_f32(xn, self.mha.in_proj_weight, out=qkv, bias=self.mha.in_proj_bias)
        att = ws.get("sab.att", (M, E), torch.float32, dev)
        dh = E // self.nhead
        dc, pd = self.dctx, self.dropout_p
        # the four dropout sites of the block, in call order; kept for the backward (same masks on the gradients)
        self.drop_specs = sp = [_spec(dc, pd) for _ in range(4)]
        ops.mha(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], att, B, T, T, self.nhead, dh, 1.0 / math.sqrt(dh),
                ldq=3 * E, ldk=3 * E, ldv=3 * E, ldo=E, dropout=sp[0])
        res1 = ws.get("sab.res1", (M, E), torch.float32, dev)
        ops.gemm_f32(att, self.mha.out_proj.weight, out=res1, bias=self.mha.out_proj.bias, residual=xn, dropout=sp[1])
        rn = ws.get("sab.rn", (M, E), torch.float32, dev)
        ops.layernorm(res1, self.norm2.weight, self.norm2.bias, 1e-5, out_f32=rn)
        f = ws.get("sab.f", (M, 4 * E), torch.float32, dev)
        ops.gemm_f32(rn, self.ffn[0].weight, out=f, bias=self.ffn[0].bias, relu=True, dropout=sp[2])
        out = ws.get("sab.out", (M, E), torch.float32, dev)
        ops.gemm_f32(f, self.ffn[3].weight, out=out, bias=self.ffn[3].bias, residual=rn, dropout=sp[3])
        return out

    def forward(self, x):
        """x (B, E, T) -> (B, E, T), the reference's layout (train.py:674-686)."""
        B, E, T = x.shape
        tok = x.permute(0, 2, 1).contiguous().view(B * T, E)
        return self.forward_tokens(tok, B, T).view(B, T, E).permute(0, 2, 1).contiguous()


class LTSF_NLinearEncoder(nn.Module):
    def __init__(self, window_size, individual, d_model):
        super().__init__()
        if not individual:
            raise NotImplementedError("only individual=True is on the hot path (train.py:1103)")
        self.window_size, self.individual, self.channels = window_size, individual, d_model
        self.encoder_linears = nn.ModuleList([_Linear(window_size, window_size) for _ in range(d_model)])


class LTSF_NLinearDecoder(nn.Module):
    def __init__(self, window_size, forecast_size, individual, d_model, polygon_embed_dim=64, use_post_mlp=True,
                 post_mlp_hidden_dim=64, post_mlp_output_dim=None, dropout_rate=0.1, cross_dim=768, cross_nhead=2,
                 output_feature_dim=2):
        super().__init__()
        if not individual:
            raise NotImplementedError("only individual=True is on the hot path (train.py:1103)")
        self.window_size, self.forecast_size, self.channels = window_size, forecast_size, d_model
        self.use_post_mlp, self.cross_dim, self.cross_nhead = use_post_mlp, cross_dim, cross_nhead
        self.decoder_linears = nn.ModuleList([_Linear(window_size, forecast_size) for _ in range(d_model)])
        self.lane_fc = _Linear(polygon_embed_dim, d_model * forecast_size)
        if post_mlp_output_dim is None:
            post_mlp_output_dim = d_model * forecast_size
        if use_post_mlp:
            self.post_mlp = nn.ModuleList([_Linear(d_model * forecast_size, post_mlp_hidden_dim), nn.Identity(),
                                           nn.Identity(), _Linear(post_mlp_hidden_dim, post_mlp_output_dim)])
        self.cross_attn = _MHA(cross_dim)
        self.dec_proj = _Linear(d_model, cross_dim)
        self.dec_unproj = _Linear(cross_dim, d_model)
        self.fusion_layer = nn.ModuleList([_Norm(d_model), _Linear(d_model, d_model), nn.Identity(),
                                           _Linear(d_model, d_model)])
        self.out_proj = _Linear(d_model, output_feature_dim)


class TransformerLTSF(nn.Module, _Prepared):
    def __init__(self, seq_len, out_len, individual, feature_size, d_model, polygon_embed_dim=64, use_post_mlp=True,
                 post_mlp_hidden_dim=64, post_mlp_output_dim=None, nhead=1, dropout_rate=0.1, cross_dim=768,
                 cross_nhead=2, output_feature_dim=2):
        super().__init__()
        self.seq_len, self.out_len, self.d_model, self.feature_size = seq_len, out_len, d_model, feature_size
        self.token_proj = nn.Module()
        self.token_proj.weight = _p(d_model, feature_size, 1)
        self.token_proj.bias = _p(d_model)
        self.nlinear_encoder = LTSF_NLinearEncoder(seq_len, individual, d_model)
        self.pos_encoding = _p(1, d_model, seq_len)
        self.attn_block = SelfAttentionBlock(embed_dim=d_model, nhead=nhead, dropout_rate=dropout_rate)
        self.decoder = LTSF_NLinearDecoder(seq_len, out_len, individual, d_model, polygon_embed_dim, use_post_mlp,
                                           post_mlp_hidden_dim, d_model * out_len, dropout_rate, cross_dim,
                                           cross_nhead, output_feature_dim)
        self._ws = _Workspace()
        self._prep = None
        self.save_for_backward = False  # set by training.Trainer
        self.dropout_p, self.dctx = dropout_rate, None
        self._kv_stream = None
        # absorbed cross-attention (see forward): on for fp16 storage; training.Trainer(lora_trainable=True) turns it off
        # (that variant's backward wants dL/dk, dL/dv of the un-absorbed form)
        self.absorb_kv = True
        self._absorbed = False

    def _prepare(self):
        dec, C = self.decoder, self.d_model
        st = lambda mods, attr: torch.stack([getattr(m, attr).detach() for m in mods], dim=0).contiguous()
        H = dec.cross_dim
        ca = dec.cross_attn
        _bf16 = lambda t: _to16(t, self.storage)
        return SimpleNamespace(
            conv_w=self.token_proj.weight.detach()[:, :, 0].contiguous(),
            enc_w=st(self.nlinear_encoder.encoder_linears, "weight"), enc_b=st(self.nlinear_encoder.encoder_linears, "bias"),
            dec_w=st(dec.decoder_linears, "weight"), dec_b=st(dec.decoder_linears, "bias"),
            pos=self.pos_encoding.detach()[0, :, : self.seq_len].contiguous(),
            w_dp=_bf16(dec.dec_proj.weight), w_q=_bf16(ca.in_proj_weight[:H]), w_k=_bf16(ca.in_proj_weight[H:2 * H]),
            w_v=_bf16(ca.in_proj_weight[2 * H:]), b_q=ca.in_proj_bias.detach()[:H].contiguous(),
            b_k=ca.in_proj_bias.detach()[H:2 * H].contiguous(), b_v=ca.in_proj_bias.detach()[2 * H:].contiguous(),
            w_co=_bf16(ca.out_proj.weight), w_un=_bf16(dec.dec_unproj.weight),
            # absorbed cross-attention (forward): W_k per head, transposed -- [nh][H][dh], the W operand of q' = q_h W_k[h]
            wk_T=_bf16(ca.in_proj_weight[H:2 * H].detach().view(dec.cross_nhead, H // dec.cross_nhead, H).transpose(1, 2)))

    def front(self, x):
        """The part of forward() that does not depend on the LLM: token projection, per-channel N-Linear
        encoder, positional term and the self-attention block (train.py:837-840).  Returns the tokens
        [B*T, C]; MultiModalTrajectoryModel runs it on a side stream while the decoder stack computes."""
        B, F, T = x.shape
        dev, C, ws = x.device, self.d_model, self._ws
        P = self._prepared()
        tok = ws.get("lt.tok", (B * T, C), torch.float32, dev)
        xp_tok = ws.get("lt.xp", (B * T, C), torch.float32, dev) if self.save_for_backward else None
        if self._stage_ok(dev):  # one C call: tcavt_ltsf_forward phase 1 (csrc/tlayers.hip), the same launch sequence
            from . import capi
            sab, a = self.attn_block, capi.LtsfArgs()
            sw, E, M = sab._ws, C, B * T
            sab.drop_specs = sp = [_spec(sab.dctx, sab.dropout_p) for _ in range(4)]
            bufs = dict(sa_xn=sw.get("sab.xn", (M, E), torch.float32, dev), sa_qkv=sw.get("sab.qkv", (M, 3 * E), torch.float32, dev),
                        sa_att=sw.get("sab.att", (M, E), torch.float32, dev), sa_res1=sw.get("sab.res1", (M, E), torch.float32, dev),
                        sa_rn=sw.get("sab.rn", (M, E), torch.float32, dev), sa_f=sw.get("sab.f", (M, 4 * E), torch.float32, dev),
                        e=sw.get("sab.out", (M, E), torch.float32, dev), tok=tok, x=x)
            wts = dict(conv_w=P.conv_w, conv_b=self.token_proj.bias, enc_w=P.enc_w, enc_b=P.enc_b, pos=P.pos,
                       sa_n1_w=sab.norm1.weight, sa_n1_b=sab.norm1.bias, sa_in_w=sab.mha.in_proj_weight, sa_in_b=sab.mha.in_proj_bias,
                       sa_out_w=sab.mha.out_proj.weight, sa_out_b=sab.mha.out_proj.bias, sa_n2_w=sab.norm2.weight,
                       sa_n2_b=sab.norm2.bias, sa_f0_w=sab.ffn[0].weight, sa_f0_b=sab.ffn[0].bias, sa_f3_w=sab.ffn[3].weight,
                       sa_f3_b=sab.ffn[3].bias)
            keep = []
            for k_, t_ in list(bufs.items()) + list(wts.items()):
                setattr(a, k_, t_.data_ptr())
                keep.append(t_)
            if xp_tok is not None:
                a.xp_tok = xp_tok.data_ptr()
            a.B, a.C, a.T, a.To, a.F, a.nhead_sa = B, C, T, self.out_len, F, sab.nhead
            if sp[0] is not None:
                a.dropout_p, a.dropout_seed, a.first_site = sp[0][0], sp[0][1] & 0xFFFFFFFFFFFFFFFF, sp[0][2]
            ops.ltsf_forward(a, 1)
            del keep
            return bufs["e"]
        ops.ltsf_front(x, P.conv_w, self.token_proj.bias, P.enc_w, P.enc_b, P.pos, tok, B, C, T, xp_tok=xp_tok)
        return self.attn_block.forward_tokens(tok, B, T)

    def _head_stage(self, x, e, lane_polygon_emb, fh16, fhT, B, T, L, Lp, H, add_last):
        """Phase 2 of tcavt_ltsf_forward: the launches of forward() below, from C++, on the same named buffers (the backward
        finds them by name)."""
        from . import capi

        dev, C, To, ws = x.device, self.d_model, self.out_len, self._ws
        dec, P = self.decoder, self._prepared()
        nh = dec.cross_nhead
        M = B * To
        f32, st = torch.float32, self.storage
        g = lambda n, shape, dt=f32: ws.get("lt." + n, shape, dt, dev)
        a = capi.LtsfArgs()
        post = dec.post_mlp[0].weight.shape[0] if dec.use_post_mlp else 0
        self.drop_post = _spec(self.dctx, self.dropout_p) if dec.use_post_mlp else None
        self.drop_xattn = _spec(self.dctx, self.dropout_p)
        out = torch.empty((B, self.feature_size, To), dtype=f32, device=dev)
        bufs = dict(x=x, e=e, poly_emb=lane_polygon_emb.contiguous(), lane=g("lane", (B, C * To)), d0=g("dec0", (B, C * To)),
                    dec_t=g("dect", (M, C)), dec_tb=g("dectb", (M, C), st), proj=g("proj", (M, H), st), cross=g("cross", (M, H), st),
                    fused=g("fused", (M, C)), fn=g("fn", (M, C)), f1=g("f1", (M, C)), f2=g("f2", (M, C)), out=out)
        if post:
            bufs.update(hid=g("hid", (B, post)), d1=g("dec1", (B, C * To)))
        fl = dec.fusion_layer
        wts = dict(lane_w=dec.lane_fc.weight, lane_b=dec.lane_fc.bias, dec_w=P.dec_w, dec_b=P.dec_b, w_dp=P.w_dp, b_dp=dec.dec_proj.bias,
                   w_q=P.w_q, b_q=P.b_q, w_co=P.w_co, b_co=dec.cross_attn.out_proj.bias, w_un=P.w_un, b_un=dec.dec_unproj.bias,
                   fl_n_w=fl[0].weight, fl_n_b=fl[0].bias, fl1_w=fl[1].weight, fl1_b=fl[1].bias, fl3_w=fl[3].weight, fl3_b=fl[3].bias,
                   out_w=dec.out_proj.weight, out_b=dec.out_proj.bias)
        if post:
            wts.update(pm0_w=dec.post_mlp[0].weight, pm0_b=dec.post_mlp[0].bias, pm3_w=dec.post_mlp[3].weight,
                       pm3_b=dec.post_mlp[3].bias)
        xa = dict(q=g("q", (M, H), st), wk_t=P.wk_T, w_v=P.w_v, b_v=P.b_v, fh=fh16, fh_t=fhT, qp=g("qp", (nh, M, H), st),
                  scores=g("S", (B * nh * To, Lp)), probs=g("P", (B * nh * To, Lp), torch.float16), ctx=g("ctx", (nh, M, H), st),
                  att=g("att", (M, H), st))
        keep = []
        for k_, t_ in list(bufs.items()) + list(wts.items()):
            setattr(a, k_, t_.data_ptr())
            keep.append(t_)
        for k_, t_ in xa.items():
            setattr(a.xattn, k_, t_.data_ptr())
            keep.append(t_)
        a.xattn.B, a.xattn.To, a.xattn.L, a.xattn.Lp, a.xattn.H, a.xattn.nhead, a.xattn.dtype16 = B, To, L, Lp, H, nh, capi.F16
        if self.drop_xattn is not None:
            a.xattn.dropout_p, a.xattn.dropout_seed, a.xattn.dropout_site = (
                self.drop_xattn[0], self.drop_xattn[1] & 0xFFFFFFFFFFFFFFFF, self.drop_xattn[2])
        a.B, a.C, a.T, a.To, a.F, a.H, a.nhead_sa = B, C, T, To, self.feature_size, H, self.attn_block.nhead
        a.poly_dim, a.post_hidden, a.add_last = lane_polygon_emb.shape[1], post, int(bool(add_last))
        if self.drop_post is not None:  # sites: the self-attention block drew first_site .. + 3 in front(), the post-MLP + 4
            a.dropout_p, a.dropout_seed, a.first_site = self.drop_post[0], self.drop_post[1] & 0xFFFFFFFFFFFFFFFF, self.drop_post[2] - 4
        ops.ltsf_forward(a, 2)
        del keep
        return out

    def _stage_ok(self, dev):
        """The C++ stage (tcavt_ltsf_forward) covers the default form: fp16 storage, absorbed cross-attention."""
        return (dev.type == "cuda" or ops._ALLOW_CPU) and self.absorb_kv and self.storage == torch.float16 and \
            os.environ.get("TCAVT_PY_TLAYERS", "0") != "1"

    def forward(self, x, lane_polygon_emb, final_hidden, final_hidden_bf16=None, _fuse_last_residual=False, _front=None):
        """x (B,2,T) fp32; lane_polygon_emb (B,64); final_hidden (B,L,H) -> (B,2,To), as
        train.py:836-842.  ``_fuse_last_residual`` additionally adds x[:, :, -1:] in the head kernel
        (the caller's "simple residual", train.py:941-943) instead of a separate pass; ``_front`` is the
        result of front(x) when the caller already computed it."""
        B, F, T = x.shape
        dev, C, To, ws = x.device, self.d_model, self.out_len, self._ws
        dec, P = self.decoder, self._prepared()
        L, H = final_hidden.shape[1], final_hidden.shape[2]
        x = x.contiguous()
        nh = dec.cross_nhead
        dh = H // nh
        Lp = (L + XATTN_PAD - 1) // XATTN_PAD * XATTN_PAD
        if final_hidden_bf16 is None:
            final_hidden_bf16 = ws.get("lt.fhb", (B * L + XATTN_PAD, H), self.storage, dev, zero=True)
            ops.cast16(final_hidden.contiguous().view(B * L, H), out=final_hidden_bf16)
        elif final_hidden_bf16.shape[0] < (B - 1) * L + Lp:
            raise ValueError("final_hidden_bf16 needs XATTN_PAD zeroed tail rows")
        # The cross-attention K / V projections (two chip-filling GEMMs over the LLM's final hidden states) do not depend
        # on the decoder chain below (lane_fc -> N-Linear decoder -> post-MLP -> dec_proj -> q projection: one-workgroup
        # launches): they go to a side stream and join before the scores.
        main = torch.cuda.current_stream() if dev.type == "cuda" else None
        absorb = self.absorb_kv and self.storage == torch.float16
        self._absorbed = absorb  # (the backward follows the form the forward ran)
        if absorb:
            kv_ctx = None
        elif main is not None:
            if self._kv_stream is None:
                self._kv_stream = streams.side_stream(dev, 1)
            self._kv_stream.wait_stream(main)
            kv_ctx = torch.cuda.stream(self._kv_stream)
        else:
            kv_ctx = contextlib.nullcontext()
        if absorb:
            # fh^T per sample [H][B*Lp] (keys padded to Lp with zeros): the W operand of ctx = P . fh.  No K / V projection:
            # see the absorbed form below.
            fhT = ws.get("lt.fhT", (H, B * Lp), self.storage, dev)
        else:
            with kv_ctx:
                # K projection [B*L, H] bf16 (tail rows only ever feed score columns >= L, which softmax ignores)
                kx = ws.get("lt.k", (B * L + XATTN_PAD, H), self.storage, dev, zero=True)
                ops.gemm_bf16(final_hidden_bf16[: B * L], P.w_k, out=kx, bias=P.b_k)
                # V projection emitted TRANSPOSED and in fp16: vT[d][b*Lp + l] = W_v[d] . x[b*L + l] + b_v[d]
                # (roles of weights and activations swapped, batched over samples), so that P.V is again
                # a K-contiguous A.W^T product
                vT = ws.get("lt.vT", (H, B * Lp), torch.float16, dev)
                ops.gemm_batched(P.w_v, final_hidden_bf16, vT, M=H, N=Lp, K=H, lda=H, ldw=H, ldc=B * Lp, batch=B, inner=1,
                                 sA=(0, 0), sW=(L * H, 0), sC=(Lp, 0), bias_row=P.b_v)
        e = _front if _front is not None else self.front(x)
        if absorb and self._stage_ok(dev):
            return self._head_stage(x, e, lane_polygon_emb, final_hidden_bf16, fhT, B, T, L, Lp, H, _fuse_last_residual)
        lane = ws.get("lt.lane", (B, C * To), torch.float32, dev)
        ops.gemm_f32(lane_polygon_emb.contiguous(), dec.lane_fc.weight, out=lane, bias=dec.lane_fc.bias)
        d0 = ws.get("lt.dec0", (B, C * To), torch.float32, dev)
        ops.ltsf_decode(e, P.dec_w, P.dec_b, lane, d0, B, C, T, To)
        if dec.use_post_mlp:
            hid = ws.get("lt.hid", (B, dec.post_mlp[0].weight.shape[0]), torch.float32, dev)
            self.drop_post = _spec(self.dctx, self.dropout_p)
            ops.gemm_f32(d0, dec.post_mlp[0].weight, out=hid, bias=dec.post_mlp[0].bias, relu=True,
                         dropout=self.drop_post)
            d1 = ws.get("lt.dec1", (B, C * To), torch.float32, dev)
            ops.gemm_f32(hid, dec.post_mlp[3].weight, out=d1, bias=dec.post_mlp[3].bias)
        else:
            d1 = d0
        dec_t = ws.get("lt.dect", (B * To, C), torch.float32, dev)
        dec_tb = ws.get("lt.dectb", (B * To, C), self.storage, dev)
        ops.transpose_ct(d1, dec_t, dec_tb, B, C, To)
        # cross attention over the LLM's final hidden states: K = V = final_hidden, no padding mask
        proj = ws.get("lt.proj", (B * To, H), self.storage, dev)
        ops.gemm_bf16(dec_tb, P.w_dp, out=proj, bias=dec.dec_proj.bias)
        q = ws.get("lt.q", (B * To, H), self.storage, dev)
        ops.gemm_bf16(proj, P.w_q, out=q, bias=P.b_q)
        S = ws.get("lt.S", (B * nh * To, Lp), torch.float32, dev)
        Pm = ws.get("lt.P", (B * nh * To, Lp), torch.float16, dev)
        att = ws.get("lt.att", (B * To, H), self.storage, dev)
        M = B * To
        if absorb:
            # Absorbed form.  With To (30) queries per sample against L (256) keys the K / V projections of the final hidden
            # states (2 x 2 M H^2 = 137 GFLOP, the head's two chip-filling GEMMs -- and three more in the backward) move to
            # the query / output side, where they cost 2 x 2 (B To) H^2 = 16 GFLOP:
            #     scores_h = q_h (fh W_k[h]^T + b_k)^T  =  (q_h W_k[h]) fh^T  + const per query   (softmax-invariant: b_k drops out)
            #     att_h    = P_h (fh W_v[h]^T + b_v)    =  (P_h fh) W_v[h]^T + b_v               (rows of P sum to 1)
            # Same arithmetic as nn.MultiheadAttention (train.py:795-798) in exact arithmetic; the rounding points move from
            # k, v to q' = q_h W_k[h] and ctx_h = P_h fh (oracle/forward.py restates both forms).
            qp = ws.get("lt.qp", (nh, M, H), self.storage, dev)
            ctx = ws.get("lt.ctx", (nh, M, H), self.storage, dev)
            self.drop_xattn = _spec(self.dctx, self.dropout_p)
            if os.environ.get("TCAVT_PY_TLAYERS", "0") == "1":  # the per-launch Python composition (A/B, bit-identical)
                ops.transpose16(final_hidden_bf16, fhT, L, H, Lp, ld_in=H, ld_out=B * Lp, batch=B, s_in=L * H, s_out=Lp)
                for h in range(nh):
                    ops.gemm_bf16(q[:, h * dh:(h + 1) * dh], P.wk_T[h], out=qp[h])
                ops.gemm_batched(qp, final_hidden_bf16, S, M=To, N=Lp, K=H, lda=H, ldw=H, ldc=Lp, batch=B * nh, inner=nh,
                                 sA=(To * H, M * H), sW=(L * H, 0), sC=(nh * To * Lp, To * Lp), acc_scale=1.0 / math.sqrt(dh),
                                 tile=64)
                ops.softmax_rows(S, Pm, B * nh * To, L, Lp, Lp, Lp, dropout=self.drop_xattn)
                ops.gemm_batched(Pm, fhT, ctx, M=To, N=H, K=Lp, lda=Lp, ldw=B * Lp, ldc=H, batch=B * nh, inner=nh,
                                 sA=(nh * To * Lp, To * Lp), sW=(Lp, 0), sC=(To * H, M * H), tile=64)
                for h in range(nh):
                    ops.gemm_bf16(ctx[h], P.w_v[h * dh:(h + 1) * dh], out=att[:, h * dh:(h + 1) * dh],
                                  bias=P.b_v[h * dh:(h + 1) * dh])
            else:  # one C call: tcavt_cross_attn_forward (csrc/tlayers.hip), the same launch sequence
                from . import capi
                ca_args = capi.CrossAttnArgs()
                for k_, t_ in (("q", q), ("wk_t", P.wk_T), ("w_v", P.w_v), ("b_v", P.b_v), ("fh", final_hidden_bf16), ("fh_t", fhT),
                               ("qp", qp), ("scores", S), ("probs", Pm), ("ctx", ctx), ("att", att)):
                    setattr(ca_args, k_, t_.data_ptr())
                ca_args.B, ca_args.To, ca_args.L, ca_args.Lp, ca_args.H, ca_args.nhead = B, To, L, Lp, H, nh
                ca_args.dtype16 = capi.F16
                if self.drop_xattn is not None:
                    ca_args.dropout_p, ca_args.dropout_seed, ca_args.dropout_site = (
                        self.drop_xattn[0], self.drop_xattn[1] & 0xFFFFFFFFFFFFFFFF, self.drop_xattn[2])
                ops.cross_attn_forward(ca_args)
        else:
            if main is not None:
                main.wait_stream(self._kv_stream)
            # scores[b,h] = q_bh . k_bh^T / sqrt(dh)  (fp32), softmax -> fp16 probabilities (zero beyond L)
            ops.gemm_batched(q, kx, S, M=To, N=Lp, K=dh, lda=H, ldw=H, ldc=Lp, batch=B * nh, inner=nh,
                             sA=(To * H, dh), sW=(L * H, dh), sC=(nh * To * Lp, To * Lp), acc_scale=1.0 / math.sqrt(dh))
            self.drop_xattn = _spec(self.dctx, self.dropout_p)
            ops.softmax_rows(S, Pm, B * nh * To, L, Lp, Lp, Lp, dropout=self.drop_xattn)
            ops.gemm_batched(Pm, vT, att, M=To, N=dh, K=Lp, lda=Lp, ldw=B * Lp, ldc=H, batch=B * nh, inner=nh,
                             sA=(nh * To * Lp, To * Lp), sW=(Lp, dh * B * Lp), sC=(To * H, dh))
        cross = ws.get("lt.cross", (B * To, H), self.storage, dev)
        ops.gemm_bf16(att, P.w_co, out=cross, bias=dec.cross_attn.out_proj.bias)
        fused = ws.get("lt.fused", (B * To, C), torch.float32, dev)
        ops.gemm_bf16(cross, P.w_un, out=fused, bias=dec.dec_unproj.bias, residual=dec_t)
        fl = dec.fusion_layer
        fn = ws.get("lt.fn", (B * To, C), torch.float32, dev)
        ops.layernorm(fused, fl[0].weight, fl[0].bias, 1e-5, out_f32=fn)
        f1 = ws.get("lt.f1", (B * To, C), torch.float32, dev)
        ops.gemm_f32(fn, fl[1].weight, out=f1, bias=fl[1].bias, relu=True)
        f2 = ws.get("lt.f2", (B * To, C), torch.float32, dev)
        ops.gemm_f32(f1, fl[3].weight, out=f2, bias=fl[3].bias)
        out = torch.empty((B, self.feature_size, To), dtype=torch.float32, device=dev)
        ops.out_head(f2, dec.out_proj.weight, dec.out_proj.bias, x, out, B, To, C, self.feature_size, T,
                     add_last=_fuse_last_residual)
        return out


# --------------------------------------------------------------------------------------
# MultiModalTrajectoryModel (train.py:847-964)
# --------------------------------------------------------------------------------------
class MultiModalTrajectoryModel(nn.Module):
    HEAD_MAX_L = 544  # decoder rows (image tokens + text) the trajectory head's cross-attention buffers are sized for

    def __init__(self, seq_len, out_len, individual, feature_size=2, d_model=64, lane_polygon_d_model=64,
                 lane_polygon_nhead=4, lane_polygon_layers=2, max_polygon_points=64, use_post_mlp=True,
                 post_mlp_hidden_dim=64, base_model_name="meta-llama/Llama-3.2-1B", use_lora=True, lora_r=8,
                 lora_alpha=32, lora_dropout=0.1, vision_dim=512, q_hidden_size=768, q_nhead=8, q_enc_layers=4,
                 q_dec_layers=4, q_num_query_tokens=16, ltsf_nhead=1, ltsf_dropout=0.1,
                 llama_shape: LlamaShape = None, dim_feedforward=2048):
        super().__init__()
        self.lane_polygon_encoder = LanePolygonEncoder(lane_polygon_d_model, lane_polygon_nhead,
                                                       lane_polygon_layers, max_polygon_points, dim_feedforward)
        self.mllm = LlamaMultiModal(base_model_name, use_lora, lora_r, lora_alpha, lora_dropout, vision_dim,
                                    q_hidden_size, q_nhead, q_enc_layers, q_dec_layers, q_num_query_tokens,
                                    llama_shape, dim_feedforward)
        self.llama_hidden_size = self.mllm.llama_hidden_size
        self.ltsf = TransformerLTSF(seq_len, out_len, individual, feature_size, d_model,
                                    polygon_embed_dim=lane_polygon_d_model, use_post_mlp=use_post_mlp,
                                    post_mlp_hidden_dim=post_mlp_hidden_dim, post_mlp_output_dim=d_model * out_len,
                                    nhead=ltsf_nhead, dropout_rate=ltsf_dropout, cross_dim=self.llama_hidden_size,
                                    cross_nhead=2, output_feature_dim=feature_size)
        self.feature_size, self.out_len, self.seq_len = feature_size, out_len, seq_len
        self._llm_cache = None  # (final_hidden, final_hidden_bf16) of an earlier pass on the same batch (evaluate_model)
        self.overlap_streams = True  # side stream for the LLM-independent small-kernel chains (see forward)
        self._side = None
        # Pipelined decoder (train.py's frozen MLLM: nothing the decoder reads is written by the step's backward or
        # optimizer): the MLLM pass runs on a stream of its own, so the decoder of step i + 1 starts as soon as the decoder
        # of step i has finished and runs over step i's head / loss / backward / AdamW -- ~200 small dependent launches
        # that leave the chip idle (2.2 of 17 ms).  Results are identical; every step still runs one pass of everything.
        # Off by default; training.Trainer turns it on for the frozen-decoder variant.  See forward / inputs_ready.
        self.pipeline_decoder = False
        self.inputs_ready = None  # see forward
        self.pipe_trace = None
        self._dec_stream, self._dec_slot, self._fwd_start_ev = None, 0, None
        # Train-mode dropout (the MC-dropout K-candidate protocol, test.py:1301-1342): active when the module
        # is in .train() mode; every forward uses seed dropout_seed + number of forwards so far.
        self.dropout_seed, self._fwd_count = 0x5EED, 0
        self._auto_range, self.range_contract = None, None  # set_storage("auto")
        # loss.backward() (autograd.py): forwards so far, in any mode -- each one overwrites the tapes a pending backward reads;
        # a training.Trainer drives its model itself and keeps it off the bridge
        self._n_forward, self.driven_by_trainer, self._bridge = 0, False, None

    @classmethod
    def from_config(cls, cfg: ModelConfig):
        return cls(seq_len=cfg.seq_len, out_len=cfg.out_len, individual=cfg.individual, feature_size=cfg.feature_size,
                   d_model=cfg.d_model, lane_polygon_d_model=cfg.lane_polygon_d_model,
                   lane_polygon_nhead=cfg.lane_polygon_nhead, lane_polygon_layers=cfg.lane_polygon_layers,
                   max_polygon_points=cfg.max_polygon_points, use_post_mlp=cfg.use_post_mlp,
                   post_mlp_hidden_dim=cfg.post_mlp_hidden_dim, use_lora=cfg.use_lora, lora_r=cfg.lora_r,
                   lora_alpha=cfg.lora_alpha, lora_dropout=cfg.lora_dropout, vision_dim=cfg.vision_dim,
                   q_hidden_size=cfg.q_hidden_size, q_nhead=cfg.q_nhead, q_enc_layers=cfg.q_enc_layers,
                   q_dec_layers=cfg.q_dec_layers, q_num_query_tokens=cfg.q_num_query_tokens,
                   ltsf_nhead=cfg.ltsf_nhead, ltsf_dropout=cfg.ltsf_dropout, llama_shape=cfg.llama,
                   dim_feedforward=cfg.transformer_ff)

    def load_weights(self, weights, device=None):
        """weights: {state-dict key: ndarray/tensor} (tcavt_amd.weights.make_weights or a checkpoint)."""
        sd = {k: (torch.from_numpy(v) if not torch.is_tensor(v) else v) for k, v in weights.items()}
        missing, unexpected = self.load_state_dict(sd, strict=False)
        missing = [k for k in missing if not k.endswith("lm_head.weight")]
        if missing or unexpected:
            raise KeyError(f"state-dict mismatch: missing={missing[:5]} unexpected={unexpected[:5]}")
        if device is not None:
            self.to(device)
        self.invalidate_prepared()
        return self

    def invalidate_prepared(self):
        for m in self.modules():
            if isinstance(m, _Prepared):
                m._invalidate()

    # stream contracts set_storage("auto") walks through, in order, until a pass raises no range flag: the plain 16-bit stream,
    # the same stream kept at 2^-k (overflow limit 65504 * 2^k; fp16 is a floating-point format, so the scale costs nothing
    # until values fall below 6.1e-5 * 2^k and go subnormal -- hence the smallest k that passes), and last an fp32 stream
    # whose 16-bit copy is kept at the smallest scale (10 instead of 4 bytes per element through the residual epilogues).
    AUTO_LADDER = ((1.0, False), (2.0 ** -2, False), (2.0 ** -4, False), (2.0 ** -6, False), (2.0 ** -8, False),
                   (2.0 ** -10, False), (2.0 ** -10, True))

    def set_storage(self, dtype, stream_scale=None, wide_stream=None):
        """16-bit storage type of every GEMM operand of the model (weights copies and activations): torch.float16 (the
        default, see _Prepared.storage) or torch.bfloat16.  Packed copies are rebuilt on the next forward.

        "auto": fp16, with the decoder's residual-stream contract chosen on the first forward: the pass runs on the plain
        16-bit stream; if its range flag comes back set (tcavt_llama_stack_args.nonfinite_flag: some 16-bit value left
        +-65504) the same batch is re-run down AUTO_LADDER until a pass is clean, and the model keeps that contract
        (self.range_contract says which; one host sync per trial, on the first forward only).  Real Llama checkpoints carry
        outlier channels orders of magnitude above the bulk of the stream; the synthetic weights here stay at ~10.
        stream_scale / wide_stream set a contract by hand (LlamaWithCrossAttnPEFT.stream_scale / .wide_stream)."""
        auto = isinstance(dtype, str) and dtype == "auto"
        if auto:
            dtype = torch.float16
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError('storage must be torch.float16, torch.bfloat16 or "auto"')
        for m in self.modules():
            if isinstance(m, _Prepared):
                m.storage = dtype
                m._invalidate()
        lw = self.mllm.llama_wrapper
        lw.set_stream_contract(1.0 if stream_scale is None else float(stream_scale), bool(wide_stream) if wide_stream is not None else False)
        if lw.stream_scale <= 0.0 or lw.stream_scale > 1.0 or math.frexp(lw.stream_scale)[0] != 0.5:
            raise ValueError("stream_scale must be a power of two in (0, 1]")
        self._auto_range = "pending" if auto else None
        self.range_contract = None
        return self

    def set_mlp_precision(self, precision="fp16"):
        """Precision of the frozen decoder's MLP GEMMs (gate|up and down) in every decoder pass that keeps no tape: forward,
        evaluate_model at any K, lm_evaluate and the prefill of generate_batch.  "fp16" (the default): the 16-bit kernels.  "mx8"
        (opt-in): activations and weights as MXFP8-E4M3 blocks of 32 (quant.quantize_mx) on the block-scaled MFMA
        (LlamaWithCrossAttnPEFT.mlp_weights).  The decode step and the KV cache are unaffected.  There is no fallback: a pass that
        cannot run on MX8 (a tape, hidden or inter not a multiple of 128, 32 rows or fewer) raises."""
        if precision not in ("fp16", "mx8"):
            raise ValueError(f"set_mlp_precision: precision must be 'fp16' or 'mx8', got {precision!r}")
        lw = self.mllm.llama_wrapper
        if precision == "mx8" and (lw.shape.hidden % 128 or lw.shape.inter % 128):
            raise ValueError(f"set_mlp_precision: 'mx8' needs hidden and inter to be multiples of 128, got {lw.shape.hidden} / {lw.shape.inter}")
        lw.mlp_precision = precision
        return self

    def _calibrate_range(self, vision_embs, context_str, input_ids, attention_mask, labels):
        """First forward under set_storage("auto"): trial passes of the MLLM down AUTO_LADDER (see set_storage)."""
        lw = self.mllm.llama_wrapper
        trials = []
        for scale, wide in self.AUTO_LADDER:
            lw.set_stream_contract(scale, wide)
            with torch.no_grad():
                self.mllm(vision_embs, context_str, input_ids=input_ids, attention_mask=attention_mask, labels=labels, return_bf16=True)
            flags = self.mllm._last_flags
            tag = int(flags[2].item())  # (host sync: calibration only)
            flags[2:3].zero_()
            trials.append((scale, wide, tag))
            if tag == 0:
                break
        self._auto_range = None
        self.range_contract = SimpleNamespace(stream_scale=lw.stream_scale, wide_stream=lw.wide_stream, trials=trials,
                                              clean=trials[-1][2] == 0)
        if not self.range_contract.clean:
            # nothing on the ladder helps: the overflow is not in the residual stream (act / q|k|v / attention output), or the
            # inputs are not finite -- back to the plain contract; check_flags() reports it as before
            lw.set_stream_contract(1.0, False)

    @property
    def storage(self):
        return self.mllm.llama_wrapper.storage

    def mllm_is_deterministic(self):
        """True when a forward of the MLLM cannot depend on the dropout seed: eval mode, or no dropout site inside it
        (Q-Former dropout 0 and no LoRA dropout).  Then the K candidates of test.py:1327-1339 share one MLLM pass."""
        lw = self.mllm.llama_wrapper
        return (not self.training) or (self.mllm.qformer.dropout_p == 0.0 and (not lw.use_lora or lw.lora_dropout == 0.0))

    def prefetch(self, vision_embs, ready=None):
        """Start the frozen Q-Former of the NEXT batch underneath the pass in flight (LlamaMultiModal.prefetch)."""
        dctx = DropoutCtx(self.dropout_seed + self._fwd_count).sub(1) if self.training else None  # the next forward's masks
        self.mllm.prefetch(vision_embs, ready=ready, dctx=dctx)

    def forward(self, x, vision_embs, context_str, lane_polygon_batch, lane_polygon_len, y=None, norm_stat=None,
                input_ids=None, attention_mask=None, labels=None):
        """(Signature of the reference's forward, scripts/train.py:914.)  With pipeline_decoder, `self.inputs_ready` says
        when the MLLM inputs of THIS call (vision_embs, input_ids, attention_mask) are ready on the device: a
        torch.cuda.Event (e.g. of the copy stream that uploaded the batch), True (already resident, nobody is writing them),
        or None: ready once the work queued on the current stream so far is done (always correct; the decoder then cannot
        start before the previous step's optimizer has finished).  It is consumed by the call (reset to None).

        In grad mode with a supported trainable set (autograd.trainable_set: train.py's frozen MLLM, or that plus the LoRA
        adapters) the outputs carry an autograd graph and loss.backward() runs the hand-written backward (autograd.py);
        in every other state they are plain tensors."""
        if torch.is_grad_enabled():
            from . import autograd as _ag

            kind = _ag.trainable_set(self)
            if kind is not None:
                return _ag.bridge_forward(self, kind, x, vision_embs, context_str, lane_polygon_batch, lane_polygon_len, y,
                                          norm_stat, input_ids, attention_mask, labels)
        return self._forward(x, vision_embs, context_str, lane_polygon_batch, lane_polygon_len, y=y, norm_stat=norm_stat,
                             input_ids=input_ids, attention_mask=attention_mask, labels=labels)

    def _check_head_limit(self, input_ids):
        """The trajectory path keeps L <= 544 (train.py truncates its text to 512; the head's cross-attention is sized for
        that).  The decoder itself serves L <= 2048, so the refusal is made here, before anything is launched."""
        if input_ids is None:  # (an MLLM pass cached by evaluate_model(reuse_prefix=True): checked when it was made)
            return
        L = self.mllm.qformer.num_query_tokens + input_ids.shape[1]
        if L > self.HEAD_MAX_L:
            raise ValueError(f"MultiModalTrajectoryModel: L = {L} decoder rows exceed the trajectory head's limit of "
                             f"{self.HEAD_MAX_L}; longer text is served by the stage-1 entry points of the MLLM alone "
                             "(mllm.lm_forward, mllm.lm_evaluate, mllm.generate_batch, training.MllmTrainer, "
                             "evaluate.evaluate_mllm), up to 2048 rows")

    def _forward(self, x, vision_embs, context_str, lane_polygon_batch, lane_polygon_len, y=None, norm_stat=None,
                 input_ids=None, attention_mask=None, labels=None):
        if (input_ids is None or attention_mask is None) and self._llm_cache is None:
            # tokenizer branch: tokenised here (host work) so that the length is known before anything is launched
            input_ids, attention_mask = self.mllm.tokenize_context(context_str, vision_embs.device)
            labels = None
        self._check_head_limit(input_ids)
        self._n_forward += 1
        if self._bridge is not None and not self.driven_by_trainer:
            self._bridge.refresh()  # (a model that has trained through loss.backward(): rebuild stale packed weights first)
        inputs_ready, self.inputs_ready = self.inputs_ready, None
        B = x.size(0)
        dev = x.device
        x = x.contiguous()
        dctx = None
        if self.training:
            dctx = DropoutCtx(self.dropout_seed + self._fwd_count)
            self._fwd_count += 1
        sub = (lambda b: dctx.sub(b)) if dctx is not None else (lambda b: None)
        self.lane_polygon_encoder.dctx, self.mllm.qformer.dctx, self.mllm.llama_wrapper.dctx = sub(0), sub(1), sub(2)
        self.ltsf.dctx = self.ltsf.attn_block.dctx = sub(3)
        if getattr(self, "_auto_range", None) == "pending" and dev.type == "cuda" and self._llm_cache is None:
            self._calibrate_range(vision_embs, context_str, input_ids, attention_mask, labels)
        # The lane-polygon encoder and the LLM-independent half of the LTSF (token projection, N-Linear
        # encoder, self-attention block) are chains of small launches that leave most CUs idle; they run
        # on a side stream, concurrently with the Q-Former / decoder stack, and join before the LTSF head.
        main = torch.cuda.current_stream() if dev.type == "cuda" else None
        if main is not None and self.overlap_streams:
            if self._side is None:
                self._side = streams.side_stream(dev, 0)
            self._side.wait_stream(main)
            with torch.cuda.stream(self._side):
                poly_emb = self.lane_polygon_encoder(lane_polygon_batch, lane_polygon_len)
                front = self.ltsf.front(x)
                poly_emb.record_stream(main)
        else:
            poly_emb = self.lane_polygon_encoder(lane_polygon_batch, lane_polygon_len)
            front = self.ltsf.front(x)
        if self._llm_cache is not None:  # evaluate_model(reuse_prefix=True): the MLLM pass of an earlier candidate
            final_hidden, final_b = self._llm_cache
        elif main is not None and self.pipeline_decoder and not self.mllm.llama_wrapper.save_for_backward:
            if self._dec_stream is None:
                self._dec_stream = torch.cuda.Stream(device=dev, priority=int(os.environ.get("TCAVT_DEC_PRIO", "0")))  # (A/B knob)
            D = self._dec_stream
            if inputs_ready is None:
                D.wait_stream(main)
            elif inputs_ready is not True:
                D.wait_event(inputs_ready)
            # output slot s was last read by the head / backward of the pass before the previous one: all of that was on the
            # caller's queue when the previous forward began
            if self._fwd_start_ev is not None:
                D.wait_event(self._fwd_start_ev)
            self._fwd_start_ev = torch.cuda.Event()
            self._fwd_start_ev.record(main)
            trace = self.pipe_trace  # (tools only) a list that receives (start, stop) timing events of every MLLM pass
            with torch.cuda.stream(D):
                if trace is not None:
                    t0 = torch.cuda.Event(enable_timing=True)
                    t0.record(D)
                final_hidden, _, final_b = self.mllm(vision_embs, context_str, input_ids=input_ids, attention_mask=attention_mask,
                                                     labels=labels, return_bf16=True, out_slot=self._dec_slot)
                done = torch.cuda.Event(enable_timing=trace is not None)
                done.record(D)
                if trace is not None:
                    trace.append((t0, done))
            self._dec_slot ^= 1
            final_hidden.record_stream(main)
            main.wait_event(done)
        else:
            final_hidden, _, final_b = self.mllm(vision_embs, context_str, input_ids=input_ids,
                                                 attention_mask=attention_mask, labels=labels, return_bf16=True)
        if main is not None and self.overlap_streams:
            main.wait_stream(self._side)
        decoded = self.ltsf(x, poly_emb, final_hidden, final_hidden_bf16=final_b, _fuse_last_residual=True,
                            _front=front)
        self.last = SimpleNamespace(poly_emb=poly_emb, final_hidden=final_hidden, final_hidden_bf16=final_b)
        if y is not None and norm_stat is not None:
            ns = norm_stat if torch.is_tensor(norm_stat) else torch.tensor([list(n) for n in norm_stat], dtype=torch.float32)
            ns = ns.to(device=dev, dtype=torch.float32).contiguous()
            sums = torch.zeros(5, dtype=torch.float32, device=dev)
            ops.traj_metrics(decoded, y.contiguous(), ns, sums, None, None, B, 1, self.out_len)
            loss = (sums[0] + sums[1]) / float(B * self.out_len)  # MSE(x) + MSE(y), train.py:959-961
            return loss, decoded
        return decoded
