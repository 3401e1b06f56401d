"""Host side of csrc/tlayers.hip: the generic post-LN transformer layers (nn.TransformerEncoder/DecoderLayer defaults)
over the C ABI, and the two modules built from them -- LanePolygonEncoder (train.py:352-383) and BlipQFormer
(train.py:388-414)."""
import math
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import capi, ops
from .parts import _LayerStack, _Linear, _p, _Prepared, _spec, _to16, _Workspace


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
        self.stage = None  # (TStackArgs, keep-list) of the last run_stack of a recording run

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
        keep = [arr]
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
            capi.bind(arr[i], keep, **bufs, **w)
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
        capi.bind(args, keep, x=x, xb=xb, mem=mem, memb=memb, key_len=key_len)
        args.B, args.L, args.Lk, args.E, args.FF, args.nhead = B, L, Lk, E, layers[0].w1.shape[0], self.nhead
        args.dtype16 = (capi.F16 if self.dt16 == torch.float16 else capi.BF16) if self.bf16 else 0
        capi.bind_dropout(args, first_site, site="first_site")
        ops.tlayer_stack_forward(args)
        # a recording run keeps the filled struct and what its pointers name: the stage backward is handed exactly this
        self.stage = (args, keep) if self.record is not None else None
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
            self.saved = SimpleNamespace(layers=run.record, lens=lens, polygon=polygon_batch, out=x, B=B, P=P, stage=run.stage)
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
