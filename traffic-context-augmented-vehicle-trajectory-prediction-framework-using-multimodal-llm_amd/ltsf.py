"""LTSF blocks (train.py:659-842): the self-attention block, the per-channel N-Linear holders and TransformerLTSF, the
trajectory head with its cross-attention over the LLM's final hidden states (C stages of csrc/tlayers.hip, or the
per-launch Python compositions).

Each part names its workspace buffers in one place -- SelfAttentionBlock._bufs, TransformerLTSF._head_bufs -- which the C
stage and the composition both fill.  A forward under ``save_for_backward`` hands them, with its inputs, shapes, dropout
sites and stage structs, to the backward as one record, ``TransformerLTSF.saved`` (as LanePolygonEncoder.saved and
BlipQFormer.saved in tlayers.py): backward.Backward reads that record and never asks a workspace for a forward buffer."""
import contextlib
import math
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import capi, ops, streams
from .layout import XATTN_PAD
from .parts import _Linear, _MHA, _Norm, _p, _Prepared, _spec, _to16, _Workspace

# TransformerLTSF._head_bufs: the head buffers whose name in the backward's record is not their workspace name, and the order
# in which the C stage's head asks for its buffers (the composition asks in another; a workspace lists its buffers in
# allocation order, and tests/golden/call_trace.json pins that list)
_RECORD_NAME = dict(dec0="d0", dec1="d1", dect="dec_t", dectb="dec_tb")
_STAGE_ORDER = ("lane", "dec0", "dect", "dectb", "proj", "cross", "fused", "fn", "f1", "f2", "hid", "dec1", "q", "qp", "S", "P", "ctx",
                "att")


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

    def _bufs(self, M, dev):
        """The block's workspace tensors for M tokens, by the names its backward uses (SimpleNamespace, in allocation order)."""
        E, g = self.embed_dim, lambda n, w: self._ws.get("sab." + n, (M, w), torch.float32, dev)
        return SimpleNamespace(xn=g("xn", E), qkv=g("qkv", 3 * E), att=g("att", E), res1=g("res1", E), rn=g("rn", E),
                               f=g("f", 4 * E), out=g("out", E))

    def _drop_specs(self):
        """The four dropout sites of the block, in call order [attention weights, after out_proj, after ReLU, after ffn.3];
        kept for the backward (same masks on the gradients)."""
        return [_spec(self.dctx, self.dropout_p) for _ in range(4)]

    def forward_tokens(self, tok, B, T):
        """tok fp32 [B*T, E] (batch-first tokens) -> (b, sp): b the block's buffers (b.out [B*T, E] is the result), sp its
        dropout sites.  Residuals start from the NORMED tensors exactly as train.py:677-684."""
        E = self.embed_dim
        b, sp = self._bufs(B * T, tok.device), self._drop_specs()
        ops.layernorm(tok, self.norm1.weight, self.norm1.bias, 1e-5, out_f32=b.xn)
        ops.gemm_f32(b.xn, self.mha.in_proj_weight, out=b.qkv, bias=self.mha.in_proj_bias)
        dh = E // self.nhead
        ops.mha(b.qkv[:, :E], b.qkv[:, E:2 * E], b.qkv[:, 2 * E:], b.att, B, T, T, self.nhead, dh, 1.0 / math.sqrt(dh),
                ldq=3 * E, ldk=3 * E, ldv=3 * E, ldo=E, dropout=sp[0])
        ops.gemm_f32(b.att, self.mha.out_proj.weight, out=b.res1, bias=self.mha.out_proj.bias, residual=b.xn, dropout=sp[1])
        ops.layernorm(b.res1, self.norm2.weight, self.norm2.bias, 1e-5, out_f32=b.rn)
        ops.gemm_f32(b.rn, self.ffn[0].weight, out=b.f, bias=self.ffn[0].bias, relu=True, dropout=sp[2])
        ops.gemm_f32(b.f, self.ffn[3].weight, out=b.out, bias=self.ffn[3].bias, residual=b.rn, dropout=sp[3])
        return b, sp

    def forward(self, x):
        """x (B, E, T) -> (B, E, T), the reference's layout (train.py:674-686)."""
        B, E, T = x.shape
        tok = x.permute(0, 2, 1).contiguous().view(B * T, E)
        return self.forward_tokens(tok, B, T)[0].out.view(B, T, E).permute(0, 2, 1).contiguous()


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
        # absorbed cross-attention (see _head): on for fp16 storage; training.Trainer(lora_trainable=True) turns it off
        # (that variant's backward wants dL/dk, dL/dv of the un-absorbed form)
        self.absorb_kv = True
        # What the backward reads of the last forward (save_for_backward), references only: shapes B, T, L, Lp; inputs x,
        # poly_emb, final_hidden_bf16; the form that ran -- absorbed, and stage / xattn_stage, the C stages' filled argument
        # structs with what their pointers name, (struct, keep-list), or None (LtsfArgs: front() fills phase 1, _head_stage
        # phase 2; CrossAttnArgs: the plain tcavt_cross_attn_forward branch, or the head stage's embedded one; the stage
        # backwards are handed these); the dropout triples sab_drop[4], drop_post, drop_xattn; the retained activations
        # (tok, xp, e, _head_bufs' names, k and vT or fhT) and sab, the self-attention block's own buffers.  front() clears
        # it and leaves its part in _front; forward() completes and publishes it.
        self.saved = self._front = None

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
        self.saved = self._front = None
        sab, stage = self.attn_block, None
        if self._stage_ok(dev):  # one C call: tcavt_ltsf_forward phase 1 (csrc/tlayers.hip), the same launch sequence
            a, sb, sp = capi.LtsfArgs(), sab._bufs(B * T, dev), sab._drop_specs()
            bufs = dict(sa_xn=sb.xn, sa_qkv=sb.qkv, sa_att=sb.att, sa_res1=sb.res1, sa_rn=sb.rn, sa_f=sb.f, e=sb.out, tok=tok, x=x)
            wts = dict(conv_w=P.conv_w, conv_b=self.token_proj.bias, enc_w=P.enc_w, enc_b=P.enc_b, pos=P.pos,
                       sa_n1_w=sab.norm1.weight, sa_n1_b=sab.norm1.bias, sa_in_w=sab.mha.in_proj_weight, sa_in_b=sab.mha.in_proj_bias,
                       sa_out_w=sab.mha.out_proj.weight, sa_out_b=sab.mha.out_proj.bias, sa_n2_w=sab.norm2.weight,
                       sa_n2_b=sab.norm2.bias, sa_f0_w=sab.ffn[0].weight, sa_f0_b=sab.ffn[0].bias, sa_f3_w=sab.ffn[3].weight,
                       sa_f3_b=sab.ffn[3].bias)
            keep = []
            capi.bind(a, keep, xp_tok=xp_tok, **bufs, **wts)
            a.B, a.C, a.T, a.To, a.F, a.nhead_sa = B, C, T, self.out_len, F, sab.nhead
            capi.bind_dropout(a, sp[0], site="first_site")
            ops.ltsf_forward(a, 1)
            stage = (a, keep)
        else:
            ops.ltsf_front(x, P.conv_w, self.token_proj.bias, P.enc_w, P.enc_b, P.pos, tok, B, C, T, xp_tok=xp_tok)
            sb, sp = sab.forward_tokens(tok, B, T)
        self._front = SimpleNamespace(B=B, T=T, tok=tok, xp=xp_tok, e=sb.out, sab=sb, sab_drop=sp, stage=stage)
        return sb.out

    def _head_bufs(self, B, Lp, H, dev, absorb, order=None):
        """The head's workspace tensors by the names the backward uses: {name: tensor}, asked for in `order` (default: as
        listed here, the order of the composition _head(); the C stage passes _STAGE_ORDER)."""
        C, To, dec, st, f32, ws = self.d_model, self.out_len, self.decoder, self.storage, torch.float32, self._ws
        M, nh = B * To, dec.cross_nhead
        R = B * nh * To
        spec = dict(lane=((B, C * To), f32), dec0=((B, C * To), f32))
        if dec.use_post_mlp:
            spec.update(hid=((B, dec.post_mlp[0].weight.shape[0]), f32), dec1=((B, C * To), f32))
        spec.update(dect=((M, C), f32), dectb=((M, C), st), proj=((M, H), st), q=((M, H), st), S=((R, Lp), f32),
                    P=((R, Lp), torch.float16), att=((M, H), st))
        if absorb:
            spec.update(qp=((nh, M, H), st), ctx=((nh, M, H), st))
        spec.update(cross=((M, H), st), fused=((M, C), f32), fn=((M, C), f32), f1=((M, C), f32), f2=((M, C), f32))
        return {_RECORD_NAME.get(n, n): ws.get("lt." + n, *spec[n], dev) for n in (order or spec) if n in spec}

    def _head_stage(self, sv, add_last):
        """Phase 2 of tcavt_ltsf_forward: the launches of _head() below, from C++, on the same buffers (_head_bufs; the
        backward reads them from the record sv), continuing on the struct front() filled: the C entry reads it at the call, so
        what is added here changes nothing for phase 1, and the stage backward is handed the one struct."""
        dec, P, To = self.decoder, self._prepared(), self.out_len
        H, nh = sv.final_hidden_bf16.shape[1], dec.cross_nhead
        a, keep = sv.stage
        post = dec.post_mlp[0].weight.shape[0] if dec.use_post_mlp else 0
        sv.drop_post = _spec(self.dctx, self.dropout_p) if dec.use_post_mlp else None
        sv.drop_xattn = _spec(self.dctx, self.dropout_p)
        out = torch.empty((sv.B, self.feature_size, To), dtype=torch.float32, device=sv.x.device)
        names = ("x", "e", "poly_emb", "lane", "d0", "dec_t", "dec_tb", "proj", "cross", "fused", "fn", "f1", "f2") + \
            (("hid", "d1") if post else ())
        fl = dec.fusion_layer
        wts = dict(lane_w=dec.lane_fc.weight, lane_b=dec.lane_fc.bias, dec_w=P.dec_w, dec_b=P.dec_b, w_dp=P.w_dp, b_dp=dec.dec_proj.bias,
                   w_q=P.w_q, b_q=P.b_q, w_co=P.w_co, b_co=dec.cross_attn.out_proj.bias, w_un=P.w_un, b_un=dec.dec_unproj.bias,
                   fl_n_w=fl[0].weight, fl_n_b=fl[0].bias, fl1_w=fl[1].weight, fl1_b=fl[1].bias, fl3_w=fl[3].weight, fl3_b=fl[3].bias,
                   out_w=dec.out_proj.weight, out_b=dec.out_proj.bias)
        if post:
            wts.update(pm0_w=dec.post_mlp[0].weight, pm0_b=dec.post_mlp[0].bias, pm3_w=dec.post_mlp[3].weight,
                       pm3_b=dec.post_mlp[3].bias)
        capi.bind(a, keep, out=out, **{n: getattr(sv, n) for n in names}, **wts)
        capi.bind(a.xattn, keep, q=sv.q, wk_t=P.wk_T, w_v=P.w_v, b_v=P.b_v, fh=sv.final_hidden_bf16, fh_t=sv.fhT, qp=sv.qp,
                  scores=sv.S, probs=sv.P, ctx=sv.ctx, att=sv.att)
        a.xattn.B, a.xattn.To, a.xattn.L, a.xattn.Lp, a.xattn.H, a.xattn.nhead, a.xattn.dtype16 = sv.B, To, sv.L, sv.Lp, H, nh, capi.F16
        capi.bind_dropout(a.xattn, sv.drop_xattn)
        a.B, a.C, a.T, a.To, a.F, a.H, a.nhead_sa = sv.B, self.d_model, sv.T, To, self.feature_size, H, self.attn_block.nhead
        a.poly_dim, a.post_hidden, a.add_last = sv.poly_emb.shape[1], post, int(bool(add_last))
        if dec.use_post_mlp:  # the one site phase 2 draws from these fields.  Sites: the self-attention block drew first_site .. + 3
            # in front(), the post-MLP + 4 (the same triple again then; a post-MLP without dropout clears what front() wrote)
            post_spec = None if sv.drop_post is None else sv.drop_post[:2] + (sv.drop_post[2] - 4,)
            a.dropout_p, a.dropout_seed, a.first_site = capi.drop_spec(post_spec)
        ops.ltsf_forward(a, 2)
        sv.xattn_stage = (a.xattn, keep)
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
        B, dev, ws, P = x.shape[0], x.device, self._ws, self._prepared()
        L, H = final_hidden.shape[1], final_hidden.shape[2]
        x = x.contiguous()
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
        absorb = self.absorb_kv and self.storage == torch.float16  # (recorded: the backward follows the form the forward ran)
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
            # see the absorbed form in _head.
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
        if _front is None:
            self.front(x)
        stage = absorb and self._stage_ok(dev)
        sv, self._front = self._front, None  # front()'s part of the record: B, T, tok, xp, e, sab, sab_drop, stage
        vars(sv).update(L=L, Lp=Lp, x=x, poly_emb=lane_polygon_emb.contiguous(), final_hidden_bf16=final_hidden_bf16,
                        absorbed=absorb, xattn_stage=None, drop_post=None, drop_xattn=None, hid=None,
                        **(dict(fhT=fhT) if absorb else dict(k=kx, vT=vT)))
        vars(sv).update(self._head_bufs(B, Lp, H, dev, absorb, _STAGE_ORDER if stage else None))
        out = self._head_stage(sv, _fuse_last_residual) if stage else self._head(sv, _fuse_last_residual, main)
        self.saved = sv if self.save_for_backward else None
        return out

    def _head(self, sv, add_last, main):
        """The head as one launch per kernel, on the buffers of the record sv (`main`: the caller's stream, which the K / V
        projections' side stream joins before the scores; None on the CPU seam)."""
        B, T, L, Lp, x, fh16 = sv.B, sv.T, sv.L, sv.Lp, sv.x, sv.final_hidden_bf16
        C, To, dec, P = self.d_model, self.out_len, self.decoder, self._prepared()
        H, nh = fh16.shape[1], dec.cross_nhead
        dh, M = H // nh, B * To
        ops.gemm_f32(sv.poly_emb, dec.lane_fc.weight, out=sv.lane, bias=dec.lane_fc.bias)
        ops.ltsf_decode(sv.e, P.dec_w, P.dec_b, sv.lane, sv.d0, B, C, T, To)
        if dec.use_post_mlp:
            sv.drop_post = _spec(self.dctx, self.dropout_p)
            ops.gemm_f32(sv.d0, dec.post_mlp[0].weight, out=sv.hid, bias=dec.post_mlp[0].bias, relu=True, dropout=sv.drop_post)
            ops.gemm_f32(sv.hid, dec.post_mlp[3].weight, out=sv.d1, bias=dec.post_mlp[3].bias)
        else:
            sv.d1 = sv.d0
        ops.transpose_ct(sv.d1, sv.dec_t, sv.dec_tb, B, C, To)
        # cross attention over the LLM's final hidden states: K = V = final_hidden, no padding mask
        ops.gemm_bf16(sv.dec_tb, P.w_dp, out=sv.proj, bias=dec.dec_proj.bias)
        q, S, Pm, att = sv.q, sv.S, sv.P, sv.att
        ops.gemm_bf16(sv.proj, P.w_q, out=q, bias=P.b_q)
        sv.drop_xattn = _spec(self.dctx, self.dropout_p)
        if sv.absorbed:
            # Absorbed form.  With To (30) queries per sample against L (256) keys the K / V projections of the final hidden
            # states (2 x 2 M H^2 = 137 GFLOP, the head's two chip-filling GEMMs -- and three more in the backward) move to
            # the query / output side, where they cost 2 x 2 (B To) H^2 = 16 GFLOP:
            #     scores_h = q_h (fh W_k[h]^T + b_k)^T  =  (q_h W_k[h]) fh^T  + const per query   (softmax-invariant: b_k drops out)
            #     att_h    = P_h (fh W_v[h]^T + b_v)    =  (P_h fh) W_v[h]^T + b_v               (rows of P sum to 1)
            # Same arithmetic as nn.MultiheadAttention (train.py:795-798) in exact arithmetic; the rounding points move from
            # k, v to q' = q_h W_k[h] and ctx_h = P_h fh (oracle/forward.py restates both forms).
            qp, ctx, fhT = sv.qp, sv.ctx, sv.fhT
            if os.environ.get("TCAVT_PY_TLAYERS", "0") == "1":  # the per-launch Python composition (A/B, bit-identical)
                ops.transpose16(fh16, fhT, L, H, Lp, ld_in=H, ld_out=B * Lp, batch=B, s_in=L * H, s_out=Lp)
                for h in range(nh):
                    ops.gemm_bf16(q[:, h * dh:(h + 1) * dh], P.wk_T[h], out=qp[h])
                ops.gemm_batched(qp, fh16, S, M=To, N=Lp, K=H, lda=H, ldw=H, ldc=Lp, batch=B * nh, inner=nh,
                                 sA=(To * H, M * H), sW=(L * H, 0), sC=(nh * To * Lp, To * Lp), acc_scale=1.0 / math.sqrt(dh),
                                 tile=64)
                ops.softmax_rows(S, Pm, B * nh * To, L, Lp, Lp, Lp, dropout=sv.drop_xattn)
                ops.gemm_batched(Pm, fhT, ctx, M=To, N=H, K=Lp, lda=Lp, ldw=B * Lp, ldc=H, batch=B * nh, inner=nh,
                                 sA=(nh * To * Lp, To * Lp), sW=(Lp, 0), sC=(To * H, M * H), tile=64)
                for h in range(nh):
                    ops.gemm_bf16(ctx[h], P.w_v[h * dh:(h + 1) * dh], out=att[:, h * dh:(h + 1) * dh],
                                  bias=P.b_v[h * dh:(h + 1) * dh])
            else:  # one C call: tcavt_cross_attn_forward (csrc/tlayers.hip), the same launch sequence
                ca_args, keep = capi.CrossAttnArgs(), []
                capi.bind(ca_args, keep, q=q, wk_t=P.wk_T, w_v=P.w_v, b_v=P.b_v, fh=fh16, fh_t=fhT, qp=qp, scores=S,
                          probs=Pm, ctx=ctx, att=att)
                ca_args.B, ca_args.To, ca_args.L, ca_args.Lp, ca_args.H, ca_args.nhead = B, To, L, Lp, H, nh
                ca_args.dtype16 = capi.F16
                capi.bind_dropout(ca_args, sv.drop_xattn)
                ops.cross_attn_forward(ca_args)
                sv.xattn_stage = (ca_args, keep)
        else:
            if main is not None:
                main.wait_stream(self._kv_stream)
            # scores[b,h] = q_bh . k_bh^T / sqrt(dh)  (fp32), softmax -> fp16 probabilities (zero beyond L)
            ops.gemm_batched(q, sv.k, S, M=To, N=Lp, K=dh, lda=H, ldw=H, ldc=Lp, batch=B * nh, inner=nh,
                             sA=(To * H, dh), sW=(L * H, dh), sC=(nh * To * Lp, To * Lp), acc_scale=1.0 / math.sqrt(dh))
            ops.softmax_rows(S, Pm, B * nh * To, L, Lp, Lp, Lp, dropout=sv.drop_xattn)
            ops.gemm_batched(Pm, sv.vT, att, M=To, N=dh, K=Lp, lda=Lp, ldw=B * Lp, ldc=H, batch=B * nh, inner=nh,
                             sA=(nh * To * Lp, To * Lp), sW=(Lp, dh * B * Lp), sC=(To * H, dh))
        ops.gemm_bf16(att, P.w_co, out=sv.cross, bias=dec.cross_attn.out_proj.bias)
        ops.gemm_bf16(sv.cross, P.w_un, out=sv.fused, bias=dec.dec_unproj.bias, residual=sv.dec_t)
        fl = dec.fusion_layer
        ops.layernorm(sv.fused, fl[0].weight, fl[0].bias, 1e-5, out_f32=sv.fn)
        ops.gemm_f32(sv.fn, fl[1].weight, out=sv.f1, bias=fl[1].bias, relu=True)
        ops.gemm_f32(sv.f1, fl[3].weight, out=sv.f2, bias=fl[3].bias)
        out = torch.empty((B, self.feature_size, To), dtype=torch.float32, device=x.device)
        ops.out_head(sv.f2, dec.out_proj.weight, dec.out_proj.bias, x, out, B, To, C, self.feature_size, T, add_last=add_last)
        return out
