"""LTSF blocks (train.py:659-842): the self-attention block, the per-channel N-Linear holders and TransformerLTSF, the
trajectory head with its cross-attention over the LLM's final hidden states (C stages of csrc/tlayers.hip, or the
per-launch Python compositions)."""
import contextlib
import math
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import capi, ops, streams
from .layout import XATTN_PAD
from .parts import _Linear, _MHA, _Norm, _p, _Prepared, _spec, _to16, _Workspace


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
        # the C stages' filled argument structs of the last forward with what their pointers name, (struct, keep-list): the
        # stage backwards are handed these (LtsfArgs: front() fills phase 1, _head_stage phase 2; CrossAttnArgs: the plain
        # tcavt_cross_attn_forward branch, or the head stage's embedded one)
        self.stage = self.xattn_stage = None

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
        self.stage = self.xattn_stage = None
        if self._stage_ok(dev):  # one C call: tcavt_ltsf_forward phase 1 (csrc/tlayers.hip), the same launch sequence
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
            capi.bind(a, keep, xp_tok=xp_tok, **bufs, **wts)
            a.B, a.C, a.T, a.To, a.F, a.nhead_sa = B, C, T, self.out_len, F, sab.nhead
            capi.bind_dropout(a, sp[0], site="first_site")
            ops.ltsf_forward(a, 1)
            self.stage = (a, keep)
            return bufs["e"]
        ops.ltsf_front(x, P.conv_w, self.token_proj.bias, P.enc_w, P.enc_b, P.pos, tok, B, C, T, xp_tok=xp_tok)
        return self.attn_block.forward_tokens(tok, B, T)

    def _head_stage(self, x, e, lane_polygon_emb, fh16, fhT, B, T, L, Lp, H, add_last):
        """Phase 2 of tcavt_ltsf_forward: the launches of forward() below, from C++, on the same named buffers (the backward's
        Python composition finds them by name), continuing on the struct front() filled: the C entry reads it at the call, so
        what is added here changes nothing for phase 1, and the stage backward is handed the one struct."""
        dev, C, To, ws = x.device, self.d_model, self.out_len, self._ws
        dec, P = self.decoder, self._prepared()
        nh = dec.cross_nhead
        M = B * To
        f32, st = torch.float32, self.storage
        g = lambda n, shape, dt=f32: ws.get("lt." + n, shape, dt, dev)
        a, keep = self.stage
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
        capi.bind(a, keep, **bufs, **wts)
        capi.bind(a.xattn, keep, **xa)
        a.xattn.B, a.xattn.To, a.xattn.L, a.xattn.Lp, a.xattn.H, a.xattn.nhead, a.xattn.dtype16 = B, To, L, Lp, H, nh, capi.F16
        capi.bind_dropout(a.xattn, self.drop_xattn)
        a.B, a.C, a.T, a.To, a.F, a.H, a.nhead_sa = B, C, T, To, self.feature_size, H, self.attn_block.nhead
        a.poly_dim, a.post_hidden, a.add_last = lane_polygon_emb.shape[1], post, int(bool(add_last))
        if dec.use_post_mlp:  # the one site phase 2 draws from these fields.  Sites: the self-attention block drew first_site .. + 3
            # in front(), the post-MLP + 4 (the same triple again then; a post-MLP without dropout clears what front() wrote)
            post_spec = None if self.drop_post is None else self.drop_post[:2] + (self.drop_post[2] - 4,)
            a.dropout_p, a.dropout_seed, a.first_site = capi.drop_spec(post_spec)
        ops.ltsf_forward(a, 2)
        self.xattn_stage = (a.xattn, keep)
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
                ca_args, keep = capi.CrossAttnArgs(), []
                capi.bind(ca_args, keep, q=q, wk_t=P.wk_T, w_v=P.w_v, b_v=P.b_v, fh=final_hidden_bf16, fh_t=fhT, qp=qp, scores=S,
                          probs=Pm, ctx=ctx, att=att)
                ca_args.B, ca_args.To, ca_args.L, ca_args.Lp, ca_args.H, ca_args.nhead = B, To, L, Lp, H, nh
                ca_args.dtype16 = capi.F16
                capi.bind_dropout(ca_args, self.drop_xattn)
                ops.cross_attn_forward(ca_args)
                self.xattn_stage = (ca_args, keep)
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
