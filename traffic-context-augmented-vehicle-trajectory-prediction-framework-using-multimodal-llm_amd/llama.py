"""Llama decoder stack (HF LlamaForCausalLM layout) with LoRA on q_proj / v_proj over the C ABI: the holders, the packed
weight copies (prefill, backward transposes, decode, MX8, LM-loss table) and the one-call decoder pass (train.py:419-453)."""
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import capi, ops
from .config import LlamaShape
from .layout import LORA_V, interleave_gate_up
from .parts import _Linear, _Norm, _p, _Prepared, _spec, _to16, _Workspace
from .rope import rope_tables


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
        self._prep_T = self._prep_dec = self._prep_dec8 = self._prep_tableT = None
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
            capi.bind(carr[li], w_qkv=d.w_qkv, w_o=d.w_o, w_gu=d.w_gu, w_d=d.w_d)
            if self.use_lora:
                capi.bind(carr[li], a_cat=d.a_cat, b_ext=d.b_ext)
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
        if self._prep_tableT is None or self._prep_tableT[0] is not P:
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
        if dtype not in ("fp16", "fp8"):
            raise ValueError(f"decode_weights: dtype must be 'fp16' or 'fp8', got {dtype!r}")
        P = self._prepared()
        slot = "_prep_dec" if dtype == "fp16" else "_prep_dec8"
        pack = ops.pack_weight16 if dtype == "fp16" else ops.pack_weight8
        cached = getattr(self, slot)
        if cached is not None and cached.of is P:
            return cached
        ll = self.shape
        if ll.hidden % 256 or ll.inter % 256 or (ll.n_q_heads * ll.head_dim) % 256 or ll.vocab % 16:
            return None
        carr = capi.clone_layers(P.carr)
        keep = []
        with torch.no_grad():
            for c, d in zip(carr, P.layers):
                capi.bind(c, keep, w_qkv=pack(d.w_qkv), w_o=pack(d.w_o), w_gu=pack(d.w_gu), w_d=pack(d.w_d))
            table = pack(P.table)
        setattr(self, slot, SimpleNamespace(of=P, carr=carr, table=table, keep=keep))
        return getattr(self, slot)

    def mlp_weights(self, dtype="mx8"):
        """MX8 images (ops.quant_mx8, quant.quantize_mx: e4m3 codes + one E8M0 scale per 32 elements along K) of the frozen gate|up
        and down matrices for the opt-in MX8 MLP, and a copy of the layer array that names them (tcavt_llama_layer.w_gu8 ...).
        Quantised from the prepared 16-bit matrices, the norm gain already folded in.  A second, 33/64-size copy of the MLP
        weights (0.83 GB at the Llama-3.2-1B shape), made on the first MX8 pass and dropped with the packed weights it was made
        from, like decode_weights."""
        if dtype != "mx8":
            raise ValueError(f"mlp_weights: dtype must be 'mx8', got {dtype!r}")
        ll = self.shape
        if ll.hidden % 128 or ll.inter % 128:
            raise ValueError(f"mlp_weights: the MX8 MLP needs hidden and inter to be multiples of 128, got {ll.hidden} / {ll.inter}")
        P = self._prepared()
        if self._prep_mx8 is not None and self._prep_mx8.of is P:
            return self._prep_mx8
        carr = capi.clone_layers(P.carr)
        keep = []
        with torch.no_grad():
            for c, d in zip(carr, P.layers):
                gu, d8 = ops.quant_mx8(d.w_gu), ops.quant_mx8(d.w_d)
                keep.append((gu, d8))
                capi.bind(c, w_gu8=gu[0], w_gu8_scale=gu[1], w_d8=d8[0], w_d8_scale=d8[1])
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
            carr = capi.clone_layers(P.carr)
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
                capi.bind(carr[li], tape_h_mid=sv.h_mid, tape_h_out=sv.h_out, tape_qkv=sv.qkv_padded, tape_gu=sv.gu, tape_att=sv.att,
                          tape_lse=sv.lse, tape_part=sv.part, tape_t=sv.t)
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
            # (masks are applied inside tcavt_lora_down: no dropped copies of the stream)
            capi.bind_dropout(args, dq, p="lora_dropout_p", site="lora_first_site")
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
