"""Host-side mirror of the reference's model classes over the gfx950 C ABI: the top-level MultiModalTrajectoryModel, and
the names callers import from here.  The parts live by class in tlayers.py (LanePolygonEncoder, BlipQFormer), llama.py
(LlamaWithCrossAttnPEFT), mllm.py (LlamaMultiModal), ltsf.py (TransformerLTSF and its blocks) and parts.py (holders, workspace,
DropoutCtx).

Same class names, constructor kwargs, ``forward()`` signatures and ``state_dict()`` key
layout as the reference's scripts/train.py:352-964 (no-LoRA key layout of
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
import math
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import ops, streams
from .config import LlamaShape, ModelConfig
from .layout import LORA_V, XATTN_PAD  # noqa: F401  (re-exported, like the classes below: callers import them from here)
from .llama import LlamaWithCrossAttnPEFT  # noqa: F401
from .ltsf import LTSF_NLinearDecoder, LTSF_NLinearEncoder, SelfAttentionBlock, TransformerLTSF  # noqa: F401
from .mllm import GENERATION_CUTOFF_MARKER, LlamaMultiModal, cut_generated_text  # noqa: F401
from .parts import DropoutCtx, _Prepared
from .tlayers import BlipQFormer, LanePolygonEncoder  # noqa: F401


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
        if self._auto_range == "pending" and dev.type == "cuda" and self._llm_cache is None:
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
