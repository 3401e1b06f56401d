"""LlamaMultiModal (train.py:459-575): Q-Former image tokens + text tokens through the decoder, the opt-in LM loss /
evaluation passes and the text-generation entry points."""
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import generation, ops, streams
from .config import LlamaShape
from .layout import XATTN_PAD
from .llama import LlamaWithCrossAttnPEFT
from .parts import _Linear, _p, _Prepared, _to16, _Workspace
from .tlayers import BlipQFormer


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
        self._last_flags = self._lm_flag = self._pool_flag = self._request_flag = self._constraint_flag = None  # device error flags of the passes so far (check_flags)

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
        if self._lm_flag is not None and self._lm_flag.item():
            self._lm_flag.zero_()
            raise ValueError("labels contain ids outside [0, vocab) other than -100, or a label at or beyond a sample's valid length")
        if self._pool_flag is not None and self._pool_flag.item():
            self._pool_flag.zero_()
            raise ValueError("generate_pool: a grouped admission named a slot outside the pool (tcavt_slot_admit_group)")
        if self._request_flag is not None and self._request_flag.item():
            self._request_flag.zero_()
            raise ValueError("a sampler row named a request outside the per-request parameter table (tcavt_sample_tokens_per_request)")
        if self._constraint_flag is not None and self._constraint_flag.item():
            bits = int(self._constraint_flag.item())
            self._constraint_flag.zero_()
            raise RuntimeError("constrained decoding: " + "; ".join(why for bit, why in (
                (1, "the sampler chose a token that the row's state does not allow (tcavt_constraint_advance)"),
                (2, "a row named a request outside the table of start states"), (4, "a row's state word lies outside the automaton"))
                if bits & bit))
        if self._last_flags is None:
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
                       poll_every=None, num_return_sequences=1, share_prefix=False, prompt_lookup_num_tokens=None,
                       max_matching_ngram_size=2, constraint=None, constraint_start=None, top_logprobs=None, return_logprobs=False,
                       num_beams=1, length_penalty=1.0, early_stopping=False):
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
        ``top_logprobs`` = k, an int with 1 <= k <= 20 (OpenAI's name; vLLM logprobs=k; DESIGN.md section 7, "top-k alternatives");
        it needs return_logprobs=True, and a bool, another type or a k outside the range raises ValueError.  info gains
        "top_token_ids" int64 and "top_token_logprobs" float32 [B * n, max_new_tokens, k]: at every position a row generated, the
        k most likely tokens of the raw logits row by (score descending, id ascending) with their log_softmax(raw) values, from
        the sums token_logprobs uses -- where the emitted token is in the list its entry equals token_logprobs bit for bit.
        Positions a row never generated hold -1 / -inf.  One call of tcavt_logprob_topk (two launches) follows every
        logprob_begin, in the captured step too; tokens, token_logprobs, sum_logprob and n_scored are those of the call without.
        The list is of the model's own distribution: it ignores the sampling arguments, and with ``constraint`` it is of the
        unmasked row and may name tokens the row's state bans.  Everything return_logprobs works with works here; num_beams > 1
        and prompt_lookup_num_tokens refuse it as they refuse return_logprobs.  None, the default, is launch for launch and
        buffer for buffer the call without the argument, return_logprobs=True included.
        ``num_beams`` = n with 2 <= n <= 16 ("beam search"): the deterministic search of HF's
        generate(num_beams=n, do_sample=False), per prompt and independent of the other prompts, on the shared prompt cache
        (share_prefix is implied; passing it makes no difference).  It needs ``do_sample=False`` (beam sampling is not built:
        ValueError); temperature, top_k, top_p and seed are ignored as in HF; repetition_penalty and no_repeat_ngram_size act on the
        log-probabilities with history = the prompt's valid ids + the beam's tokens; eos_token_id ends a hypothesis.  A finished
        hypothesis scores sum of log-probabilities / length ** ``length_penalty`` (a finite float); ``early_stopping`` = False
        (HF's heuristic: stop once no running beam can beat the worst kept hypothesis) or True (stop as soon as n hypotheses are
        kept).  ``num_return_sequences`` = r with 1 <= r <= n returns the r best hypotheses per prompt, best first: row b * r + j is
        hypothesis j of prompt b, EOS kept and pad_token_id behind it.  One step is tcavt_llama_decode_step_shared ->
        tcavt_beam_select -> tcavt_beam_reorder at B * n rows; use_graph, poll_every and return_info work as above, and info holds
        "sequences_scores" float32 [B * r], "n_generated" int32 [B * r], "finish_reason" (1 EOS, 4 ran out), "steps" and
        "beam_trace" (per step, prompt and candidate k < 2 n: "parent", "token" int32 and "acc" float32 [steps + 1, B, 2 n]).
        ``decode_weights="fp8"`` needs B * n <= 32.  Refused with ValueError before anything touches a device: kv_cache="fp8",
        stop_token_ids / stop_sequences / min_new_tokens, return_logprobs=True, early_stopping="never", a vocabulary below 2 n, a
        num_beams that is no int in [1, 16], a length_penalty that is not finite.  num_beams = 1, the default, is launch for
        launch the call without the argument.  generate_pool does not take the three.
        ``prompt_lookup_num_tokens`` = k with 1 <= k <= 7 (HF's name; DESIGN.md section 7, "prompt-lookup decoding"): speculative
        decoding without a draft model.  Every step drafts up to k tokens per sequence -- the continuation of the earliest earlier
        occurrence of the sequence's last n ids, n from ``max_matching_ngram_size`` (1 .. 8) down to 1, in [the prompt's ids | the
        tokens so far] (tcavt_ngram_draft) --, runs the decoder on all k + 1 positions of every sequence at once
        (tcavt_llama_decode_step_multi, S * (k + 1) <= 32 rows, S = B * num_return_sequences) and commits the drafts the model
        would have chosen itself plus its own next token (tcavt_spec_verify): 1 .. k + 1 tokens per step.  Every position is
        selected by the plain sampler on the state the plain loop has at that token, with the uniform the plain loop draws there,
        so the tokens are those of the call without the argument wherever the decode step's logits do not depend on the row count
        (DESIGN.md states what was measured), sampled or greedy.  The loop runs at most max_new_tokens - 1 steps and reads the
        finished flags every ``poll_every`` steps (default 4 here); return_info adds "drafted" and "accepted" (host int32 per
        sequence) and "steps" counts the steps run.  decode_weights="fp8" and num_return_sequences > 1 work as above.  Refused with
        ValueError before anything touches a device: kv_cache="fp8", share_prefix=True, num_beams > 1, return_logprobs=True,
        stop_sequences, S * (k + 1) > 32, a pad_token_id outside the vocabulary (the rows behind a draft feed it to the step), a k
        or max_matching_ngram_size outside its range.  None, the default, is launch for launch the call without the argument.
        generate_pool does not take the two.
        Per-request parameters ("per-request parameters"): each of ``do_sample``, ``temperature``, ``top_k``,
        ``top_p``, ``repetition_penalty``, ``no_repeat_ngram_size``, ``eos_token_id`` (entries may be None), ``seed`` and
        ``min_new_tokens`` is one value, or a list / tuple / 1-D tensor of exactly B values, one per prompt; with
        ``num_return_sequences`` = n prompt b's value serves its n rows.  With a sequence among them the values go to the device
        once per call as a table of B * n entries (checked on the host first: a wrong length or an illegal element raises
        ValueError naming the argument and the index, before anything touches a device) and every sampler launch is
        tcavt_sample_tokens_per_request, which reads row r's parameters at entry r; a row then gets exactly the tokens, finish_reason,
        n_generated and log-probabilities it gets in the call where every prompt uses its values (wherever the decode step's logits
        do not depend on the row count).  share_prefix, kv_cache, decode_weights, the ending rules, poll_every, return_info and
        return_logprobs work as above; a positive minimum needs that prompt's own eos_token_id, or stop_token_ids.  ``pad_token_id``,
        ``stop_token_ids`` and ``stop_sequences`` stay one value per call.  Refused with ValueError together with num_beams > 1 or
        prompt_lookup_num_tokens (beam search and tcavt_spec_verify keep the one struct).  With nine single values the call is
        launch for launch, buffer for buffer and bit for bit the call without this.
        ``constraint`` = a constraint.TokenConstraint ("constrained decoding"): every row may only emit tokens
        that its automaton state allows -- HF's prefix_allowed_tokens_fn / suppress_tokens / allowed vocabulary, with the rule held
        on the device.  The automaton goes to the device once per call (tcavt_constraint_build: one allowed-token bitmap per
        state), and every token selection, in the captured step too, becomes [logprob_begin ->] tcavt_constraint_mask -> the
        selection entry the call takes anyway -> tcavt_constraint_advance [-> logprob_finish]: the mask writes -inf over the scores
        of the tokens the row's state does not allow (the sampler treats -inf as banned on every path; the repetition penalty and
        the warpers never un-ban a score, so this equals HF's order), the advance follows the chosen token.  Log-probabilities stay
        those of the raw row.  ``constraint_start``: None (the constraint's own start state), one state, or a list / tuple / 1-D
        tensor of B states, one per prompt (TokenConstraint.union returns the start of each member); with
        ``num_return_sequences`` = n every continuation of a prompt starts in the prompt's state.  return_info adds
        "constraint_state": the final state per row, host int32 [B * n].  decode_weights, kv_cache, num_return_sequences,
        share_prefix, return_logprobs, stop tokens and stop sequences, poll_every and per-request parameters work as above.
        Refused with ValueError before anything touches a device: num_beams > 1 (the per-row state would have to follow
        tcavt_beam_reorder), prompt_lookup_num_tokens (the verification runs the sampler pass by pass inside one kernel),
        no_repeat_ngram_size > 0 or min_new_tokens > 0 as one value or in any list element (either can ban every token a state
        allows, and the sampler has no defined answer on a row without a finite score; an automaton states a minimum length
        itself, and a form needs repeated n-grams) -- no_repeat_ngram_size defaults to 3 from the reference: pass 0 --, a
        constraint over another vocabulary, a start state outside the automaton.  With those excluded and every state validated
        non-empty no row reaches the sampler empty; a chosen token outside the state would set a flag that check_flags() raises
        as RuntimeError.  None, the default, is launch for launch and bit for bit the call without the argument.
        Returns int64 [B * n, max_new_tokens] token ids (pad_token_id after a row's end), or a list of B * n strings in the same
        order with a tokenizer."""
        out, info = generation.generate_batch(
            self, vision_embs_batch, context_str_list=context_str_list, max_new_tokens=max_new_tokens, input_ids=input_ids,
            attention_mask=attention_mask, do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p,
            repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, eos_token_id=eos_token_id,
            pad_token_id=pad_token_id, seed=seed, use_graph=use_graph, decode_weights=decode_weights, kv_cache=kv_cache,
            stop_token_ids=stop_token_ids, stop_sequences=stop_sequences, min_new_tokens=min_new_tokens, return_info=return_info,
            poll_every=poll_every, num_return_sequences=num_return_sequences, share_prefix=share_prefix,
            return_logprobs=return_logprobs, num_beams=num_beams, length_penalty=length_penalty, early_stopping=early_stopping,
            prompt_lookup_num_tokens=prompt_lookup_num_tokens, max_matching_ngram_size=max_matching_ngram_size,
            constraint=constraint, constraint_start=constraint_start, top_logprobs=top_logprobs)
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
                      stop_token_ids=None, stop_sequences=None, min_new_tokens=0, return_info=False, return_logprobs=False,
                      constraint=None, constraint_start=None, top_logprobs=None):
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
        sampler uses, and a request's three results do not depend on its slot, the schedule or its partners (for a fixed G).
        ``top_logprobs`` = k (1 <= k <= 20, needs return_logprobs=True; anything else raises ValueError): as in generate_batch,
        the stats gain "top_token_ids" int64 and "top_token_logprobs" float32 [R, max budget, k] -- the k most likely tokens of the
        raw row at every position request r generated, -1 / -inf elsewhere -- written by tcavt_logprob_topk after every
        logprob_begin of the three sampler uses; with ``constraint`` the list is of the unmasked row and may name banned tokens.
        A request's lists do not depend on its slot, the schedule or its partners (for a fixed G).
        Per-request parameters ("per-request parameters"): each of ``do_sample``, ``temperature``, ``top_k``,
        ``top_p``, ``repetition_penalty``, ``no_repeat_ngram_size``, ``eos_token_id`` (entries may be None), ``seed`` and
        ``min_new_tokens`` is one value, or a list / tuple / 1-D tensor of exactly R values -- a greedy request next to sampled ones,
        every request its own temperature or seed, in ONE call.  With a sequence among them the values are checked on the host (a
        wrong length or an illegal element raises ValueError naming the argument and the index; nothing is launched, no workspace
        buffer requested), uploaded once as a table of R entries, and all three sampler uses become
        tcavt_sample_tokens_per_request, which reads a row's parameters at its request index out_row[slot]; the captured graphs
        stay valid.  Request r then gets exactly the tokens, finish_reason, n_generated and log-probabilities that it gets in the
        call where all requests use its values: the independence from slot, schedule, group row and partners extends to the
        partners' parameters (for a fixed G).  A positive minimum needs that request's own eos_token_id, or stop_token_ids.
        ``pad_token_id`` (idle and finished slots feed it to the decode step), ``stop_token_ids`` and ``stop_sequences`` stay one
        value per call.  A row that names a request outside the table is inert and sets a flag that check_flags() reports.  With
        nine single values the call is launch for launch, buffer for buffer and bit for bit the call without this.
        ``constraint`` / ``constraint_start``: constrained decoding as in generate_batch, around all three sampler uses;
        ``constraint_start`` is one state or one per request, so that the requests of one list can follow different forms
        (TokenConstraint.union).  A slot's state is reset by the rule itself -- a row whose step word is 0 takes its request's start
        state -- so the admission launches are unchanged, and a request's tokens stay independent of slot, schedule and partners
        (for a fixed G).  return_info adds "constraint_state": host int32 [R], every request's final state.  Refused with
        ValueError before anything touches a device: no_repeat_ngram_size > 0 (the default is 3: pass 0) or min_new_tokens > 0, as
        one value or in any list element; a constraint over another vocabulary; a start state outside the automaton."""
        out, stats = generation.generate_pool(
            self, vision_embs, input_ids=input_ids, attention_mask=attention_mask, max_new_tokens=max_new_tokens, slots=slots,
            poll_every=poll_every, do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p,
            repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, eos_token_id=eos_token_id,
            pad_token_id=pad_token_id, seed=seed, use_graph=use_graph, decode_weights=decode_weights, kv_cache=kv_cache,
            admit_group=admit_group, stop_token_ids=stop_token_ids, stop_sequences=stop_sequences, min_new_tokens=min_new_tokens,
            return_info=return_info, return_logprobs=return_logprobs, constraint=constraint, constraint_start=constraint_start,
            top_logprobs=top_logprobs)
        res = self._generated_texts(out)
        return (res, stats) if return_info or return_logprobs else res
