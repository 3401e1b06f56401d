"""Host side of text generation: what LlamaMultiModal.generate_batch and generate_pool run.  The user
contract -- arguments, defaults, semantics -- is documented on those two methods (mllm.py); this module is the code behind them,
one piece per job:

  Prefill          image tokens + prompt through the decoder into a KV cache, last rows through the lm_head -> first logits
  select           the one place that chooses a sampler entry (tcavt_sample_logits[_slots|_rows] / tcavt_sample_tokens[_per_request])
  Selection        what one call puts around every select: built once per call from the request table, the ending rules and the
                   two records below, called at every token selection ([logprob_begin -> [logprob_topk]] -> [constraint_mask] ->
                   select -> [constraint_advance] -> [logprob_finish]), and the source of the records' host-side results
  LogprobRecord    return_logprobs: the three score tensors and the arguments of the tcavt_logprob_begin / _finish bracket;
                   rank_continuations orders a prompt's n continuations by them (host only);
                   top_logprobs = k (check_top_logprobs): the two list tensors and tcavt_logprob_topk right after begin
  ConstraintRecord, check_constraint   constraint=: the device table, the per-row states and the arguments of the
                   tcavt_constraint_mask / _advance bracket, inside the log-probability bracket; the argument checks
  prompt_tokens, begin, shared_prefix_state   what generate_batch and beam_search share: the prompt and its checks, the move to
                   the device (begin: every entry; it drops the last call's error flags), the rows on a shared prompt cache
  capture          "it has run eagerly once; capture it as a hipGraph" -> the callable that replays it
  FinishedPoll     the finished flags to pinned host memory and an event wait
  decode_loop      the N - 1 steps behind the first selection: one eager, the rest replayed, polled or not
  check_prompt_lookup, prompt_lookup_step   generate_batch(prompt_lookup_num_tokens = k): the argument checks, and the step
                   tcavt_ngram_draft -> tcavt_llama_decode_step_multi -> tcavt_spec_verify that commits 1 .. k + 1 tokens
  beam_search      generate_batch(num_beams > 1): tcavt_beam_select / tcavt_beam_reorder around the shared-prefix decode step
  decode_args      the tcavt_decode_args of the decode step
  request_params   the nine sampling arguments -> the call's struct and, when one of them is given per request, the device table
  sample_params, eval_arithmetic, the check_* / stop_rules argument checks, cache_buffers (with the KV8 plane table)

Workspace names and the order in which they are first requested are part of what tests/test_generation_trace_cpu.py pins;
``Prefill.reserve`` exists so that the pool can request a prefill's buffers where that order has them."""
import contextlib
import math
import numbers
import os
from types import SimpleNamespace

import torch

from . import capi, ops
from .pool import SlotScheduler
from .constraint import TokenConstraint
from .stopping import BUDGET, StopRules

I32, I64 = torch.int32, torch.int64
KV8_PLANES = (("kc", 64), ("ks", 2), ("vc", 64), ("vs", 2))  # plane -> bytes per cached row and kv head (quant.kv8_quantize)


# --------------------------------------------------------------------------------------
# argument checks shared by both entries (each entry calls them in its own, fixed order; nothing here touches a device)
# --------------------------------------------------------------------------------------
def check_format(who, name, value):
    if value not in ("fp16", "fp8"):
        raise ValueError(f"{who}: {name} must be 'fp16' or 'fp8', got {value!r}")


def stop_rules(who, mllm, stop_token_ids, stop_sequences, min_new_tokens, eos_token_id):
    rules = StopRules(mllm.llama_wrapper.shape.vocab, stop_token_ids, stop_sequences, min_new_tokens)
    if rules.min_new_tokens > 0 and eos_token_id is None and not rules.stop_token_ids:
        raise ValueError(f"{who}: min_new_tokens needs eos_token_id or stop_token_ids (nothing to ban)")
    return rules


def check_fp8_weights(who, decode_weights, rows, rows_name):
    if decode_weights == "fp8":
        if rows > 32:
            raise ValueError(f"{who}: decode_weights='fp8' runs on the skinny decode path only ({rows_name} <= 32), "
                             f"got {rows_name} = {rows}")
        if os.environ.get("TCAVT_DECODE_ROWMAJOR", "0") == "1":
            raise ValueError(f"{who}: decode_weights='fp8' has no row-major form (TCAVT_DECODE_ROWMAJOR=1 is set)")


# --------------------------------------------------------------------------------------
# the pieces
# --------------------------------------------------------------------------------------
@contextlib.contextmanager
def eval_arithmetic(mllm):
    """Generation runs eval arithmetic (model.eval() at train.py:581): no dropout context, no decoder tape, no autograd.  The
    decoder's two settings are put back afterwards; the Q-Former's dropout context stays None."""
    LW = mllm.llama_wrapper
    with torch.no_grad():
        was_dctx, LW.dctx, mllm.qformer.dctx = LW.dctx, None, None
        was_saving, LW.save_for_backward = LW.save_for_backward, False
        try:
            yield
        finally:
            LW.dctx, LW.save_for_backward = was_dctx, was_saving


def sample_params(temperature, top_p, repetition_penalty, top_k, no_repeat_ngram_size, do_sample, eos_token_id, pad_token_id, seed):
    return capi.SampleParams(float(temperature), float(top_p), float(repetition_penalty), int(top_k), int(no_repeat_ngram_size),
                             int(bool(do_sample)), -1 if eos_token_id is None else int(eos_token_id), int(pad_token_id),
                             int(seed) & 0xFFFFFFFFFFFFFFFF)


PER_REQUEST_ARGS = ("do_sample", "temperature", "top_k", "top_p", "repetition_penalty", "no_repeat_ngram_size", "eos_token_id", "seed",
                    "min_new_tokens")


def per_request_names(**nine):
    """The names among the nine sampling arguments that are given per request: a list, a tuple or a 1-D tensor."""
    return [k for k, v in nine.items() if isinstance(v, (list, tuple)) or (isinstance(v, torch.Tensor) and v.dim() >= 1)]


def request_params(who, n_req, repeat, rules, pad_token_id, **nine):
    """The nine sampling arguments -> (sp, table).  sp: the call's tcavt_sample_params (the values of request 0 where an argument is
    given per request; it carries pad_token_id).  table: None when every argument is one value -- the call is then the call of
    today -- else an ops.RequestTable of n_req * repeat entries, request-major (generate_batch: a prompt's value serves its
    ``repeat`` continuations), built and checked on the host; ``table.to(device)`` uploads it.  A wrong length or an illegal
    element raises ValueError naming the argument and the index; nothing here touches a device."""
    assert tuple(nine) == PER_REQUEST_ARGS
    names = per_request_names(**nine)
    if not names:
        return sample_params(nine["temperature"], nine["top_p"], nine["repetition_penalty"], nine["top_k"], nine["no_repeat_ngram_size"],
                             nine["do_sample"], nine["eos_token_id"], pad_token_id, nine["seed"]), None
    cols = {}
    for k, v in nine.items():
        if k in names:
            v = v.tolist() if isinstance(v, torch.Tensor) else list(v)
            if isinstance(nine[k], torch.Tensor) and nine[k].dim() != 1:
                raise ValueError(f"{who}: {k} must be one value or a 1-D sequence, got a {nine[k].dim()}-D tensor")
            if len(v) != n_req:
                raise ValueError(f"{who}: {k} has {len(v)} values for {n_req} requests")
        else:
            v = [v] * n_req
        cols[k] = v
    if n_req == 0:
        return None, None
    has_stop = bool(rules.stop_token_ids)
    params, mins = [], []
    for r in range(n_req):
        c = {k: cols[k][r] for k in PER_REQUEST_ARGS}

        def bad(k, why):
            return ValueError(f"{who}: {k}[{r}] = {c[k]!r} {why}" if k in names else f"{who}: {k} = {c[k]!r} {why} (request {r})")

        for k in PER_REQUEST_ARGS:  # numbers only (bool counts as one); eos_token_id may be None
            if not (isinstance(c[k], numbers.Real) or (k == "eos_token_id" and c[k] is None)):
                raise bad(k, "is not a number")
        for k in ("top_k", "no_repeat_ngram_size", "seed", "min_new_tokens", "eos_token_id"):
            if c[k] is not None and int(c[k]) != c[k]:
                raise bad(k, "is not an integer")
        if c["do_sample"]:
            if not c["temperature"] > 0:
                raise bad("temperature", "must be > 0 when sampling")
            if not 1 <= c["top_k"] <= 256:
                raise bad("top_k", "outside [1, 256] when sampling")
            if not 0 < c["top_p"] <= 1:
                raise bad("top_p", "outside (0, 1] when sampling")
        if not c["repetition_penalty"] > 0:
            raise bad("repetition_penalty", "must be > 0")
        if c["no_repeat_ngram_size"] < 0:
            raise bad("no_repeat_ngram_size", "must be >= 0")
        if c["min_new_tokens"] < 0:
            raise bad("min_new_tokens", "must be >= 0")
        try:
            rules.check_bannable(int(c["min_new_tokens"]), c["eos_token_id"])
        except ValueError:
            raise bad("min_new_tokens", "needs the request's eos_token_id or stop_token_ids (nothing to ban)") from None
        params.append(sample_params(c["temperature"], c["top_p"], c["repetition_penalty"], c["top_k"], c["no_repeat_ngram_size"],
                                    c["do_sample"], c["eos_token_id"], pad_token_id, c["seed"]))
        mins.append(int(c["min_new_tokens"]))
    try:
        table = ops.RequestTable([p_ for p_ in params for _ in range(repeat)],
                                 [m_ for m_ in mins for _ in range(repeat)] if any(mins) else None, has_stop_bitmap=has_stop)
    except capi.TcavtError as e:
        raise ValueError(f"{who}: {e}") from None
    return params[0], table


def sample_workspace(ws, name, rows, dev):
    """Workspace of the two-stage token selection (rows x 16 workgroups + one per sample) for ``rows`` logits rows, or None:
    the samplers then take their one-workgroup form."""
    if os.environ.get("TCAVT_SAMPLE_ONE_STAGE", "0") == "1":  # (A/B switch)
        return None
    return ws.get(name, (int(capi.lib().tcavt_sample_workspace_bytes(rows)),), torch.uint8, dev, zero=True)


def cache_buffers(ws, tag, LW, kv_cache, B, rows, dev, zero=False):
    """The KV cache of B samples x ``rows`` positions under ``tag``: the 16-bit pair (k, v), or the four KV8 planes."""
    ll = LW.shape
    if kv_cache == "fp8":
        return tuple(ws.get(f"{tag}.kv8.{nm}", (ll.layers, B, ll.n_kv_heads, rows, per), torch.uint8, dev, zero=zero)
                     for nm, per in KV8_PLANES)
    return tuple(ws.get(f"{tag}.{nm}", (ll.layers, B, rows, ll.n_kv_heads * ll.head_dim), LW.storage, dev, zero=zero)
                 for nm in ("kc", "vc"))


class Prefill:
    """The ordinary batched decoder pass over [image tokens | prompt] at B rows that writes a KV cache of ``cache_rows``
    positions and ends in the logits of every row's last valid position.  Its buffers live in the workspace as ``{tag}.h``
    (fp32 stream; not with the 16-bit stream), ``.kvlen``, ``.final16``, ``.x16``, ``.logits`` and the cache (``.kc`` / ``.vc`` or
    ``.kv8.{kc,ks,vc,vs}``): ``buf(name)`` hands one out ("cache": the tuple), requesting it on first use."""

    def __init__(self, mllm, tag, B, Lt, cache_rows, kv_cache, dev):
        LW = mllm.llama_wrapper
        self.mllm, self.tag, self.B, self.cache_rows, self.kv_cache, self.dev = mllm, tag, B, cache_rows, kv_cache, dev
        self.L = mllm.qformer.num_query_tokens + Lt
        self.P, self.PL = mllm._prepared(), LW._prepared()
        H, M = mllm.llama_hidden_size, B * self.L
        self.specs = dict(h=((M, H), torch.float32), kvlen=((B,), I32), final16=((M, H), LW.storage), x16=((B, H), LW.storage),
                          logits=((B, LW.shape.vocab), torch.float32))
        self.flags = None  # mm.flags of the last run

    def buf(self, name):
        m = self.mllm
        if name == "cache":
            return cache_buffers(m._ws, self.tag, m.llama_wrapper, self.kv_cache, self.B, self.cache_rows, self.dev)
        if name == "h" and m.llama_wrapper.stream16:
            return None
        return m._ws.get(f"{self.tag}.{name}", *self.specs[name], self.dev)

    def reserve(self, *names):
        for name in names:
            self.buf(name)

    def run(self, vision, ids, mask64, after_stack=None):
        """vision [B, ...], ids int64 [B, Lt], mask64 int64 [B, Lt] (right padded) -> fp32 logits [B, vocab] of the first new
        token.  ``after_stack`` runs between the decoder stack and the gather of the last rows (the pool's admission launch)."""
        m, B, L, dev = self.mllm, self.B, self.L, self.dev
        LW, P, PL = m.llama_wrapper, self.P, self.PL
        H, Nq = m.llama_hidden_size, m.qformer.num_query_tokens
        img = m._image_tokens(vision)
        h = self.buf("h")
        flags = self.flags = m._last_flags = m._ws.get("mm.flags", (3,), I32, dev, zero=True)
        h16, part = LW.norm_inputs(B * L, dev)
        ops.embed_fuse(PL.table, ids, img, P.vis, P.txt, h, flags[0:1], h16=h16, part=part, npart=LW.norm_npart(B * L),
                       stream_scale=LW.stream_scale)
        kv_len = self.buf("kvlen")
        ops.mask_to_kvlen(mask64, Nq, kv_len, flags[1:2])
        cache, final16 = self.buf("cache"), self.buf("final16")
        LW.decoder_stack(h, kv_len, B, L, out_bf16=final16, kv_cache=cache + (self.cache_rows,), nonfinite_flag=flags[2:3])
        if after_stack is not None:
            after_stack()
        x16 = self.buf("x16")
        ops.gather_last(final16, kv_len, x16, B, L, H)
        logits = self.buf("logits")
        ops.gemm_bf16(x16, PL.table, out=logits)  # lm_head, tied to embed_tokens
        return logits


def slot_state(history, hist_len, step, cur, pos, finished, max_new=None, out_row=None, cstate=None):
    """The device-resident generation state the samplers advance: one row / entry per sample (step: one word), or -- with
    max_new and out_row -- per decode slot.  cstate: the automaton state words of a constrained call (ConstraintRecord)."""
    return SimpleNamespace(history=history, hist_len=hist_len, step=step, cur=cur, pos=pos, finished=finished, max_new=max_new,
                           out_row=out_row, cstate=cstate)


def slot_view(st, s):
    """The state of slot s alone, as views (the one-row logits of a request being admitted)."""
    return slot_state(*(t[s:s + 1] for t in (st.history, st.hist_len, st.step, st.cur, st.pos, st.finished, st.max_new, st.out_row)),
                      cstate=None if st.cstate is None else st.cstate[s:s + 1])


def check_bool(who, name, value):
    if not isinstance(value, bool):
        raise ValueError(f"{who}: {name} must be a bool, got {value!r}")


class LogprobRecord:
    """The scores of return_logprobs: device tensors indexed like ``out`` (token_logprobs fp32 [rows, N] filled with 0.0, as out
    is with the pad id; sum_logprob fp32 [rows]; n_scored int32 [rows]) and the workspaces of the tcavt_logprob_begin / _finish
    bracket, one per logits shape, under ``{tag}.lp.ws`` -- new names, requested only with the flag.  ``top_k`` (top_logprobs = k):
    also top_ids int32 and top_logprobs fp32 [rows, N, k], filled with -1 / -inf (the kernel writes the positions a live row
    generates and nothing else), and the workspaces of tcavt_logprob_topk under ``{tag}.lp.top.ws``, requested only with it."""

    def __init__(self, ws, out, top_k=None):
        rows, dev = out.shape[0], out.device
        self.ws, self.out, self.top_k = ws, out, top_k
        self.token_logprobs = torch.zeros(out.shape, dtype=torch.float32, device=dev)
        self.sum_logprob = torch.zeros(rows, dtype=torch.float32, device=dev)
        self.n_scored = torch.zeros(rows, dtype=I32, device=dev)
        if top_k is not None:
            self.top_ids = torch.full(tuple(out.shape) + (top_k,), -1, dtype=I32, device=dev)
            self.top_logprobs = torch.full(tuple(out.shape) + (top_k,), float("-inf"), dtype=torch.float32, device=dev)

    def reserve(self, tag, rows, hist_cap):
        """The bracket's workspace for ``rows`` logits rows under ``tag`` (requested here, so before any capture)."""
        return self.ws.get(f"{tag}.lp.ws", (ops.logprob_workspace_bytes(rows, hist_cap),), torch.uint8, self.out.device)

    def args(self, tag, logits, st, slot_of_row):
        return ops.logprob_args(logits, st.history, st.hist_len, st.step, st.finished, self.out, self.token_logprobs, self.sum_logprob,
                                self.n_scored, self.reserve(tag, logits.shape[0], st.history.shape[1]), out_row=st.out_row,
                                slot_of_row=slot_of_row)

    def topk_args(self, tag, largs):
        """The tcavt_logprob_topk launch inside the bracket ``largs`` (its workspace requested here, so before any capture)."""
        wsb = self.ws.get(f"{tag}.lp.top.ws", (ops.logprob_topk_workspace_bytes(largs.rows, self.top_k),), torch.uint8, self.out.device)
        return ops.logprob_topk_args(largs, self.out, self.top_ids, self.top_logprobs, wsb)

    def host(self):
        res = dict(token_logprobs=self.token_logprobs.cpu(), sum_logprob=self.sum_logprob.cpu(), n_scored=self.n_scored.cpu())
        if self.top_k is not None:
            res.update(top_token_ids=self.top_ids.cpu().to(I64), top_token_logprobs=self.top_logprobs.cpu())
        return res


def check_top_logprobs(who, top_logprobs, return_logprobs):
    """top_logprobs = k -> k as an int, None -> None.  Nothing here touches a device."""
    if top_logprobs is None:
        return None
    k = top_logprobs
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= ops.TOP_LOGPROBS_MAX:
        raise ValueError(f"{who}: top_logprobs must be None or an int in [1, {ops.TOP_LOGPROBS_MAX}], got {top_logprobs!r}")
    if return_logprobs is not True:
        raise ValueError(f"{who}: top_logprobs needs return_logprobs=True (got return_logprobs={return_logprobs!r})")
    return int(k)


def rank_continuations(sum_logprob, n_scored, n, length_penalty=1.0):
    """The n continuations of every prompt, best first: int64 [B, n] of indices j (row b * n + j of a generate_batch result with
    num_return_sequences = n) ordered by sum_logprob / n_scored ** length_penalty, descending; ties go to the lower index.
    length_penalty = 1.0 is the mean log-probability per token, 0.0 the plain sum.  Host only (float64)."""
    n = int(n)
    s = torch.as_tensor(sum_logprob).detach().cpu().to(torch.float64).reshape(-1)
    k = torch.as_tensor(n_scored).detach().cpu().to(torch.float64).reshape(-1)
    if n < 1 or s.numel() != k.numel() or s.numel() % n != 0:
        raise ValueError(f"rank_continuations: {s.numel()} sums and {k.numel()} counts do not make rows of n = {n}")
    score = (s / k.clamp(min=1.0) ** float(length_penalty)).reshape(-1, n)
    return torch.argsort(score, dim=1, descending=True, stable=True)


def check_constraint(who, mllm, constraint, constraint_start, num_beams, prompt_lookup_num_tokens, no_repeat_ngram_size, min_new_tokens):
    """The arguments of a call with ``constraint`` or ``constraint_start`` set (the start states themselves are checked by
    TokenConstraint.starts once the number of requests is known).  Nothing here touches a device."""
    if constraint is None:
        raise ValueError(f"{who}: constraint_start needs a constraint")
    if not isinstance(constraint, TokenConstraint):
        raise ValueError(f"{who}: constraint must be a constraint.TokenConstraint or None, got {type(constraint).__name__}")
    for name, bad, why in (("num_beams > 1", num_beams != 1, "the per-row state would have to follow tcavt_beam_reorder"),
                           ("prompt_lookup_num_tokens", prompt_lookup_num_tokens is not None,
                            "the verification runs the sampler pass by pass inside one kernel")):
        if bad:
            raise ValueError(f"{who}: constraint is not built for {name} ({why})")

    def values(v):
        return v.reshape(-1).tolist() if isinstance(v, torch.Tensor) else list(v) if isinstance(v, (list, tuple)) else [v]

    # either can ban every token a state allows, and the sampler has no defined answer on a row without a finite score
    if any(isinstance(v, numbers.Real) and v > 0 for v in values(no_repeat_ngram_size)):
        raise ValueError(f"{who}: constraint needs no_repeat_ngram_size = 0, got {no_repeat_ngram_size!r} (the default is the reference's "
                         "3: pass 0; a form repeats n-grams, and the ban can empty a row's allowed set)")
    if any(isinstance(v, numbers.Real) and v > 0 for v in values(min_new_tokens)):
        raise ValueError(f"{who}: constraint needs min_new_tokens = 0, got {min_new_tokens!r} (the automaton states a minimum length "
                         "itself, and the ban can empty a row's allowed set)")
    vocab = mllm.llama_wrapper.shape.vocab
    if constraint.vocab != vocab:
        raise ValueError(f"{who}: constraint is over {constraint.vocab} token ids, the model's vocabulary has {vocab}")


class ConstraintRecord:
    """The device side of a call's ``constraint``: the table (uploaded and built here, once per call: tcavt_constraint_build), the
    start state of every request, the state word of every sample / slot, the final state per request, the flag word, and the
    workspaces of the tcavt_constraint_mask / _advance bracket, one per logits shape, under ``{tag}.cs.ws`` -- new names,
    requested only with a constraint.  Without a state row (an empty request list) there is no table: nothing is launched."""

    def __init__(self, ws, constraint, starts, n_state, dev):
        self.ws, self.dev = ws, dev
        self.table = ops.ConstraintTable(constraint.token_class, constraint.trans, dev).build() if n_state else None
        self.start = starts.to(dev)
        self.state = torch.zeros(n_state, dtype=I32, device=dev)
        self.request_state = self.start.clone()
        self.flag = torch.zeros(1, dtype=I32, device=dev)

    def reserve(self, tag, rows):
        """The bracket's workspace for ``rows`` logits rows under ``tag`` (requested here, so before any capture)."""
        return self.ws.get(f"{tag}.cs.ws", (ops.constraint_workspace_bytes(rows),), torch.uint8, self.dev)

    def args(self, tag, logits, st, slot_of_row):
        return ops.constraint_args(self.table, logits, st.step, st.finished, st.cur, st.cstate, self.start,
                                   self.reserve(tag, logits.shape[0]), out_row=st.out_row, slot_of_row=slot_of_row,
                                   request_state=self.request_state, flag=self.flag)

    def host(self):
        return dict(constraint_state=self.request_state.cpu())


def select(logits, st, sp, out, advance_pos, workspace, drules, slot_of_row=None, table=None):
    """Logits processors + token selection on the state ``st``.  The form follows from the arguments: ``slot_of_row`` -> the rows
    of a grouped admission, a state with max_new / out_row -> decode slots, neither -> a batch.  Without ending rules or records
    (``drules`` None) the launch is the form's own entry, otherwise tcavt_sample_tokens.  ``table`` (an uploaded
    ops.RequestTable): tcavt_sample_tokens_per_request in the place of whichever entry the call would otherwise take."""
    if table is not None or drules is not None:
        ops.sample_tokens(logits, st.history, st.hist_len, sp, st.step, st.cur, st.pos, st.finished, out, advance_pos=advance_pos,
                          workspace=workspace, max_new=st.max_new, out_row=st.out_row, slot_of_row=slot_of_row, stop=drules,
                          per_request=table)
    elif slot_of_row is not None:
        ops.sample_logits_rows(logits, slot_of_row, st.history, st.hist_len, sp, st.step, st.max_new, st.out_row, st.cur, st.pos,
                               st.finished, out, advance_pos=advance_pos, workspace=workspace)
    elif st.max_new is not None:
        ops.sample_logits_slots(logits, st.history, st.hist_len, sp, st.step, st.max_new, st.out_row, st.cur, st.pos, st.finished,
                                out, advance_pos=advance_pos, workspace=workspace)
    else:
        ops.sample_logits(logits, st.history, st.hist_len, sp, st.step, st.cur, st.pos, st.finished, out, advance_pos=advance_pos,
                          workspace=workspace)


class Selection:
    """What one call of a generate entry puts around every ``select``, built once per call (the device arrays are then fixed, so
    a captured step stays valid): the request table uploaded, the ending rules with the per-request records (``drules``: with
    rules or return_info), the LogprobRecord (return_logprobs; ``n_top``: top_logprobs) and the ConstraintRecord (one upload and
    one tcavt_constraint_build) over the output rows ``out``, and the two flags that mllm.check_flags reads.  ``st``: the state
    the call selects on, which gains the constraint's state words (a slot's is reset by the rule itself, at step 0) -- or None
    for an empty request list: the records alone, and nothing is launched."""

    def __init__(self, mllm, sp, table, rules, return_info, return_logprobs, n_top, constraint, starts, out, st):
        ws, dev = mllm._ws, out.device
        self.sp, self.out, self.return_info = sp, out, return_info
        self.table = self.cs = None
        if table is not None:
            self.table = table.to(dev)
            mllm._request_flag = table.flag
        self.drules = rules.to(dev).records(out.shape[0], dev) if return_info or not rules.empty else None
        self.lp = LogprobRecord(ws, out, n_top) if return_logprobs else None  # (the flag alone does not change the sampler entry)
        if constraint is not None:
            self.cs = ConstraintRecord(ws, constraint, starts, 0 if st is None else st.finished.shape[0], dev)
            if st is not None:
                st.cstate, mllm._constraint_flag = self.cs.state, self.cs.flag

    def __call__(self, logits, st, advance_pos, tag, workspace, slot_of_row=None):
        """One token selection on ``logits`` and ``st`` (the call's state, or a slot_view of it).  The brackets' workspaces live
        under ``tag``, one per logits shape, requested at first use.  tcavt_logprob_begin / _finish read the raw row before
        anything touches it and the chosen token afterwards, tcavt_logprob_topk takes the raw row's k best right after begin;
        tcavt_constraint_mask / _advance sit inside them -- the scores stay those of the raw row; select is the one without."""
        lp, cs = self.lp, self.cs
        if lp is not None:
            largs = lp.args(tag, logits, st, slot_of_row)
            ops.logprob_begin(largs)
            if lp.top_k is not None:
                ops.logprob_topk(lp.topk_args(tag, largs))
        if cs is not None:
            cargs = cs.args(tag, logits, st, slot_of_row)
            ops.constraint_mask(cargs)
        select(logits, st, self.sp, self.out, advance_pos, workspace, self.drules, slot_of_row, self.table)
        if cs is not None:
            ops.constraint_advance(cargs)
        if lp is not None:
            ops.logprob_finish(largs)

    def host(self, finish=True):
        """The records on the host, as the entries return them: finish_reason / n_generated (``finish``, and where the call has
        them), the scores of return_logprobs, constraint_state under return_info."""
        res = {}
        if finish and self.drules is not None:
            res.update(finish_reason=self.drules.finish_reason.cpu(), n_generated=self.drules.n_generated.cpu())
        if self.lp is not None:
            res.update(self.lp.host())
        if self.cs is not None and self.return_info:
            res.update(self.cs.host())
        return res


def capture(fn, dev, use_graph):
    """``fn`` has run eagerly once -- the warm-up of its workspaces and of every kernel form it uses.  -> the callable for its
    later runs: the replay of a hipGraph captured here (the capture launches nothing), or ``fn`` itself without graphs."""
    if not (use_graph and dev.type == "cuda"):
        return fn
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


class FinishedPoll:
    """Reads the finished flags back: [n] int32 to pinned host memory, then an event wait."""

    def __init__(self, n, dev):
        cuda = dev.type == "cuda"
        self.host = torch.empty(n, dtype=I32).pin_memory() if cuda else torch.empty(n, dtype=I32)
        self.event = torch.cuda.Event() if cuda else None

    def read(self, finished):
        self.host.copy_(finished, non_blocking=True)
        if self.event is not None:
            self.event.record()
            self.event.synchronize()
        return self.host


def decode_loop(one_step, N, rows, dev, use_graph, poll_every, finished):
    """The N - 1 decode steps behind the first token selection (N > 1) -> how many ran.  Token 2 runs eagerly (also the warm-up of
    every kernel form the step uses), the N - 2 replays of the captured step are tokens 3 .. N.  poll_every: every poll_every steps
    the finished flags are read, and the loop ends once every row has ended (a finished row only ever writes pad: the result is
    the same)."""
    one_step()
    steps_run = 1
    if N > 2:
        step = capture(one_step, dev, use_graph)
        if poll_every is None:
            for _ in range(N - 2):
                step()
            steps_run = N - 1
        else:
            poll = FinishedPoll(rows, dev)
            while steps_run < N - 1:
                n_now = min(int(poll_every), N - 1 - steps_run)
                for _ in range(n_now):
                    step()
                steps_run += n_now
                if bool((poll.read(finished) != 0).all()):
                    break
    return steps_run


def decode_args(mllm, tag, who, B, Lmax, decode_weights, cache, cur, pos, logits, flags):
    """tcavt_decode_args of a decode step at B rows on the cache `cache` = (k, v, Lmax) or (k_codes, k_scales, v_codes,
    v_scales, Lmax); scratch buffers come from the workspace under ``tag``; ``who`` names the caller in errors.
    On a shared prompt cache (tcavt_llama_decode_step_shared) `cache` = (k, v, rows) is the rows' suffix cache and Lmax still
    sizes the RoPE tables."""
    LW, ws, P = mllm.llama_wrapper, mllm._ws, mllm._prepared()
    ll, PL, dev = LW.shape, LW._prepared(), logits.device
    H, st = mllm.llama_hidden_size, LW.storage
    nqkv = (ll.n_q_heads + 2 * ll.n_kv_heads) * ll.head_dim
    cos, sin = LW._rope_tables(Lmax, dev)
    a = capi.DecodeArgs()
    # fragment-major weight copies for the step's weight streams and, on the 16-bit stream, fragment-major
    # activations between its kernels (16 or 32 whole rows per buffer); TCAVT_DECODE_ROWMAJOR=1 /
    # TCAVT_DECODE_ACT_ROWMAJOR=1: the row-major forms (A/B, tests)
    DW = LW.decode_weights(decode_weights) if (B <= 32 and os.environ.get("TCAVT_DECODE_ROWMAJOR", "0") != "1") else None
    if DW is None and decode_weights == "fp8":
        raise ValueError(f"{who}: decode_weights='fp8': this decoder shape has no skinny form "
                         "(hidden, inter and n_q_heads * head_dim must be multiples of 256, vocab of 16)")
    # (B <= 8: row-major activation rows are HALF the bytes of a 16-token fragment -- lanes of the empty token slots
    #  repeat the last row -- and the step is 0.89 vs 0.91 ms; B = 16: 0.98 vs 1.05, B = 32: 1.09 vs 1.21 ms)
    frag_act = DW is not None and LW.stream16 and os.environ.get("TCAVT_DECODE_ACT_ROWMAJOR", "0") != "1"
    # up to 8 samples: ONE block of 8 tokens (a k-step of activations = 512 consecutive bytes); blocks of 16 beyond
    # (TCAVT_DECODE_ACT_FRAG=16: blocks of 16 at any B, A/B)
    act_mode = 0 if not frag_act else (2 if B <= 8 and os.environ.get("TCAVT_DECODE_ACT_FRAG", "") != "16" else 1)
    Br = B if not frag_act else (8 if act_mode == 2 else 16 if B <= 16 else 32)
    bufs = dict(h16=ws.get(f"{tag}.dh16", (Br, H), st, dev, zero=True),
                part=ws.get(f"{tag}.dpart", (B, H // 16), torch.float32, dev),
                qkv=ws.get(f"{tag}.dqkv", (B, nqkv), st, dev),
                att=ws.get(f"{tag}.datt", (Br, ll.n_q_heads * ll.head_dim), st, dev, zero=True),
                act=ws.get(f"{tag}.dact", (Br, ll.inter), st, dev, zero=True), t=ws.get(f"{tag}.dt", (B, 64), st, dev, zero=True))
    if not LW.stream16:
        bufs["h"] = ws.get(f"{tag}.dh", (B, H), torch.float32, dev)
    capi.bind(a, **bufs)
    a.layers, a.gamma_final = PL.carr, PL.g_final.data_ptr()
    if DW is not None:
        a.layers, a.table_packed = DW.carr, DW.table.data_ptr()
        a.w_layout = capi.W_FRAG8 if decode_weights == "fp8" else capi.W_FRAG16
    a.act_layout = act_mode
    a.rope_cos, a.rope_sin, a.rope_L = cos.data_ptr(), sin.data_ptr(), Lmax
    a.table, a.txt_mod = PL.table.data_ptr(), P.txt.data_ptr()
    a.cur_tok, a.pos = cur.data_ptr(), pos.data_ptr()
    if len(cache) == 5:  # the four KV8 planes
        a.kv8_k_codes, a.kv8_k_scales, a.kv8_v_codes, a.kv8_v_scales = (t_.data_ptr() for t_ in cache[:4])
        a.kv_lmax = Lmax
    else:
        a.k_cache, a.v_cache, a.kv_lmax = cache[0].data_ptr(), cache[1].data_ptr(), cache[2]
    dx16 = ws.get(f"{tag}.dx16", (Br, H), st, dev, zero=True) if frag_act else ws.get(f"{tag}.x16", (B, H), st, dev)
    a.x16, a.logits, a.bad_id_flag = dx16.data_ptr(), logits.data_ptr(), flags.data_ptr()
    a.nonfinite_flag = flags[2:3].data_ptr()
    if LW.use_lora and LW.lora_r <= 8 and os.environ.get("TCAVT_DECODE_LORA_LAUNCH", "0") != "1":  # (A/B switch)
        a.lora_part, a.lora_rank = ws.get(f"{tag}.lpart", (B * H,), torch.float32, dev).data_ptr(), LW.lora_r
    # K split across workgroups (tcavt_gemm_args.splitk_ws): off by default -- measured 1.30 vs 1.22 ms per step
    # at B = 8 and 1.84 vs 1.87 at B = 32 (the hand-off costs what the split gains)
    if os.environ.get("TCAVT_DECODE_SPLITK", "0") == "1":
        skws = ws.get(f"{tag}.splitk", (9 << 20,), torch.uint8, dev, zero=True)  # tickets zeroed once, slabs behind
        a.splitk_ws, a.splitk_ws_bytes = skws.data_ptr(), skws.numel()
    a.n_layers, a.B, a.H, a.I, a.nq, a.nkv, a.V = ll.layers, B, H, ll.inter, ll.n_q_heads, ll.n_kv_heads, ll.vocab
    a.dtype16 = capi.F16 if st == torch.float16 else capi.BF16
    a.rms_eps, a.lora_scale = ll.rms_eps, (LW.lora_alpha / LW.lora_r) if LW.use_lora else 0.0
    a.stream_scale = float(LW.stream_scale)
    return a


# --------------------------------------------------------------------------------------
# generate_batch(prompt_lookup_num_tokens = k): prompt-lookup speculative decoding
# --------------------------------------------------------------------------------------
PROMPT_LOOKUP_MAX_TOKENS, PROMPT_LOOKUP_MAX_NGRAM, PROMPT_LOOKUP_MAX_ROWS, PROMPT_LOOKUP_POLL = 7, 8, 32, 4


def check_prompt_lookup(who, k, m, kv_cache, share_prefix, num_beams, return_logprobs, stop_sequences):
    """The arguments of a call with prompt_lookup_num_tokens = k set -> (k, m) as ints.  Nothing here touches a device."""
    for name, v, hi in (("prompt_lookup_num_tokens", k, PROMPT_LOOKUP_MAX_TOKENS), ("max_matching_ngram_size", m, PROMPT_LOOKUP_MAX_NGRAM)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 1 <= v <= hi:
            raise ValueError(f"{who}: {name} must be an int in [1, {hi}], got {v!r}")
    for name, bad, why in (("kv_cache='fp8'", kv_cache == "fp8", "the multi-position attention reads the 16-bit cache"),
                           ("share_prefix=True", share_prefix is True, "the multi-position attention has no shared-prefix form"),
                           ("num_beams > 1", num_beams != 1, "beam search has its own step"),
                           ("return_logprobs=True", return_logprobs is True, "the log-probability bracket is per single step"),
                           ("stop_sequences", bool(stop_sequences), "a stop sequence can end inside a block of drafts")):
        if bad:
            raise ValueError(f"{who}: prompt_lookup_num_tokens is not built for {name} ({why})")
    return int(k), int(m)


def prompt_lookup_step(mllm, who, k, m, Lmax, decode_weights, cache, st, selection, pad_token_id, flags):
    """-> (one_step, drafted, accepted).  one_step: tcavt_ngram_draft (every sequence's draft of up to k ids and the S * (k + 1)
    token / position rows) -> tcavt_llama_decode_step_multi (the logits of all k + 1 positions in one step) -> tcavt_spec_verify
    (select every position with the plain sampler on the state the plain loop has there, commit while it equals the draft; the
    call's ``selection`` gives the parameters, the output and the ending rules -- the checks have refused what else it could hold).
    The device arrays are fixed for the call, so the captured step stays valid.  Buffers under ``gen.pl.*``."""
    sp, out, drules = selection.sp, selection.out, selection.drules
    ws, LW, dev = mllm._ws, mllm.llama_wrapper, out.device
    S, T = out.shape[0], k + 1
    R = S * T
    n_draft, cur_rows, pos_rows = ws.get("gen.pl.n_draft", (S,), I32, dev), ws.get("gen.pl.cur", (R,), I64, dev), ws.get("gen.pl.pos", (R,), I32, dev)
    scratch = ws.get("gen.pl.slot", (R + S,), I32, dev, zero=True)
    drafted, accepted = torch.zeros(S, dtype=I32, device=dev), torch.zeros(S, dtype=I32, device=dev)
    logits = ws.get("gen.pl.logits", (R, LW.shape.vocab), torch.float32, dev)
    sws = sample_workspace(ws, "gen.pl.sample_ws", R, dev)
    a = decode_args(mllm, "gen.pl", who, R, Lmax, decode_weights, cache, cur_rows, pos_rows, logits, flags)
    v = ops.spec_verify_args(logits, T, n_draft, cur_rows, scratch, drafted, accepted, st.history, st.hist_len, sp, st.step, st.max_new,
                             st.out_row, st.cur, st.pos, st.finished, out, advance_pos=True, workspace=sws, stop=drules)

    def one_step():
        ops.ngram_draft(st.history, st.hist_len, st.cur, st.pos, st.finished, k, m, pad_token_id, n_draft, cur_rows, pos_rows)
        ops.llama_decode_step_multi(a, T)
        ops.spec_verify(v)

    return one_step, drafted, accepted


# what the entries share between their own refusals and the first launch (each entry calls them at its own, fixed point)
def the_nine(kw):
    """The keywords an entry does not name are the nine per-request arguments, all of them -> in PER_REQUEST_ARGS' order."""
    assert sorted(kw) == sorted(PER_REQUEST_ARGS), sorted(kw)
    return {k: kw[k] for k in PER_REQUEST_ARGS}


def check_poll_every(who, poll_every):
    if poll_every is not None and int(poll_every) < 1:
        raise ValueError(f"{who}: poll_every must be None or >= 1, got {poll_every}")


def prompt_tokens(mllm, context_str_list, input_ids, attention_mask, max_new_tokens):
    """The prompt of generate_batch -> (input_ids, attention_mask, B, Lt, N): the ids as given, or the tokenizer's as the
    reference makes them; N = max_new_tokens, checked.  Nothing here touches a device."""
    if input_ids is None:
        if mllm.tokenizer is None or context_str_list is None:
            raise NotImplementedError(
                "generate_batch needs input_ids / attention_mask: no tokenizer can be fetched offline (train.py:500,590-598)")
        enc = mllm.tokenizer(["<image> " + c for c in context_str_list], padding=True, truncation=True, max_length=256,
                             return_tensors="pt")
        input_ids, attention_mask = enc["input_ids"], enc["attention_mask"]
    B, Lt = input_ids.shape
    N = int(max_new_tokens)
    if N < 1:
        raise ValueError("max_new_tokens must be >= 1")
    return input_ids, attention_mask, B, Lt, N


def begin(mllm, dev, input_ids, attention_mask):
    """Every entry passes here once it has refused what it refuses: the error flags of the last call's request table and
    constraint are dropped (mllm.check_flags), and the prompt goes to the device -> (input_ids, the mask as int64; None: ones)."""
    mllm._request_flag = mllm._constraint_flag = None
    input_ids = input_ids.to(dev).contiguous()
    mask = attention_mask if attention_mask is not None else torch.ones_like(input_ids)
    return input_ids, mask.to(dev).to(I64).contiguous()


def fanout_state(rows, hist_cap, step_words, dev):
    """The state of ``rows`` decode rows that a fan-out launch fills: hist_len and pos are left to it."""
    return slot_state(torch.zeros(rows, hist_cap, dtype=I64, device=dev), torch.empty(rows, dtype=I32, device=dev),
                      torch.zeros(step_words, dtype=I32, device=dev), torch.zeros(rows, dtype=I64, device=dev),
                      torch.empty(rows, dtype=I32, device=dev), torch.zeros(rows, dtype=I32, device=dev))


def shared_prefix_state(mllm, pf, logits_src, input_ids, n, N, step_words):
    """n decode rows per prompt on the shared prompt cache (share_prefix=True, beam search) -> (st, logits, cache, prefix).  The
    prompts' cache stays where the prefill ``pf`` wrote it (``prefix``: what tcavt_llama_decode_step_shared reads in place);
    the rows own the suffix cache ``gen.sfx.*`` of the N - 1 tokens a row can append (``cache``, its row count last), and one
    tcavt_state_fanout makes their state -- ``step_words`` step words -- and first logits ``gen.logits`` of ``logits_src``."""
    LW, ws, dev = mllm.llama_wrapper, mllm._ws, input_ids.device
    Nq, (B, Lt), kv_len = mllm.qformer.num_query_tokens, input_ids.shape, pf.buf("kvlen")
    sfx_rows = max(N - 1, 1)
    cache = cache_buffers(ws, "gen.sfx", LW, "fp16", B * n, sfx_rows, dev) + (sfx_rows,)
    pk, pv = pf.buf("cache")
    prefix = capi.KvPrefix(pk.data_ptr(), pv.data_ptr(), kv_len.data_ptr(), n, Nq + Lt)
    st = fanout_state(B * n, Lt + N, step_words, dev)
    logits = ws.get("gen.logits", (B * n, LW.shape.vocab), torch.float32, dev)
    ops.state_fanout(n, input_ids, kv_len, Nq, logits_src, logits, st.history, st.hist_len, st.pos, st.finished)
    return st, logits, cache, prefix


# --------------------------------------------------------------------------------------
# LlamaMultiModal.generate_batch
# --------------------------------------------------------------------------------------
def generate_batch(mllm, vision_embs_batch, *, context_str_list, max_new_tokens, input_ids, attention_mask, pad_token_id, use_graph,
                   decode_weights, kv_cache, stop_token_ids, stop_sequences, return_info, poll_every, num_return_sequences,
                   share_prefix, return_logprobs, num_beams, length_penalty, early_stopping, prompt_lookup_num_tokens,
                   max_matching_ngram_size, constraint, constraint_start, top_logprobs, **nine):
    """-> (out int64 [B * num_return_sequences, max_new_tokens] on the device, info or None).  With n = num_return_sequences > 1
    the prompts are prefilled once, at B rows (``gen.src.*``), one tcavt_kv_fanout makes the state of B * n decode rows of it, and
    everything from the first token selection on runs at B * n rows; n = 1 is launch for launch the call without the argument.
    share_prefix (any n >= 1): the prompts' cache ``gen.src.*`` stays where the prefill wrote it and is read in place by every
    decode step (tcavt_attn_decode_shared); one tcavt_state_fanout makes the rows' state and first logits, and the decode rows
    own a suffix cache ``gen.sfx.*`` of their generated tokens alone.  num_beams > 1: beam_search below.
    prompt_lookup_num_tokens = k: the cache has k more rows, the state is the per-slot form (step [S], max_new = N, out_row[s] = s:
    the same Philox rows and the same tokens as the batch form) and a step is prompt_lookup_step above; None is the call without."""
    who = "generate_batch"
    k = m = None
    n_top = check_top_logprobs(who, top_logprobs, return_logprobs)  # (before anything touches a device; beams and prompt lookup
    #                                                                   refuse return_logprobs=True below, and with it this)
    nine = the_nine(nine)
    if constraint is not None or constraint_start is not None:  # (before anything touches a device, and before the beam search)
        check_constraint(who, mllm, constraint, constraint_start, num_beams, prompt_lookup_num_tokens, nine["no_repeat_ngram_size"],
                         nine["min_new_tokens"])
    listed = per_request_names(**nine)
    if listed and (num_beams != 1 or prompt_lookup_num_tokens is not None):  # (beam search and tcavt_spec_verify keep the one struct)
        raise ValueError(f"{who}: per-request values ({', '.join(listed)}) are not built for "
                         f"{'num_beams > 1' if num_beams != 1 else 'prompt_lookup_num_tokens'}: one value per call there")
    if prompt_lookup_num_tokens is not None:  # (before anything touches a device, and before the beam search takes over)
        k, m = check_prompt_lookup(who, prompt_lookup_num_tokens, max_matching_ngram_size, kv_cache, share_prefix, num_beams,
                                   return_logprobs, stop_sequences)
    if isinstance(num_beams, bool) or not isinstance(num_beams, numbers.Integral) or not 1 <= num_beams <= ops.BEAMS_MAX:
        raise ValueError(f"generate_batch: num_beams must be an int in [1, {ops.BEAMS_MAX}], got {num_beams!r}")
    if num_beams > 1:
        return beam_search(mllm, vision_embs_batch, int(num_beams), nine, context_str_list=context_str_list,
                           max_new_tokens=max_new_tokens, input_ids=input_ids, attention_mask=attention_mask, pad_token_id=pad_token_id,
                           use_graph=use_graph, decode_weights=decode_weights, kv_cache=kv_cache, stop_token_ids=stop_token_ids,
                           stop_sequences=stop_sequences, return_info=return_info, poll_every=poll_every,
                           num_return_sequences=num_return_sequences, return_logprobs=return_logprobs, length_penalty=length_penalty,
                           early_stopping=early_stopping)
    check_format(who, "kv_cache", kv_cache)  # (before anything touches a device)
    check_bool(who, "return_logprobs", return_logprobs)
    check_bool(who, "share_prefix", share_prefix)
    if share_prefix and kv_cache == "fp8":
        raise ValueError("generate_batch: share_prefix=True reads the 16-bit prompt cache in place; kv_cache='fp8' has no shared form")
    rules = stop_rules(who, mllm, stop_token_ids, stop_sequences, nine["min_new_tokens"], nine["eos_token_id"])
    check_poll_every(who, poll_every)
    n = num_return_sequences
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1:
        raise ValueError(f"generate_batch: num_return_sequences must be an int >= 1, got {num_return_sequences!r}")
    n = int(n)
    input_ids, attention_mask, B, Lt, N = prompt_tokens(mllm, context_str_list, input_ids, attention_mask, max_new_tokens)
    check_format(who, "decode_weights", decode_weights)
    src_B, B = B, B * n  # the prefill's rows; from here on B counts decode rows (n continuations per prompt, prompt-major)
    check_fp8_weights(who, decode_weights, B, "B" if n == 1 else "B * num_return_sequences")
    if k is not None:
        if B * (k + 1) > PROMPT_LOOKUP_MAX_ROWS:
            raise ValueError(f"{who}: prompt_lookup_num_tokens = {k} needs sequences * (k + 1) <= {PROMPT_LOOKUP_MAX_ROWS} decode rows, "
                             f"got {B} * {k + 1}")
        if not 0 <= int(pad_token_id) < mllm.llama_wrapper.shape.vocab:  # (the rows behind a draft feed the pad token to the step)
            raise ValueError(f"{who}: prompt_lookup_num_tokens needs pad_token_id inside [0, vocab), got {pad_token_id}")
    sp, table = request_params(who, src_B, n, rules, pad_token_id, **nine)  # (host only; a table: one entry per decode row)
    starts = constraint.starts(who, constraint_start, src_B, n) if constraint is not None else None  # (host only, likewise)
    dev = vision_embs_batch.device
    input_ids, mask64 = begin(mllm, dev, input_ids, attention_mask)
    Nq = mllm.qformer.num_query_tokens
    Lmax = Nq + Lt + N + (k or 0)  # (a verify step writes k rows beyond the last position a row can reach)
    # n > 1: the prompts alone, into a cache of the prompt's own 16 + Lt rows (the width of the pool's one-sample prefill)
    own_cache = n == 1 and not share_prefix  # the prefill writes straight into the decode rows' cache
    pf = Prefill(mllm, "gen", B, Lt, Lmax, kv_cache, dev) if own_cache else Prefill(mllm, "gen.src", src_B, Lt, Nq + Lt, kv_cache, dev)
    with eval_arithmetic(mllm):
        # ---- prefill: image tokens + prompt through the decoder, keys / values of every layer into the cache
        logits = pf.run(vision_embs_batch, input_ids, mask64)
        # ---- device-resident generation state
        prefix = None
        if own_cache:
            cache, kv_len = pf.buf("cache") + (Lmax,), pf.buf("kvlen")
            history = torch.zeros(B, Lt + N, dtype=I64, device=dev)
            history[:, :Lt] = input_ids
            st = slot_state(history, (kv_len - Nq).to(I32), torch.zeros(1, dtype=I32, device=dev),
                            torch.zeros(B, dtype=I64, device=dev), kv_len.clone(), torch.zeros(B, dtype=I32, device=dev))
        elif share_prefix:  # the state and the first logits alone: the prompts' cache is read where it is
            st, logits, cache, prefix = shared_prefix_state(mllm, pf, logits, input_ids, n, N, 1)
        else:
            # one launch: every prompt's cache rows, first logits, history, hist_len, pos and finished to its n decode rows
            LW = mllm.llama_wrapper
            cache = cache_buffers(mllm._ws, "gen", LW, kv_cache, B, Lmax, dev) + (Lmax,)
            st = fanout_state(B, Lt + N, 1, dev)
            logits_src, logits = logits, mllm._ws.get("gen.logits", (B, LW.shape.vocab), torch.float32, dev)
            ops.kv_fanout(pf.buf("cache"), cache[:-1], n, Nq + Lt, Nq + Lt, Lmax, LW.shape.layers, LW.shape.n_kv_heads, input_ids,
                          pf.buf("kvlen"), Nq, logits_src, logits, st.history, st.hist_len, st.pos, st.finished)
        if k is not None:  # the per-slot form of the same state: every row has its own step word and the budget N
            st.step, st.max_new = torch.zeros(B, dtype=I32, device=dev), torch.full((B,), N, dtype=I32, device=dev)
            st.out_row = torch.arange(B, dtype=I64, device=dev)
        out = torch.full((B, N), int(pad_token_id), dtype=I64, device=dev)
        sws = sample_workspace(mllm._ws, "gen.sample_ws", B, dev)
        selection = Selection(mllm, sp, table, rules, return_info, return_logprobs, n_top, constraint, starts, out, st)
        selection(logits, st, False, "gen", sws)
        steps_run = 0
        drafted = accepted = None
        if N > 1 and k is not None:
            one_step, drafted, accepted = prompt_lookup_step(mllm, who, k, m, Lmax, decode_weights, cache, st, selection,
                                                             int(pad_token_id), pf.flags)
            steps_run = decode_loop(one_step, N, B, dev, use_graph, PROMPT_LOOKUP_POLL if poll_every is None else poll_every,
                                    st.finished)
        elif N > 1:
            a = decode_args(mllm, "gen", who, B, Lmax, decode_weights, cache, st.cur, st.pos, logits, pf.flags)

            def one_step():
                if prefix is None:
                    ops.llama_decode_step(a)
                else:
                    ops.llama_decode_step_shared(a, prefix)
                selection(logits, st, True, "gen", sws)

            steps_run = decode_loop(one_step, N, B, dev, use_graph, poll_every, st.finished)
        info = None
        if return_info or return_logprobs:
            info = dict(selection.host(finish=return_info), steps=steps_run)
        if return_info:
            ran_out = info["finish_reason"] == 0  # (no device budget in this form: a row that never ended ran out at max_new_tokens)
            info["finish_reason"][ran_out], info["n_generated"][ran_out] = BUDGET, N
            if k is not None:
                zero = torch.zeros(B, dtype=I32)
                info.update(drafted=zero if drafted is None else drafted.cpu(), accepted=zero.clone() if accepted is None else accepted.cpu())
    return out, info


# --------------------------------------------------------------------------------------
# LlamaMultiModal.generate_batch(num_beams = n > 1)
# --------------------------------------------------------------------------------------
def beam_search(mllm, vision_embs_batch, n, nine, *, context_str_list, max_new_tokens, input_ids, attention_mask, pad_token_id, use_graph,
                decode_weights, kv_cache, stop_token_ids, stop_sequences, return_info, poll_every, num_return_sequences, return_logprobs,
                length_penalty, early_stopping):
    """Beam search with n beams per prompt on the shared prompt cache -> (out int64 [B * r, max_new_tokens] on the device, info or
    None), r = num_return_sequences <= n.  The prompts are prefilled at B rows (``gen.src.*``), tcavt_state_fanout makes the state
    and first logits of the R = B * n beam rows, which own the suffix cache ``gen.sfx.*``; the first selection runs on the
    prefill's logits, then one step is tcavt_llama_decode_step_shared -> tcavt_beam_select -> tcavt_beam_reorder.  Scores, beams,
    the finished store and the done flags live on the device (include/tcavt.h states the semantics); the result is copied out
    of the finished store at the end.  ``nine``: the call's nine sampling arguments, every one a single value; the search reads
    do_sample, repetition_penalty, no_repeat_ngram_size, eos_token_id and (to refuse it) min_new_tokens."""
    who = "generate_batch"
    eos_token_id, min_new_tokens = nine["eos_token_id"], nine["min_new_tokens"]
    # ---- every illegal value is refused before anything touches a device
    check_format(who, "kv_cache", kv_cache)
    check_format(who, "decode_weights", decode_weights)
    if nine["do_sample"]:
        raise ValueError("generate_batch: num_beams > 1 needs do_sample=False (beam sampling is not built)")
    if kv_cache == "fp8":
        raise ValueError("generate_batch: num_beams > 1 reads the 16-bit prompt cache in place; kv_cache='fp8' has no beam form")
    for name, value, unset in (("stop_token_ids", stop_token_ids, not stop_token_ids), ("stop_sequences", stop_sequences, not stop_sequences),
                               ("min_new_tokens", min_new_tokens, min_new_tokens in (0, None))):
        if not unset:
            raise ValueError(f"generate_batch: {name} is not built for num_beams > 1 (got {value!r})")
    if return_logprobs is not False:
        raise ValueError(f"generate_batch: return_logprobs is not built for num_beams > 1 (got {return_logprobs!r})")
    if not isinstance(early_stopping, bool):
        raise ValueError(f"generate_batch: early_stopping must be False or True (HF's 'never' is not built), got {early_stopping!r}")
    if isinstance(length_penalty, bool) or not isinstance(length_penalty, numbers.Real) or not math.isfinite(length_penalty):
        raise ValueError(f"generate_batch: length_penalty must be a finite number, got {length_penalty!r}")
    V = mllm.llama_wrapper.shape.vocab
    if V < 2 * n:
        raise ValueError(f"generate_batch: num_beams = {n} needs a vocabulary of at least 2 * num_beams ids, got {V}")
    r = num_return_sequences
    if isinstance(r, bool) or not isinstance(r, numbers.Integral) or not 1 <= r <= n:
        raise ValueError(f"generate_batch: num_return_sequences must be an int in [1, num_beams = {n}], got {num_return_sequences!r}")
    r = int(r)
    check_poll_every(who, poll_every)
    input_ids, attention_mask, B, Lt, N = prompt_tokens(mllm, context_str_list, input_ids, attention_mask, max_new_tokens)
    R, K = B * n, 2 * n
    check_fp8_weights(who, decode_weights, R, "B * num_beams")
    dev = vision_embs_batch.device
    input_ids, mask64 = begin(mllm, dev, input_ids, attention_mask)
    LW, ws = mllm.llama_wrapper, mllm._ws
    Nq = mllm.qformer.num_query_tokens
    Lmax = Nq + Lt + N
    pf = Prefill(mllm, "gen.src", B, Lt, Nq + Lt, "fp16", dev)
    with eval_arithmetic(mllm):
        logits_src = pf.run(vision_embs_batch, input_ids, mask64)
        # ---- device-resident state: the rows' (one step word per prompt), the prompts' and the finished store
        st, logits, sfx, prefix = shared_prefix_state(mllm, pf, logits_src, input_ids, n, N, B)
        kv_len = pf.buf("kvlen")
        z32 = lambda *shape: torch.zeros(*shape, dtype=I32, device=dev)  # noqa: E731
        run_score = torch.zeros(R, dtype=torch.float32, device=dev)
        live = z32(B, n)
        live[:, 0] = 1
        fin_tokens = torch.full((B, n, N), int(pad_token_id), dtype=I64, device=dev)
        fin_score, fin_flag, fin_len = torch.zeros(B, n, dtype=torch.float32, device=dev), z32(B, n), z32(B, n)
        unsat, done, parent, plan = torch.ones(B, dtype=I32, device=dev), z32(B), z32(R), z32(B, 4)
        len_pow = torch.tensor([float(s + 1) ** float(length_penalty) for s in range(N)], dtype=torch.float64).to(torch.float32).to(dev)
        trace = torch.full((N, B, K, 3), -1, dtype=I32, device=dev) if return_info else None
        bws = ws.get("gen.beam_ws", (ops.beam_workspace_bytes(R),), torch.uint8, dev)
        sel = ops.beam_args(logits, n, N, st.history, st.hist_len, run_score, live, fin_tokens, fin_score, fin_flag, fin_len, unsat, done,
                            st.cur, st.pos, st.finished, st.step, kv_len, len_pow, parent, plan, bws, eos_token_id, pad_token_id,
                            nine["repetition_penalty"], nine["no_repeat_ngram_size"], early_stopping, trace=trace)
        reo = ops.beam_reorder_args(n, parent, plan, st.cur, st.history, st.hist_len, st.pos, st.step, sfx[0], sfx[1], LW.shape.layers,
                                    LW.shape.n_kv_heads)
        ops.beam_select(sel)  # the first selection: from the prefill's logits
        ops.beam_reorder(reo)
        steps_run = 0
        if N > 1:
            a = decode_args(mllm, "gen", who, R, Lmax, decode_weights, sfx, st.cur, st.pos, logits, pf.flags)

            def one_step():
                ops.llama_decode_step_shared(a, prefix)
                ops.beam_select(sel)
                ops.beam_reorder(reo)

            steps_run = decode_loop(one_step, N, R, dev, use_graph, poll_every, st.finished)
        out = fin_tokens[:, :r].reshape(B * r, N).contiguous()
        info = None
        if return_info:
            n_gen = fin_len[:, :r].reshape(-1).cpu()
            last = out.cpu().gather(1, (n_gen.to(I64) - 1).clamp(min=0)[:, None])[:, 0]
            is_eos = (last == int(eos_token_id)) if eos_token_id is not None else torch.zeros_like(last, dtype=torch.bool)
            reason = torch.where(is_eos, 1, BUDGET).to(I32)
            t = trace[:steps_run + 1].cpu()
            info = dict(sequences_scores=fin_score[:, :r].reshape(-1).cpu(), n_generated=n_gen, finish_reason=reason, steps=steps_run,
                        beam_trace=dict(parent=t[..., 0].contiguous(), token=t[..., 1].contiguous(),
                                        acc=t[..., 2].contiguous().view(torch.float32)))
    return out, info


# --------------------------------------------------------------------------------------
# LlamaMultiModal.generate_pool
# --------------------------------------------------------------------------------------
def generate_pool(mllm, vision_embs, *, input_ids, attention_mask, max_new_tokens, slots, poll_every, pad_token_id, use_graph,
                  decode_weights, kv_cache, admit_group, stop_token_ids, stop_sequences, return_info, return_logprobs, constraint,
                  constraint_start, top_logprobs, **nine):
    """-> (out int64 [R, max budget] on the device, mllm.pool_stats)."""
    who = "generate_pool"
    nine = the_nine(nine)
    n_top = check_top_logprobs(who, top_logprobs, return_logprobs)
    # ---- every illegal value is refused before anything touches a device
    check_format(who, "kv_cache", kv_cache)
    check_format(who, "decode_weights", decode_weights)
    check_bool(who, "return_logprobs", return_logprobs)
    if constraint is not None or constraint_start is not None:
        check_constraint(who, mllm, constraint, constraint_start, 1, None, nine["no_repeat_ngram_size"], nine["min_new_tokens"])
    rules = stop_rules(who, mllm, stop_token_ids, stop_sequences, nine["min_new_tokens"], nine["eos_token_id"])
    S, poll_every = int(slots), int(poll_every)
    if S < 1:
        raise ValueError(f"generate_pool: slots must be >= 1, got {slots}")
    if poll_every < 1:
        raise ValueError(f"generate_pool: poll_every must be >= 1, got {poll_every}")
    G = int(admit_group)
    if not 1 <= G <= S:
        raise ValueError(f"generate_pool: admit_group must be in [1, slots = {S}], got {admit_group}")
    if input_ids.dim() != 2 or attention_mask.shape != input_ids.shape or vision_embs.shape[0] != input_ids.shape[0]:
        raise ValueError("generate_pool: vision_embs [R, ...], input_ids [R, Lt] and attention_mask [R, Lt] must agree")
    R, Lt = input_ids.shape
    scalar = not hasattr(max_new_tokens, "__len__")
    budgets = [int(max_new_tokens)] * R if scalar else [int(n) for n in max_new_tokens]
    if len(budgets) != R:
        raise ValueError(f"generate_pool: max_new_tokens has {len(budgets)} budgets for {R} requests")
    if (scalar and int(max_new_tokens) < 1) or any(n < 1 for n in budgets):
        raise ValueError("generate_pool: every budget in max_new_tokens must be >= 1")
    Nmax = int(max_new_tokens) if scalar else max(budgets, default=0)
    LW, ws = mllm.llama_wrapper, mllm._ws
    ll = LW.shape
    if not 0 <= int(pad_token_id) < ll.vocab:  # (idle and finished slots feed the pad token to the decode step)
        raise ValueError(f"generate_pool: pad_token_id = {pad_token_id} outside [0, vocab = {ll.vocab})")
    check_fp8_weights(who, decode_weights, S, "slots")
    sp, table = request_params(who, R, 1, rules, pad_token_id, **nine)  # (host only)
    starts = constraint.starts(who, constraint_start, R, 1) if constraint is not None else None  # (host only, likewise)
    dev = vision_embs.device
    input_ids, mask64 = begin(mllm, dev, input_ids, attention_mask)
    out = torch.full((R, Nmax), int(pad_token_id), dtype=I64, device=dev)
    stats = mllm.pool_stats = dict(steps=0, admitted=[], retired=[], groups=[])
    mllm._pool_flag = None  # (the grouped admission's bad-slot flag: check_flags)
    records = (mllm, sp, table, rules, return_info, return_logprobs, n_top, constraint, starts, out)
    if R == 0:  # the records of no request: no launch, no workspace buffer
        stats.update(Selection(*records, st=None).host())
        return out, stats
    Nq = mllm.qformer.num_query_tokens
    L = Nq + Lt
    Lmax = L + Nmax  # 16 + Lt + max budget
    pf = Prefill(mllm, "pool.pf", 1, Lt, L, kv_cache, dev)  # a request on its own, into a one-sample cache
    with eval_arithmetic(mllm):
        flags = mllm._last_flags = ws.get("mm.flags", (3,), I32, dev, zero=True)
        # ---- the pool: S-slot cache and per-slot state
        cache = cache_buffers(ws, "pool", LW, kv_cache, S, Lmax, dev, zero=True)
        pf.reserve("cache")
        for t_ in cache:
            t_.select(-2, 0).zero_()
        # idle state: zeroed cache row 0, pos = 0, finished = 1, cur_tok = pad
        st = slot_state(history=ws.get("pool.history", (S, Lt + Nmax), I64, dev, zero=True),
                        hist_len=ws.get("pool.hist_len", (S,), I32, dev).zero_(),
                        step=ws.get("pool.step", (S,), I32, dev).zero_(),
                        max_new=ws.get("pool.max_new", (S,), I32, dev).fill_(1),
                        out_row=ws.get("pool.out_row", (S,), I64, dev).zero_(),
                        pos=ws.get("pool.pos", (S,), I32, dev).zero_(),
                        finished=ws.get("pool.finished", (S,), I32, dev).fill_(1),
                        cur=ws.get("pool.cur", (S,), I64, dev).fill_(int(pad_token_id)))
        logits = ws.get("pool.logits", (S, ll.vocab), torch.float32, dev)
        pf.reserve("logits", "kvlen", "final16", "x16", "h")
        poll = FinishedPoll(S, dev)
        sws, sws1 = sample_workspace(ws, "pool.sample_ws", S, dev), sample_workspace(ws, "pool.pf.sample_ws", 1, dev)
        a = decode_args(mllm, "pool", who, S, Lmax, decode_weights, cache + (Lmax,), st.cur, st.pos, logits, flags)
        selection = Selection(*records, st=st)
        # what both admission launches share: rows, src_lmax, kv_lmax, n_layers, S, nkv ... and the eight state arrays
        geometry = (L, L, Lmax, ll.layers, S, ll.n_kv_heads)
        state = (st.history, st.hist_len, st.step, st.max_new, st.out_row, st.pos, st.finished, st.cur)

        def one_step():
            ops.llama_decode_step(a)
            selection(logits, st, True, "pool", sws)

        def admit(s, r):
            # the request on its own: the ordinary decoder pass at B = 1 into the one-sample cache, the copy into slot s,
            # and the first token from the one-row logits with the slot's state (views that start at slot s)
            logits1 = pf.run(vision_embs[r:r + 1], input_ids[r:r + 1], mask64[r:r + 1], after_stack=lambda: ops.slot_admit(
                pf.buf("cache"), cache, s, *geometry, input_ids[r], pf.buf("kvlen"), Nq, budgets[r], r, *state))
            selection(logits1, slot_view(st, s), False, "pool.pf", sws1)

        if G > 1:
            # ---- grouped admission: ONE decoder pass at exactly B = G rows per group (pool.pg.*); a short group is filled
            # with pad rows (its first request again, slot -1), so M = G * L and with it every kernel form is constant
            pg = Prefill(mllm, "pool.pg", G, Lt, L, kv_cache, dev)
            pg_vis = ws.get("pool.pg.vis", (G,) + tuple(vision_embs.shape[1:]), vision_embs.dtype, dev)
            pg_ids = ws.get("pool.pg.ids", (G, Lt), I64, dev)
            pg_mask = ws.get("pool.pg.mask", (G, Lt), I64, dev)
            pg_slot = ws.get("pool.pg.slot", (G,), I32, dev)
            pg_budget = ws.get("pool.pg.budget", (G,), I32, dev)
            pg_outrow = ws.get("pool.pg.outrow", (G,), I64, dev)
            pg.reserve("cache", "logits", "kvlen", "final16", "x16", "h")
            pg_sws = sample_workspace(ws, "pool.pg.sample_ws", G, dev)
            bad_slot = mllm._pool_flag = ws.get("pool.pg.bad_slot", (1,), I32, dev, zero=True)
            vis_all = vision_embs.contiguous()
            budgets_dev = torch.tensor(budgets, dtype=I32, device=dev)

            def stage(group):
                # the group's rows of the request list -> the staging buffers (device-side gathers; two small uploads)
                reqs = [r for _, r in group] + [group[0][1]] * (G - len(group))
                idx = torch.tensor(reqs, dtype=I64, device=dev)
                torch.index_select(vis_all, 0, idx, out=pg_vis)
                torch.index_select(input_ids, 0, idx, out=pg_ids)
                torch.index_select(mask64, 0, idx, out=pg_mask)
                torch.index_select(budgets_dev, 0, idx, out=pg_budget)
                pg_outrow.copy_(idx)
                pg_slot.copy_(torch.tensor([s for s, _ in group] + [-1] * (G - len(group)), dtype=I32, device=dev))

            def group_pass():
                logits_g = pg.run(pg_vis, pg_ids, pg_mask, after_stack=lambda: ops.slot_admit_group(
                    pg.buf("cache"), cache, pg_slot, *geometry, pg_ids, pg.buf("kvlen"), Nq, pg_budget, pg_outrow, bad_slot, *state))
                selection(logits_g, st, False, "pool.pg", pg_sws, slot_of_row=pg_slot)

        sched = SlotScheduler(R, S, G)
        step = later_pass = None
        while True:
            for group in (sched.admission_groups() if G > 1 else ()):
                stage(group)
                if not stats["groups"]:
                    group_pass()  # the first pass runs eagerly: the warm-up of the workspaces and of every kernel form
                else:
                    if later_pass is None:  # captured once, before the second pass; only the staging buffers change
                        later_pass = capture(group_pass, dev, use_graph)
                    later_pass()
                stats["groups"].append((tuple(r for _, r in group), tuple(s for s, _ in group), stats["steps"]))
                stats["admitted"] += [(r, s, stats["steps"]) for s, r in group]
            for s, r in (sched.admissions() if G == 1 else ()):
                admit(s, r)
                stats["admitted"].append((r, s, stats["steps"]))
            if not sched.busy():
                break
            if step is None:
                # the first step runs eagerly and unpolled, as in generate_batch: it is the warm-up of every kernel form
                # the step uses; then the capture
                one_step()
                stats["steps"] = 1
                step = capture(one_step, dev, use_graph)
            for _ in range(poll_every):
                step()
            stats["steps"] += poll_every
            n_ret = len(sched.retired)
            sched.retire(poll.read(st.finished).tolist())
            stats["retired"] += [(r, s, stats["steps"]) for r, s in sched.retired[n_ret:]]
        stats.update(selection.host())
    return out, stats
