"""loss.backward() on MultiModalTrajectoryModel: the reference's own training loop (scripts/train.py:1127-1183 --
DistributedDataParallel wrap, frozen MLLM, torch.optim.AdamW, zero_grad / forward / loss.backward() / step) on the
hand-written backward of backward.py, through one torch.autograd.Function.

Activation.  MultiModalTrajectoryModel.forward routes through the bridge only when trainable_set() names a supported set:
grad mode is on, no training.Trainer drives the model, some parameter outside `mllm` requires grad, and inside `mllm`
either nothing does (S0, train.py:1141-1142) or exactly the LoRA adapters of q_proj / v_proj do (S1, Trainer's
lora_trainable=True set).  Every other state -- the default one, where every parameter requires grad, included -- runs the
forward as before, with plain outputs.

The Function's inputs are forward's batch arguments and the parameters that require grad; its outputs are (loss, decoded),
or decoded alone without y / norm_stat.  Gradients go to the parameters only: a backward through a batch tensor that requires
grad raises.
Forward and backward launch only this project's kernels, under the model flags and with the backward schedule that
training.Trainer uses (training.backward_flags / make_backward / run_backward); the flags are set around the two calls and
restored after them.

Staleness.  (1) Packed weight copies: once a model has been on the bridge, each of its forwards (no_grad ones included, so
that a validation pass after a torch.optim step sees the new weights) compares every trainable parameter's (data_ptr,
_version) with the values seen when its module's copies were last built and rebuilds the stale ones -- a torch.optim step, a
DDP broadcast or an in-place edit is picked up.  Models never put on the bridge keep their forward's host cost.
(2) Tapes: they live in the model's workspaces, which any later forward overwrites; a backward after another forward of the
model raises, before it writes a gradient, and so does a second backward over one graph or a backward after a trainable
parameter changed in place.

Gradient hand-off.  The stages write into one flat fp32 vector (backward.GradBook, not bound to the parameters); backward
returns a view of it per trainable parameter, which AccumulateGrad may keep as p.grad.  Every backward writes into a newly
allocated vector: the views of an earlier one may be held anywhere (p.grad, torch.autograd.grad's result, a tensor hook), and
none of them ever changes afterwards."""
import torch

from .backward import GradBook
from .llm_backward import lora_named_parameters
from .training import backward_flags, make_backward, run_backward, trainable_named_parameters

S0, S1 = "S0", "S1"  # train.py's set; that set plus the LoRA adapters (modify_train.py's LoRA-only subset)


def trainable_set(model):
    """S0, S1 or None (inactive) for the model's current requires-grad state (see the module docstring)."""
    if not torch.is_grad_enabled() or model.driven_by_trainer or model._llm_cache is not None:
        return None
    lora = _lora_ids(model)
    n_lora = 0
    for p in model.mllm.parameters():
        if p.requires_grad:
            if id(p) not in lora:
                return None  # a Llama / Q-Former / projection weight trains: out of scope
            n_lora += 1
    if not any(p.requires_grad for p in model.lane_polygon_encoder.parameters()) and \
            not any(p.requires_grad for p in model.ltsf.parameters()):
        return None
    if n_lora == 0:
        return S0
    return S1 if n_lora == len(lora) else None


def _lora_ids(model):
    if not model.mllm.llama_wrapper.use_lora:
        return frozenset()
    ids = getattr(model, "_lora_id_cache", None)
    if ids is None:
        ids = model._lora_id_cache = frozenset(id(p) for _, p in lora_named_parameters(model))
    return ids


class _Bridge:
    """Per-model state of one trainable set: the gradient book and backward stages, and the parameter keys that the
    packed copies were built from."""

    def __init__(self, model, kind):
        self.model, self.kind = model, kind
        named = trainable_named_parameters(model)
        groups = [(model.ltsf, [p for n, p in named if n.startswith("ltsf.")]),
                  (model.lane_polygon_encoder, [p for n, p in named if n.startswith("lane_polygon_encoder.")])]
        if kind == S1:
            lora = lora_named_parameters(model)
            named = named + lora
            groups.append((model.mllm.llama_wrapper, [p for _, p in lora]))
        self.named, self.groups = named, groups
        self.book = GradBook(named, next(model.parameters()).device, bind=False)
        self.bw, self.lbw, self.qbw = make_backward(model, self.book, kind == S1)
        self.flags = backward_flags(model, kind == S1)
        self.keys = {}

    def refresh(self):
        """Rebuild the packed copies of every module whose trainable parameters changed since they were built."""
        for mod, params in self.groups:
            key = tuple((p.data_ptr(), p._version) for p in params)
            if self.keys.get(id(mod)) != key:
                if mod is self.model.mllm.llama_wrapper:
                    mod.refresh_lora()
                else:
                    mod._invalidate()
                self.keys[id(mod)] = key

    def param_key(self):
        return tuple((p.data_ptr(), p._version) for _, p in self.named)

    def set_flags(self):
        saved = [(obj, attr, getattr(obj, attr)) for obj, attr, _ in self.flags]
        for obj, attr, value in self.flags:
            setattr(obj, attr, value)
        return saved

    def grads_for_backward(self):
        """A new zeroed flat gradient vector for this backward.  The views of the previous one may still be held anywhere --
        as p.grad, by torch.autograd.grad's caller, by a tensor hook -- so a vector is never written twice; the caching
        allocator hands the block of a vector nobody holds any more back to the next one."""
        dev = self.book.grads.device
        self.book.grads = self.book.g = None  # (the previous vector's block can serve this allocation if nothing holds it)
        self.book.set_grads(torch.zeros(self.book.total, dtype=torch.float32, device=dev))
        return self.book.grads

def _restore(saved):
    for obj, attr, value in saved:
        setattr(obj, attr, value)


_N_BATCH = 10  # forward's batch arguments, Function inputs ahead of the parameters


class _TrajectoryFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, br, *inputs):
        m = br.model
        x, vision_embs, context_str, poly, poly_len, y, norm_stat, input_ids, attention_mask, labels = inputs[:_N_BATCH]
        saved = br.set_flags()
        try:
            out = m._forward(x, vision_embs, context_str, poly, poly_len, y=y, norm_stat=norm_stat, input_ids=input_ids,
                             attention_mask=attention_mask, labels=labels)
        finally:
            _restore(saved)
        has_loss = isinstance(out, tuple)
        loss, decoded = out if has_loss else (None, out)
        ns = None
        if has_loss:
            ns = norm_stat if torch.is_tensor(norm_stat) else torch.tensor([list(n) for n in norm_stat])
            ns = ns.to(device=x.device, dtype=torch.float32).contiguous()
        L = m.last.final_hidden.shape[1]  # query tokens + text tokens of this pass (the tokenizer branch included)
        ctx.br, ctx.n_forward, ctx.key, ctx.done = br, m._n_forward, br.param_key(), False
        ctx.args = (decoded.detach(), y.contiguous() if has_loss else None, ns, x.contiguous(), x.shape[0], L)
        ctx.has_loss = has_loss
        ctx.mask = [p.requires_grad for _, p in br.named]  # which parameters are inputs (fixed here, not at backward time)
        ctx.set_materialize_grads(False)
        return (loss, decoded) if has_loss else decoded

    @staticmethod
    def backward(ctx, *grads):
        br = ctx.br
        m = br.model
        if ctx.done:
            raise RuntimeError("MultiModalTrajectoryModel: a second backward through the same forward is not supported "
                               "(the hand-written backward does not keep its graph); run the forward again")
        if m._n_forward != ctx.n_forward:
            raise RuntimeError(f"MultiModalTrajectoryModel: backward of a stale forward -- the model ran "
                               f"{m._n_forward - ctx.n_forward} forward pass(es) since, which overwrote the activations this "
                               "backward reads; call backward before the next forward")
        if br.param_key() != ctx.key:
            raise RuntimeError("MultiModalTrajectoryModel: a trainable parameter was modified in place between this forward "
                               "and its backward")
        batch_grad = [i for i in range(_N_BATCH) if ctx.needs_input_grad[1 + i]]
        if batch_grad:
            raise RuntimeError("MultiModalTrajectoryModel: a batch tensor of forward() requires grad (argument "
                               f"{', '.join(_BATCH_NAMES[i] for i in batch_grad)}); the backward produces parameter gradients "
                               "only -- detach it, or train what produced it separately")
        n_in = 1 + _N_BATCH + sum(ctx.mask)
        g_loss, g_dec = grads if ctx.has_loss else (None, grads[0])
        if g_loss is None and g_dec is None:
            return (None,) * n_in
        ctx.done = True
        decoded, y, ns, x, B, L = ctx.args
        if g_loss is not None:
            g_loss = g_loss.detach().to(torch.float32).reshape(1).contiguous()
        if g_dec is not None:
            g_dec = g_dec.detach().to(torch.float32).contiguous()
        flat = br.grads_for_backward()
        saved = br.set_flags()
        try:
            run_backward(m, br.bw, br.lbw, br.qbw, decoded, y, ns, x, B, L, seed=(g_loss, g_dec))
        finally:
            _restore(saved)
        out = []
        for (n, _), on in zip(br.named, ctx.mask):
            if on:
                o, sz, shape = br.book.offsets[n]
                out.append(flat[o:o + sz].view(shape))
        return (None,) * (1 + _N_BATCH) + tuple(out)


_BATCH_NAMES = ("x", "vision_embs", "context_str", "lane_polygon_batch", "lane_polygon_len", "y", "norm_stat", "input_ids",
                "attention_mask", "labels")


def bridge_forward(model, kind, x, vision_embs, context_str, lane_polygon_batch, lane_polygon_len, y, norm_stat, input_ids,
                   attention_mask, labels):
    """MultiModalTrajectoryModel.forward with an autograd graph over its trainable parameters (set `kind`)."""
    br = model._bridge
    if br is None or br.kind != kind:
        br = model._bridge = _Bridge(model, kind)
    params = [p for _, p in br.named if p.requires_grad]
    return _TrajectoryFunction.apply(br, x, vision_embs, context_str, lane_polygon_batch, lane_polygon_len, y, norm_stat,
                                     input_ids, attention_mask, labels, *params)
