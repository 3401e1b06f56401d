"""Pieces every module of the model's host side shares: the parameter holders (no compute; their names reproduce the
reference's state-dict keys), the named scratch workspace, the train-mode dropout bookkeeping and the mixin that keeps
packed 16-bit device copies of the parameters."""
import torch
import torch.nn as nn

from . import ops


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
