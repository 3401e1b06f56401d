"""A stub library for the CPU tests of text generation's host code (generation.py): it accepts every C entry, records the call
with its integer scalars and plays the device's part in the bookkeeping that the host loops wait on -- an admission resets its
slot, a sampler call counts steps and finishes rows -- so generate_batch / generate_pool run end to end on CPU tensors.

``record_all()`` runs the scenarios of tests/test_generation_trace_cpu.py and returns {scenario: {"calls", "workspace"}};
``python tests/generation_stub.py OUT.json`` writes that as the golden file (run with the package of the commit to record on
the path)."""
import contextlib
import ctypes
import functools
import json
import os
import sys

import torch

I32P, I64P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
INT_TYPES = (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64)  # (c_int is c_int32 here)
FINISH_AT = 4  # the batch form has no budget on the device: every row ends when the step word reaches this
EOS, BUDGET = 1, 4  # stopping.py's finish reasons, as the stub reports them


def _scalars(sig, args):
    """The integer arguments of a call, in order; a struct passed by reference contributes a dict of its integer fields."""
    out = []
    for t, v in zip(sig, args):
        if t in INT_TYPES:
            out.append(int(v))
        elif isinstance(t, type) and issubclass(t, ctypes._Pointer) and issubclass(t._type_, ctypes.Structure) and v is not None:
            s = v._obj if hasattr(v, "_obj") else v.contents
            out.append({n: int(getattr(s, n)) for n, ft in s._fields_ if ft in INT_TYPES})
    return out


class StubLibrary:
    def __init__(self):
        self.calls = []  # [name, integer scalars] per C entry, in call order

    def __getattr__(self, name):
        if not name.startswith("tcavt_"):
            raise AttributeError(name)
        from tcavt_amd import capi

        def fn(*args):
            self.calls.append([name, _scalars(capi._SIGNATURES[name], args)])
            play = getattr(self, "_" + name[len("tcavt_"):], None)
            if play is not None:
                play(*args)
            return 0

        return fn

    # ---- admissions: the slot's state as the kernels leave it
    @staticmethod
    def _reset(a, slot, budget, out_row):
        ctypes.cast(a.step, I32P)[slot] = 0
        ctypes.cast(a.finished, I32P)[slot] = 0
        ctypes.cast(a.max_new, I32P)[slot] = budget
        ctypes.cast(a.out_row, I64P)[slot] = out_row

    def _slot_admit(self, args, stream):
        a = args._obj
        self._reset(a, a.slot, a.max_new_value, a.out_row_value)

    def _slot_admit_group(self, args, stream):
        a = args._obj
        slot, budget, rows = ctypes.cast(a.slot, I32P), ctypes.cast(a.max_new_value, I32P), ctypes.cast(a.out_row_value, I64P)
        for g in range(a.G):
            if slot[g] >= 0:
                self._reset(a, slot[g], budget[g], rows[g])

    # ---- samplers: no token is written; the step counts up and a row ends at FINISH_AT (batch) or at its budget (slots)
    @staticmethod
    def _advance(live, step, fin, max_new=None, out_row=None, stop=None):
        step, fin = ctypes.cast(step, I32P), ctypes.cast(fin, I32P)
        if max_new is None:
            step[0] += 1
        else:
            max_new, out_row = ctypes.cast(max_new, I32P), ctypes.cast(out_row, I64P)
        for s in live:
            if fin[s]:
                continue
            if max_new is not None:
                step[s] += 1
            n, end = (step[0], FINISH_AT) if max_new is None else (step[s], max_new[s])
            fin[s] = int(n == end)
            if fin[s] and stop:  # the request's records (tcavt_stop_rules)
                r = s if max_new is None else out_row[s]
                ctypes.cast(stop.contents.finish_reason, I32P)[r] = EOS if max_new is None else BUDGET
                ctypes.cast(stop.contents.n_generated, I32P)[r] = n

    def _sample_logits(self, *a):
        self._advance(range(a[1]), a[7], a[10])

    def _sample_logits_slots(self, *a):
        self._advance(range(a[1]), a[7], a[12], a[8], a[9])

    def _sample_logits_rows(self, *a):
        m = ctypes.cast(a[3], I32P)
        self._advance([m[g] for g in range(a[1]) if m[g] >= 0], a[9], a[14], a[10], a[11])

    def _sample_tokens(self, args, stream):
        a = args._obj
        live = range(a.rows)
        if a.slot_of_row:
            m = ctypes.cast(a.slot_of_row, I32P)
            live = [m[g] for g in range(a.rows) if m[g] >= 0]
        self._advance(live, a.step, a.finished, a.max_new, a.out_row, a.stop)


@contextlib.contextmanager
def stubbed():
    """ops runs against a fresh StubLibrary on CPU tensors; everything is put back on exit."""
    from tcavt_amd import ops

    stub = StubLibrary()
    saved = (ops.lib, ops.stream_ptr, ops._ALLOW_CPU, os.environ.get("TCAVT_DECODE_ROWMAJOR"))
    ops.lib, ops.stream_ptr, ops._ALLOW_CPU = (lambda: stub), (lambda: None), True
    os.environ["TCAVT_DECODE_ROWMAJOR"] = "1"  # (packing the fragment-major weight copies needs a device stream)
    try:
        yield stub
    finally:
        ops.lib, ops.stream_ptr, ops._ALLOW_CPU = saved[:3]
        if saved[3] is None:
            del os.environ["TCAVT_DECODE_ROWMAJOR"]
        else:
            os.environ["TCAVT_DECODE_ROWMAJOR"] = saved[3]


@functools.lru_cache(maxsize=None)
def _tiny_weights():
    from tcavt_amd import config
    from tcavt_amd.weights import make_weights

    cfg = config.tiny()
    return cfg, make_weights(cfg, 0)


def tiny_model():
    """A fresh tiny model (fresh workspaces: their allocation order is part of a trace) on the weights made once."""
    from tcavt_amd import model

    cfg, weights = _tiny_weights()
    return cfg, model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights).eval()


def _requests(cfg, R, Lt=6):
    ids = torch.arange(R)[:, None] * 10 + torch.arange(Lt)[None]
    return torch.zeros(R, 1, cfg.vision_dim), ids, torch.ones_like(ids)


RULES = dict(stop_token_ids=[3, 5], return_info=True)
POOL_1 = dict(max_new_tokens=[3, 1, 6, 2, 4], slots=2, poll_every=2, admit_group=1)  # test_generate_pool_cpu's case
POOL_2 = dict(max_new_tokens=[3, 1, 6, 2, 4, 5, 2], slots=4, poll_every=1, admit_group=2)  # test_pool_groups_cpu's case
SCENARIOS = {  # name -> (entry, requests, keyword arguments)
    "batch_n1": ("generate_batch", 3, dict(max_new_tokens=1)),
    "batch_n2": ("generate_batch", 3, dict(max_new_tokens=2)),
    "batch_n5": ("generate_batch", 3, dict(max_new_tokens=5)),
    "batch_rules_poll2": ("generate_batch", 3, dict(max_new_tokens=6, poll_every=2, **RULES)),
    "pool_g1": ("generate_pool", 5, POOL_1),
    "pool_g1_rules": ("generate_pool", 5, dict(POOL_1, **RULES)),
    "pool_g2": ("generate_pool", 7, POOL_2),
    "pool_g2_rules": ("generate_pool", 7, dict(POOL_2, **RULES)),
    "pool_empty": ("generate_pool", 0, dict(max_new_tokens=5, slots=2)),
}


def record(name, kv_cache):
    """One scenario on a fresh model: the C entries called with their integer scalars, and afterwards the (name, shape, dtype)
    of every workspace buffer of the multimodal wrapper and of the decoder, in allocation order."""
    entry, R, kw = SCENARIOS[name]
    with stubbed() as stub:
        cfg, m = tiny_model()
        vis, ids, mask = _requests(cfg, R)
        if entry == "generate_batch":
            m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, pad_token_id=7, kv_cache=kv_cache, **kw)
        else:
            m.mllm.generate_pool(vis, ids, mask, use_graph=False, pad_token_id=7, kv_cache=kv_cache, **kw)
    bufs = [[n, list(shape), str(dt)] for ws in (m.mllm._ws, m.mllm.llama_wrapper._ws) for n, shape, dt in ws._bufs]
    return dict(calls=stub.calls, workspace=bufs)


def record_all():
    return {f"{name}/{kv}": record(name, kv) for name in SCENARIOS for kv in ("fp16", "fp8")}


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(record_all(), f, separators=(",", ":"))
        f.write("\n")
