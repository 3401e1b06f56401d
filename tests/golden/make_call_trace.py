"""Recorder behind tests/test_call_trace_cpu.py and writer of its fixture tests/golden/call_trace.json.

A stub library accepts every C entry on CPU tensors and stores, per call, the entry's name and its arguments read through
``capi._SIGNATURES``: integers and floats verbatim; a struct pointer followed field by field (arrays behind ``layers`` /
``grads`` element by element) as {field: value} WITHOUT the fields that are NULL or zero; every ``void *`` as None (NULL) or
``"p<k>"``, k being the ordinal of the address's first appearance WITHIN THAT CALL -- which arguments alias which, without the
addresses themselves; a ``void **`` as NULL / "set".  After a scenario the (name, shape, dtype) of every workspace buffer of
the model follows, in allocation order.

``python tests/golden/make_call_trace.py OUT.json`` writes the dump of every scenario; the committed file was written at the
commit before model.py was split by class.  A change to it is a change of launches, aliasing or buffers and needs its own
reason.  The file holds every distinct call once (``pool``, one per line) and every distinct workspace buffer once
(``buffers``); a scenario is a list of indices into the pool and, per workspace, a list of indices into the buffers -- most
calls and buffers recur within and across the scenarios.  ``load`` gives back the plain {scenario: {"calls", "workspace"}}."""
import contextlib
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.util import batch_tensors, load_case  # noqa: E402

WORKSPACES = ("lane_polygon_encoder", "mllm", "mllm.qformer", "mllm.llama_wrapper", "ltsf", "ltsf.attn_block")
# the stage forwards whose argument struct the matching stage backward is handed (entry -> the backward that takes it)
STAGE_FORWARDS = {"tcavt_ltsf_forward": "tcavt_ltsf_backward", "tcavt_tlayer_stack_forward": "tcavt_tlayer_stack_backward",
                  "tcavt_cross_attn_forward": "tcavt_cross_attn_backward"}


def _is_struct_ptr(t):
    return isinstance(t, type) and issubclass(t, ctypes._Pointer) and issubclass(t._type_, ctypes.Structure)


class _Dump:
    """The arguments of one call; ``seen`` numbers the addresses in order of first appearance."""

    def __init__(self):
        self.seen = {}

    def pointer(self, v):
        v = getattr(v, "value", v)
        if not v:
            return None
        return "p%d" % self.seen.setdefault(int(v), len(self.seen))

    def struct(self, s):
        out = {}
        for name, ft in s._fields_:
            v = getattr(s, name)
            if not v and not isinstance(v, ctypes.Structure):
                continue  # NULL / zero: left out
            if ft is ctypes.c_void_p:
                out[name] = self.pointer(v)
            elif _is_struct_ptr(ft):
                if not v:
                    out[name] = None
                elif name == "layers":
                    out[name] = [self.struct(v[i]) for i in range(s.n_layers)]
                elif name == "grads":
                    out[name] = [self.struct(v[i]) for i in range(s.fwd.contents.n_layers)]
                else:
                    out[name] = self.struct(v.contents)
            elif isinstance(ft, type) and issubclass(ft, ctypes._Pointer):
                out[name] = "set" if v else None
            elif isinstance(ft, type) and issubclass(ft, ctypes.Structure):
                out[name] = self.struct(v)
            else:
                out[name] = v  # int / float
        return out

    def argument(self, t, v):
        if t is ctypes.c_void_p:
            return self.pointer(v)
        if _is_struct_ptr(t):
            return None if v is None else self.struct(v._obj if hasattr(v, "_obj") else v.contents)
        if isinstance(t, type) and issubclass(t, ctypes._Pointer):
            return None if v is None else "set"
        return v


class RecordingLibrary:
    def __init__(self):
        self.calls = []  # [entry, [argument, ...]] in call order
        # (index into calls, entry, the argument struct itself) of every stage forward and of every stage backward: the objects are
        # kept alive, so an address cannot be reused by a struct built later
        self.stage_forwards, self.stage_backwards = [], []

    def __getattr__(self, name):
        if not name.startswith("tcavt_"):
            raise AttributeError(name)
        from tcavt_amd import capi

        sig = capi._SIGNATURES[name]

        def fn(*args):
            assert len(args) == len(sig), (name, len(args), len(sig))
            d = _Dump()
            if name in STAGE_FORWARDS:
                self.stage_forwards.append((len(self.calls), name, args[0]._obj))
            elif name in STAGE_FORWARDS.values():
                self.stage_backwards.append((len(self.calls), name, args[0]._obj))
            self.calls.append([name, [d.argument(t, v) for t, v in zip(sig, args)]])
            return 0

        return fn


@contextlib.contextmanager
def recording(env=None):
    """ops runs against a fresh RecordingLibrary on CPU tensors, with ``env`` set; everything is put back on exit."""
    from tcavt_amd import ops

    stub = RecordingLibrary()
    saved = (ops.lib, ops.stream_ptr, ops._ALLOW_CPU)
    saved_env = {k: os.environ.get(k) for k in (env or {})}
    ops.lib, ops.stream_ptr, ops._ALLOW_CPU = (lambda: stub), (lambda: None), True
    os.environ.update(env or {})
    try:
        yield stub
    finally:
        ops.lib, ops.stream_ptr, ops._ALLOW_CPU = saved
        for k, v in saved_env.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _forward(m, t):
    with torch.no_grad():
        m(t["traj_emb"], t["vision_emb"], None, t["lane_polygon"], t["lane_polygon_len"], y=t["target_traj"],
          norm_stat=t["norm_stat"], input_ids=t["input_ids"], attention_mask=t["attention_mask"], labels=t["labels"])


def _step(m, t, lora_trainable=False):
    from tcavt_amd import training

    tr = training.Trainer(m, lora_trainable=lora_trainable, max_grad_norm=1.0 if lora_trainable else None)
    tr.step(t["traj_emb"], t["vision_emb"], t["lane_polygon"], t["lane_polygon_len"], t["target_traj"], t["norm_stat"],
            t["input_ids"], t["attention_mask"], t["labels"])


def _lm(entry):
    def run(m, t):
        with torch.no_grad():
            getattr(m.mllm, entry)(t["vision_emb"], None, input_ids=t["input_ids"], attention_mask=t["attention_mask"],
                                   labels=t["labels"])
    return run


LORA, NOLORA = "tiny_6_12_lora_ragged", "tiny_18_30_nolora_ragged"
SCENARIOS = {  # name -> (fixture, train mode, run(model, tensors), environment, setup(model) or None)
    "eval_forward": (LORA, False, _forward, None, None),
    "train_forward": (LORA, True, _forward, None, None),
    "step_frozen": (LORA, False, _step, None, None),
    "step_lora": (LORA, False, lambda m, t: _step(m, t, True), None, None),
    "step_frozen_dropout": (LORA, True, _step, None, None),
    "step_lora_dropout": (LORA, True, lambda m, t: _step(m, t, True), None, None),
    "nolora_eval_forward": (NOLORA, False, _forward, None, None),
    "nolora_step_frozen": (NOLORA, False, _step, None, None),
    "bf16_eval_forward": (LORA, False, _forward, None, lambda m: m.set_storage(torch.bfloat16)),
    "py_tlayers_step_frozen": (LORA, False, _step, {"TCAVT_PY_TLAYERS": "1"}, None),
    "py_tlayers_step_frozen_dropout": (LORA, True, _step, {"TCAVT_PY_TLAYERS": "1"}, None),
    "lm_forward": (LORA, False, _lm("lm_forward"), None, None),
    "lm_evaluate": (LORA, False, _lm("lm_evaluate"), None, None),
}


def record(name):
    """One scenario on a fresh model -> (dump, stub): dump = {"calls", "workspace"}; the stub keeps the stage structs."""
    from tcavt_amd import model

    case, train, run, env, setup = SCENARIOS[name]
    cfg, weights, fx = load_case(case)
    t = batch_tensors(fx)
    with recording(env) as stub:
        m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights)
        m.train(train)
        if setup is not None:
            setup(m)
        run(m, t)
    ws = {}
    for path in WORKSPACES:
        mod = m
        for part in path.split("."):
            mod = getattr(mod, part)
        ws[path] = [[n, list(shape), str(dt)] for n, shape, dt in mod._ws._bufs]
    return dict(calls=stub.calls, workspace=ws), stub


def _index(pool, item):
    return pool.setdefault(json.dumps(item, separators=(",", ":")), len(pool))


def write(path):
    pool, bufs, scenarios = {}, {}, {}
    for name in SCENARIOS:
        d = record(name)[0]
        scenarios[name] = dict(calls=[_index(pool, c) for c in d["calls"]],
                               workspace={k: [_index(bufs, b) for b in v] for k, v in d["workspace"].items()})
    with open(path, "w") as f:
        f.write('{"pool":[\n' + ",\n".join(pool) + '\n],\n"buffers":[' + ",".join(bufs) + '],\n"scenarios":')
        json.dump(scenarios, f, separators=(",", ":"))
        f.write("}\n")


def load(path):
    with open(path) as f:
        d = json.load(f)
    return {name: dict(calls=[d["pool"][i] for i in s["calls"]], workspace={k: [d["buffers"][i] for i in v] for k, v in s["workspace"].items()})
            for name, s in d["scenarios"].items()}


if __name__ == "__main__":
    write(sys.argv[1])
