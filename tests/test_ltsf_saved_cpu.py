"""TransformerLTSF.saved, the record its backward reads (CPU, stub library of tests/test_host_dryrun.py's seam): one
Trainer.step per form -- frozen default (C stages), frozen with TCAVT_PY_TLAYERS=1, frozen on bf16 storage (the un-absorbed
composition), LoRA-trainable, train mode with dropout -- on tiny_6_12_lora_ragged.  The backward asks no workspace for a
forward buffer (no ``lt.*`` / ``sab.*`` request during Backward.run or lora_backward, and lora_backward does not ask for
``xa.g_k`` / ``xa.g_v``), the record aliases the forward's workspace buffers, a second forward replaces it, and a backward
without a record raises before its first C call.  No arithmetic happens here; numerics are the GPU tests' job."""
import pytest
import torch

from tests.util import batch_tensors, load_case

FORMS = {  # name -> (environment, setup(model) or None, lora_trainable, train mode)
    "stages": ({}, None, False, False),
    "py_tlayers": ({"TCAVT_PY_TLAYERS": "1"}, None, False, False),
    "bf16": ({}, lambda m: m.set_storage(torch.bfloat16), False, False),
    "lora": ({}, None, True, False),
    "dropout": ({}, None, False, True),
}
INPUTS = ("x", "poly_emb", "final_hidden_bf16")  # the record's tensors that are the forward's arguments, not its buffers
REMOVED = ("_absorbed", "stage", "xattn_stage", "drop_post", "drop_xattn")


class _StubLib:
    """Accepts every C entry; keeps the entries' names and the batch size B that each LTSF backward call carries."""

    def __init__(self):
        self.calls, self.batch = [], []

    def __getattr__(self, name):
        if not name.startswith("tcavt_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append(name)
            if name == "tcavt_ltsf_backward":  # the stage: B of the forward struct it is handed
                self.batch.append(args[0]._obj.fwd.contents.B)
            elif name == "tcavt_out_head_bwd":  # the composition's first launch: (..., B, To, C, F, stream)
                self.batch.append(getattr(args[6], "value", args[6]))
            return 0

        return fn


@pytest.fixture
def dry(monkeypatch):
    from tcavt_amd import ops

    stub = _StubLib()
    monkeypatch.setattr(ops, "lib", lambda: stub)
    monkeypatch.setattr(ops, "stream_ptr", lambda: None)
    monkeypatch.setattr(ops, "_ALLOW_CPU", True)
    return stub


def _trainer(monkeypatch, form):
    from tcavt_amd import model, training

    env, setup, lora, train = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, weights, fx = load_case("tiny_6_12_lora_ragged")
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights)
    m.train(train)
    if setup is not None:
        setup(m)
    return m, training.Trainer(m, lora_trainable=lora, max_grad_norm=1.0 if lora else None), batch_tensors(fx)


def _args(t, n=None):
    """Trainer.step's arguments from the fixture's tensors (the first n samples)."""
    keys = ("traj_emb", "vision_emb", "lane_polygon", "lane_polygon_len", "target_traj", "norm_stat", "input_ids",
            "attention_mask", "labels")
    return [t[k][:n] for k in keys]


def _forward_keys(m):
    return {k for mod in (m.ltsf, m.ltsf.attn_block) for k in mod._ws._bufs if k[0].startswith(("lt.", "sab."))}


def _tensors(ns):
    return {k: v for k, v in vars(ns).items() if torch.is_tensor(v)}


@pytest.mark.parametrize("form", list(FORMS))
def test_backward_reads_the_record_and_no_forward_buffer_by_name(dry, monkeypatch, form):
    from tcavt_amd import backward, parts, training

    m, tr, t = _trainer(monkeypatch, form)
    lora = FORMS[form][2]
    phase, requests, at_entry = [], [], {}
    get, run, lora_backward = parts._Workspace.get, backward.Backward.run, training.lora_backward

    def logged_get(self, name, *a, **kw):
        if phase:
            requests.append((phase[-1], name))
        return get(self, name, *a, **kw)

    def logged_run(self, *a, **kw):  # entry = the state the forward left behind
        sv = m.ltsf.saved
        at_entry.update(record=sv, keys=_forward_keys(m),
                        ptrs={b.data_ptr() for mod in (m.ltsf, m.ltsf.attn_block) for b in mod._ws._bufs.values()})
        phase.append("run")
        try:
            return run(self, *a, **kw)
        finally:
            phase.pop()

    def logged_lora_backward(*a, **kw):
        phase.append("lora_backward")
        try:
            return lora_backward(*a, **kw)
        finally:
            phase.pop()

    monkeypatch.setattr(parts._Workspace, "get", logged_get)
    monkeypatch.setattr(backward.Backward, "run", logged_run)
    monkeypatch.setattr(training, "lora_backward", logged_lora_backward)

    B = t["traj_emb"].shape[0]
    tr.step(*_args(t))
    sv = m.ltsf.saved
    assert sv is at_entry["record"] and (sv.B, sv.T) == (B, t["traj_emb"].shape[2])
    assert {p for p, _ in requests} == ({"run", "lora_backward"} if lora else {"run"})
    assert [r for r in requests if r[1].startswith(("lt.", "sab."))] == []
    assert [r for r in requests if r[0] == "lora_backward" and r[1] in ("bw.xa.g_k", "bw.xa.g_v")] == []
    # the record aliases the forward's buffers and its inputs: nothing is copied
    held = {**_tensors(sv), **{"sab." + k: v for k, v in _tensors(sv.sab).items()}}
    assert {"tok", "xp", "e", "d0", "dec_tb", "proj", "q", "S", "P", "att", "cross", "fused", "fn", "f1", "f2", "sab.xn", "sab.qkv",
            "sab.att", "sab.res1", "sab.rn", "sab.f", "sab.out"} <= set(held)
    assert ({"qp", "ctx", "fhT"} if sv.absorbed else {"k", "vT"}) <= set(held)
    assert sv.absorbed == (form not in ("bf16", "lora")) and (sv.stage is not None) == (form in ("stages", "dropout"))
    for name, buf in held.items():
        if name not in INPUTS:
            assert buf.data_ptr() in at_entry["ptrs"], name
    assert sv.poly_emb is m.last.poly_emb and sv.final_hidden_bf16 is m.last.final_hidden_bf16
    assert sv.x.data_ptr() == t["traj_emb"].data_ptr()
    assert len(sv.sab_drop) == 4 and all((s is not None) == (form == "dropout") for s in sv.sab_drop + [sv.drop_post, sv.drop_xattn])
    # the backward added no forward buffer to the workspaces
    assert _forward_keys(m) == at_entry["keys"]
    if lora:
        g_k, g_v = tr.bw.kv_grads
        assert g_k is tr.bw._buf("xa.g_k", tuple(g_k.shape), torch.bfloat16) and g_v is tr.bw._buf("xa.g_v", tuple(g_v.shape), torch.bfloat16)
    # the loose attributes the record replaces are gone
    assert not any(hasattr(m.ltsf, a) for a in REMOVED) and not hasattr(m.ltsf.attn_block, "drop_specs")
    assert not any(hasattr(tr.bw, a) for a in ("_poly_emb", "_fh_b", "_L"))
    assert dry.batch == [B]

    # a second forward, one sample fewer: a new record, and the backward that follows carries the new B
    del dry.calls[:], dry.batch[:]
    tr.step(*_args(t, B - 1))
    assert m.ltsf.saved is not sv and m.ltsf.saved.B == B - 1 and at_entry["record"] is m.ltsf.saved
    assert dry.batch == [B - 1]


@pytest.mark.parametrize("form", ["stages", "lora"])
def test_backward_without_a_record_raises_before_any_c_call(dry, monkeypatch, form):
    from tcavt_amd import training

    m, tr, t = _trainer(monkeypatch, form)
    x, y, ns = t["traj_emb"], t["target_traj"], t["norm_stat"].float().contiguous()
    B, L = x.shape[0], m.mllm.qformer.num_query_tokens + t["input_ids"].shape[1]
    del dry.calls[:]
    if form == "lora":  # no Backward.run yet: no dL/dk, dL/dv to start the decoder's backward from
        with pytest.raises(RuntimeError, match="lora_backward"):
            training.lora_backward(m, tr.bw, tr.lbw, tr.qbw, B, L)
        assert dry.calls == []
    _, decoded = tr.forward_backward(*_args(t))
    assert m.ltsf.saved is not None and (tr.bw.kv_grads is not None) == (form == "lora")
    m.ltsf.saved = None
    del dry.calls[:]
    with pytest.raises(RuntimeError, match="TransformerLTSF"):
        tr.bw.run(decoded, y, ns, x)
    assert dry.calls == [] and tr.bw.kv_grads is None
    if form == "lora":  # run() reset what the earlier backward had left
        with pytest.raises(RuntimeError, match="lora_backward"):
            training.lora_backward(m, tr.bw, tr.lbw, tr.qbw, B, L)
        assert dry.calls == []


def test_forward_without_save_for_backward_leaves_no_record(dry, monkeypatch):
    m, tr, t = _trainer(monkeypatch, "stages")
    m.ltsf.save_for_backward = False
    with torch.no_grad():
        m(t["traj_emb"], t["vision_emb"], None, t["lane_polygon"], t["lane_polygon_len"], input_ids=t["input_ids"],
          attention_mask=t["attention_mask"])
    assert m.ltsf.saved is None and m.ltsf._front is None
