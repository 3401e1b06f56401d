"""CPU-side checks of the slot pool (LlamaMultiModal.generate_pool): the two new symbols and the ctypes mirror of
tcavt_slot_admit_args against the header compiled with the host C compiler, the refusals that need no device, the slot scheduler
on a scripted `finished` feed, generate_pool's argument errors, and its host call sequence against a stub library."""
import ctypes
import itertools
import os
import subprocess

import pytest
import torch

from test_lm_loss_abi_cpu import ROOT, _struct_fields

NEW = ("tcavt_sample_logits_slots", "tcavt_slot_admit")


def test_symbols_are_exported_and_abi_version_stays():
    from tcavt_amd import capi

    assert set(NEW) <= set(capi.EXPORTED_SYMBOLS)
    handle = ctypes.CDLL(capi.LIB_PATH)
    assert all(hasattr(handle, n) for n in NEW)
    assert capi.lib().tcavt_abi_version() == capi.ABI_VERSION == 5


def test_admit_mirror_matches_header_layout(tmp_path):
    from tcavt_amd import capi

    cls, cname = capi.SlotAdmitArgs, "tcavt_slot_admit_args"
    names = _struct_fields(cname)
    assert names == [f[0] for f in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tcavt.h"\nint main(void) {\n'
                   + f'  printf("%zu\\n", sizeof({cname}));\n'
                   + "".join(f'  printf("%zu\\n", offsetof({cname}, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(cls)
    assert out[1:] == [getattr(cls, n).offset for n in names]


F16_PTRS = ("src_k", "src_v", "dst_k", "dst_v")
KV8_PTRS = ("src_k_codes", "src_k_scales", "src_v_codes", "src_v_scales", "dst_k_codes", "dst_k_scales", "dst_v_codes", "dst_v_scales")
STATE_PTRS = ("prompt_ids", "kv_len", "history", "hist_len", "step", "max_new", "out_row", "pos", "finished", "cur_tok")


def _admit_args(capi, form):
    """Arguments that would launch (fake, aligned pointers: every call below is refused first)."""
    a = capi.SlotAdmitArgs()
    for n in (F16_PTRS if form == "f16" else KV8_PTRS) + STATE_PTRS:
        setattr(a, n, 256)
    a.n_layers, a.S, a.slot, a.rows, a.src_lmax, a.kv_lmax, a.nkv, a.dtype16 = 2, 3, 1, 36, 40, 72, 2, capi.F16
    a.n_ids, a.hist_cap, a.n_image, a.max_new_value, a.out_row_value = 20, 32, 16, 5, 4
    return a


def test_slot_admit_refuses_bad_arguments_without_a_device():
    from tcavt_amd import capi

    lib = capi.lib()

    def refused(a, msg):
        rc = lib.tcavt_slot_admit(ctypes.byref(a), None) if a is not None else lib.tcavt_slot_admit(None, None)
        err = lib.tcavt_last_error()
        assert rc == 1 and err.startswith(b"slot_admit:") and msg in err, (rc, err, msg)

    refused(None, b"args")
    for form in ("f16", "kv8"):
        a = _admit_args(capi, form)
        a.rows = 41  # > src_lmax
        refused(a, b"rows = 41")
        a = _admit_args(capi, form)
        a.kv_lmax, a.rows = 30, 36  # > kv_lmax
        refused(a, b"rows = 36")
        a = _admit_args(capi, form)
        a.rows = 0
        refused(a, b"rows = 0")
        for slot in (-1, 3):
            a = _admit_args(capi, form)
            a.slot = slot
            refused(a, b"slot = %d outside" % slot)
        for n in STATE_PTRS:
            a = _admit_args(capi, form)
            setattr(a, n, None)
            refused(a, n.encode())
        for n in (F16_PTRS if form == "f16" else KV8_PTRS):  # one pointer of the form missing
            a = _admit_args(capi, form)
            setattr(a, n, None)
            refused(a, b"null pointer")
        for n in (KV8_PTRS if form == "f16" else F16_PTRS):  # one pointer of the other form on top
            a = _admit_args(capi, form)
            setattr(a, n, 256)
            refused(a, b"exclude each other")
        a = _admit_args(capi, form)
        a.n_ids = 33
        refused(a, b"n_ids = 33")
        a = _admit_args(capi, form)
        a.dtype16 = capi.F32
        refused(a, b"dtype16")
    for n in ("src_k_codes", "src_v_codes", "dst_k_codes", "dst_v_codes"):
        a = _admit_args(capi, "kv8")
        setattr(a, n, 264)
        refused(a, b"code planes must be 16-byte aligned")
    a = _admit_args(capi, "kv8")
    a.dst_v_scales = 257
    refused(a, b"scale planes")
    a = _admit_args(capi, "f16")
    a.dst_k = 264
    refused(a, b"16-byte aligned")
    a = capi.SlotAdmitArgs()  # neither form
    for n in STATE_PTRS:
        setattr(a, n, 256)
    refused(a, b"null pointer")


def test_sample_logits_slots_refuses_bad_arguments_without_a_device():
    from tcavt_amd import capi

    lib = capi.lib()
    names = ["logits", "S", "V", "history", "hist_cap", "hist_len", "params", "step", "max_new", "out_row", "cur_tok", "pos", "finished",
             "out_tokens", "out_cap", "advance_pos", "workspace", "workspace_bytes", "stream"]
    sp = capi.SampleParams(0.9, 0.9, 1.2, 40, 3, 1, -1, 0, 1)

    def call(**kw):
        v = dict(logits=256, S=2, V=512, history=256, hist_cap=8, hist_len=256, params=ctypes.byref(sp), step=256, max_new=256, out_row=256,
                 cur_tok=256, pos=256, finished=256, out_tokens=256, out_cap=4, advance_pos=1, workspace=None, workspace_bytes=0,
                 stream=None)
        v.update(kw)
        rc = lib.tcavt_sample_logits_slots(*[v[n] for n in names])
        return rc, lib.tcavt_last_error()

    for n in ("logits", "history", "hist_len", "params", "step", "max_new", "out_row", "cur_tok", "pos", "finished", "out_tokens"):
        rc, err = call(**{n: None})
        assert rc == 1 and err.startswith(b"sample_logits_slots:") and n.encode() in err and b"null" in err, (n, rc, err)
    for n in ("S", "V", "hist_cap", "out_cap"):
        rc, err = call(**{n: 0})
        assert rc == 1 and err.startswith(b"sample_logits_slots:") and n.encode() + b" = 0" in err, (n, rc, err)
    for bad in (dict(top_k=0), dict(top_k=257), dict(temperature=0.0), dict(top_p=0.0), dict(repetition_penalty=0.0),
                dict(no_repeat_ngram_size=-1)):
        p2 = capi.SampleParams(0.9, 0.9, 1.2, 40, 3, 1, -1, 0, 1)
        for k, v in bad.items():
            setattr(p2, k, v)
        rc, err = call(params=ctypes.byref(p2))
        assert rc == 1 and err.startswith(b"sample_logits_slots:") and next(iter(bad)).split("_")[0].encode() in err, (bad, rc, err)
    rc, err = call(workspace=264, workspace_bytes=1 << 30)  # a workspace that is large enough and misaligned
    assert rc == 1 and b"workspace must be 16-byte aligned" in err


# ------------------------------------------------------------------------------------------------
# the scheduler on a scripted feed
# ------------------------------------------------------------------------------------------------
def _drive(R, slots, lengths, poll_every=1, max_rounds=10_000):
    """Simulates the device: a request admitted to a slot needs lengths[r] steps; -> (admission log, retire log, rounds)."""
    from tcavt_amd.pool import SlotScheduler

    sched = SlotScheduler(R, slots)
    left = [0] * slots  # steps the slot's live request still needs
    finished = [1] * slots  # idle slots read as finished
    admitted, live_log = [], []
    rounds = 0
    while True:
        for s, r in sched.admissions():
            assert left[s] == 0 and finished[s] == 1, "admitted into a slot that still holds a live request"
            admitted.append((r, s))
            left[s], finished[s] = lengths[r] - 1, int(lengths[r] == 1)  # the first token comes with the admission
        live = [r for r in sched.slot_request if r is not None]
        assert len(live) == len(set(live)) <= slots
        live_log.append(list(sched.slot_request))
        if not sched.busy():
            break
        for _ in range(poll_every):
            for s in range(slots):
                if not finished[s]:
                    left[s] -= 1
                    finished[s] = int(left[s] == 0)
        sched.retire(list(finished))
        rounds += 1
        assert rounds < max_rounds, "the scheduler does not terminate"
    return sched, admitted, live_log, rounds


@pytest.mark.parametrize("poll_every", [1, 4])
def test_scheduler_serves_every_request_once_in_order(poll_every):
    lengths = [3, 9, 1, 5, 2, 7, 4]
    sched, admitted, live_log, rounds = _drive(7, 3, lengths, poll_every)
    assert [r for r, _ in admitted] == list(range(7))  # exactly once, FIFO
    assert sorted(r for r, _ in sched.retired) == list(range(7))
    assert sched.live() == 0 and not sched.busy() and sched.next_request == 7
    assert admitted[:3] == [(0, 0), (1, 1), (2, 2)]
    if poll_every == 1:  # request 2 (one token) ends at once, request 0 after two steps: 3 takes slot 2, 4 takes slot 0
        assert admitted[3:5] == [(3, 2), (4, 0)]
    # a slot is never handed out while its request lives: between two admissions to slot s its request was retired
    for s in range(3):
        reqs = [r for r, s_ in admitted if s_ == s]
        order = [r for r, s_ in sched.retired if s_ == s]
        assert reqs == order


def test_scheduler_with_fewer_requests_than_slots_and_with_none():
    sched, admitted, live_log, rounds = _drive(2, 5, [4, 2])
    assert admitted == [(0, 0), (1, 1)] and rounds == 3 and len(sched.retired) == 2
    assert all(r is None for r in live_log[-1])
    sched, admitted, live_log, rounds = _drive(0, 3, [])
    assert admitted == [] and rounds == 0 and not sched.busy()


def test_scheduler_ignores_the_flag_of_an_idle_slot_and_checks_its_input():
    from tcavt_amd.pool import SlotScheduler

    s = SlotScheduler(1, 2)
    assert s.admissions() == [(0, 0)] and s.admissions() == []
    assert s.retire([0, 1]) == [] and s.busy()  # slot 1 is idle: its flag means nothing
    with pytest.raises(ValueError):
        s.retire([1])
    assert s.retire([1, 1]) == [0] and not s.busy()
    with pytest.raises(ValueError):
        SlotScheduler(3, 0)


# ------------------------------------------------------------------------------------------------
# generate_pool's host side
# ------------------------------------------------------------------------------------------------
def _tiny_model():
    from tcavt_amd import config, model
    from tcavt_amd.weights import make_weights

    cfg = config.tiny()
    return cfg, model.MultiModalTrajectoryModel.from_config(cfg).load_weights(make_weights(cfg, 0)).eval()


def test_generate_pool_raises_on_illegal_arguments_before_touching_a_device():
    cfg, m = _tiny_model()
    ids = torch.zeros(2, 4, dtype=torch.int64)
    mask = torch.ones_like(ids)
    vis = torch.zeros(2, 1, 8)
    for kw, msg in ((dict(slots=0), "slots must be >= 1"), (dict(poll_every=0), "poll_every must be >= 1"),
                    (dict(max_new_tokens=0), "budget"), (dict(max_new_tokens=[3, 0]), "budget"),
                    (dict(max_new_tokens=[3]), "1 budgets for 2 requests"), (dict(max_new_tokens=[3, 3, 3]), "3 budgets for 2 requests"),
                    (dict(kv_cache="fp4"), "kv_cache must be 'fp16' or 'fp8'.*'fp4'"),
                    (dict(decode_weights="int4"), "decode_weights must be 'fp16' or 'fp8'.*'int4'"),
                    (dict(decode_weights="fp8", slots=33), "slots <= 32"), (dict(pad_token_id=cfg.llama.vocab), "pad_token_id")):
        with pytest.raises(ValueError, match=msg):
            m.mllm.generate_pool(vis, ids, mask, **kw)
    with pytest.raises(ValueError, match="must agree"):
        m.mllm.generate_pool(vis, ids, mask[:, :3])
    with pytest.raises(ValueError, match="must agree"):
        m.mllm.generate_pool(vis[:1], ids, mask)
    # no request: an empty result of the right shape, and nothing is launched
    out = m.mllm.generate_pool(vis[:0], ids[:0], mask[:0], max_new_tokens=5)
    assert out.dtype == torch.int64 and tuple(out.shape) == (0, 5)


def test_generate_pool_call_sequence_against_a_stub_library(monkeypatch):
    """The host side of generate_pool end to end on the CPU: the library is a stub that accepts every call and plays the device's
    part in the slot bookkeeping (admission resets a slot, the sampler counts steps up to the budget), so every wrapper's host
    guard sees the real shapes, and the loop must admit each request once, in order, and stop."""
    from tcavt_amd import capi, ops

    calls, admitted = [], []
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)

    class Stub:
        def __getattr__(self, name):
            if not name.startswith("tcavt_"):
                raise AttributeError(name)

            def fn(*args):
                calls.append(name)
                if name == "tcavt_slot_admit":
                    a = args[0]._obj
                    admitted.append((a.out_row_value, a.slot, a.rows, a.src_lmax, a.kv_lmax, a.max_new_value))
                    ctypes.cast(a.step, i32p)[a.slot] = 0
                    ctypes.cast(a.finished, i32p)[a.slot] = 0
                    ctypes.cast(a.max_new, i32p)[a.slot] = a.max_new_value
                    ctypes.cast(a.out_row, i64p)[a.slot] = a.out_row_value
                if name == "tcavt_sample_logits_slots":
                    S = args[1]
                    step, max_new, fin = (ctypes.cast(args[i], i32p) for i in (7, 8, 12))
                    for s in range(S):
                        if not fin[s]:
                            step[s] += 1
                            fin[s] = int(step[s] == max_new[s])
                return 0

            return fn

    monkeypatch.setattr(ops, "lib", lambda: Stub())
    monkeypatch.setattr(ops, "stream_ptr", lambda: None)
    monkeypatch.setattr(ops, "_ALLOW_CPU", True)
    monkeypatch.setenv("TCAVT_DECODE_ROWMAJOR", "1")  # (packing the fragment-major weight copies needs a device stream)
    cfg, m = _tiny_model()
    R, Lt = 5, 6
    ids = torch.randint(0, cfg.llama.vocab, (R, Lt), generator=torch.Generator().manual_seed(0))
    mask = torch.ones_like(ids)
    vis = torch.zeros(R, 1, cfg.vision_dim) if hasattr(cfg, "vision_dim") else torch.zeros(R, 1, 8)
    budgets = [3, 1, 6, 2, 4]
    for kv in ("fp16", "fp8"):
        calls.clear()
        admitted.clear()
        out = m.mllm.generate_pool(vis, ids, mask, max_new_tokens=budgets, slots=2, poll_every=2, use_graph=False, pad_token_id=7, kv_cache=kv)
        assert tuple(out.shape) == (R, 6) and bool((out == 7).all())  # (the stub writes no token)
        assert [a[0] for a in admitted] == list(range(R))
        assert all(a[2:] == (16 + Lt, 16 + Lt, 16 + Lt + 6, budgets[a[0]]) for a in admitted)
        assert calls.count("tcavt_slot_admit") == calls.count("tcavt_llama_stack_forward") == calls.count("tcavt_gather_last") == R
        steps = m.mllm.pool_stats["steps"]
        st = m.mllm.pool_stats
        assert [a[0] for a in st["admitted"]] == list(range(R)) and sorted(a[0] for a in st["retired"]) == list(range(R))
        assert steps % 2 == 1  # the first step is eager and unpolled, then groups of poll_every
        assert calls.count("tcavt_llama_decode_step") == steps
        assert calls.count("tcavt_sample_logits_slots") == steps + R
        assert calls.count("tcavt_sample_logits") == 0


# every combination the entry accepts (top_logprobs needs return_logprobs=True: the others are refused, test_top_logprobs_trace_cpu)
@pytest.mark.parametrize("return_info, return_logprobs, top_logprobs, constrained",
                         [c for c in itertools.product([False, True], [False, True], [None, 4], [False, True]) if c[1] or c[2] is None])
def test_the_stats_of_an_empty_request_list_are_those_of_a_served_one_with_no_rows(return_info, return_logprobs, top_logprobs, constrained):
    """generate_pool on no request against generation_stub.POOL_1's five: the same keys, and every per-request tensor with the same
    dtype and trailing shape and a leading dimension of 0 -- with nothing called and no workspace buffer requested."""
    import generation_stub as GS
    from tcavt_amd.constraint import TokenConstraint

    with GS.stubbed() as stub:
        cfg, m = GS.tiny_model()
        kw = dict(GS.POOL_1, use_graph=False, pad_token_id=7, return_info=return_info, return_logprobs=return_logprobs, top_logprobs=top_logprobs)
        if constrained:
            kw.update(constraint=TokenConstraint.from_sequences(cfg.llama.vocab, [[11, 12], [30]], 5), no_repeat_ngram_size=0)
        vis, ids, mask = GS._requests(cfg, 5)
        m.mllm.generate_pool(vis, ids, mask, **kw)
        served = m.mllm.pool_stats
        _, m0 = GS.tiny_model()
        n_calls = len(stub.calls)
        m0.mllm.generate_pool(vis[:0], ids[:0], mask[:0], **dict(kw, max_new_tokens=max(GS.POOL_1["max_new_tokens"])))
        empty = m0.mllm.pool_stats
        assert len(stub.calls) == n_calls and not m0.mllm._ws._bufs
    assert list(empty) == list(served)
    for key, t in served.items():
        if isinstance(t, torch.Tensor):
            assert t.shape[0] == 5 and empty[key].dtype == t.dtype and tuple(empty[key].shape) == (0,) + tuple(t.shape[1:]), key
        else:
            assert empty[key] == (0 if key == "steps" else []), key
