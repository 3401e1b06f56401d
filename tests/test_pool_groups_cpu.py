"""CPU-side checks of the grouped admissions of LlamaMultiModal.generate_pool (admit_group=G): the scheduler's group policy on a
scripted `finished` feed, the two new entries and the ctypes mirror of tcavt_slot_admit_group_args against the header, the
refusals that need no device, and generate_pool's admit_group errors."""
import ctypes
import os
import subprocess

import pytest
import torch

from test_lm_loss_abi_cpu import ROOT, _struct_fields

NEW = ("tcavt_slot_admit_group", "tcavt_sample_logits_rows")


# ------------------------------------------------------------------------------------------------
# the scheduler on a scripted feed
# ------------------------------------------------------------------------------------------------
def _drive(R, slots, group, lengths):
    """Simulates the device (a request admitted to a slot needs lengths[r] steps; the first token comes with the admission) and
    checks the release rule at EVERY visit: no group while free < min(G, waiting), and one the first time that holds.
    -> (scheduler, groups with the round they went in)."""
    from tcavt_amd.pool import SlotScheduler

    sched = SlotScheduler(R, slots, group)
    left, finished = [0] * slots, [1] * slots
    log, rounds = [], 0
    while True:
        free = [s for s in range(slots) if sched.slot_request[s] is None]
        waiting = R - sched.next_request
        groups = sched.admission_groups()
        for g in groups:
            need = min(group, waiting)
            assert 1 <= len(g) == need <= group  # full, or the whole tail
            assert [s for s, _ in g] == free[:need]  # distinct, free, lowest first
            assert [r for _, r in g] == list(range(R - waiting, R - waiting + need))  # FIFO
            free, waiting = free[need:], waiting - need
            for s, r in g:
                assert left[s] == 0 and finished[s] == 1, "admitted into a slot that still holds a live request"
                left[s], finished[s] = lengths[r] - 1, int(lengths[r] == 1)
            log.append((g, rounds))
        # what is left waiting could not go: fewer free slots than min(G, waiting) -- so a group IS released the first time it can
        assert waiting == 0 or len(free) < min(group, waiting)
        assert free == [s for s in range(slots) if sched.slot_request[s] is None]
        if not sched.busy():
            break
        for s in range(slots):
            if not finished[s]:
                left[s] -= 1
                finished[s] = int(left[s] == 0)
        sched.retire(list(finished))
        rounds += 1
        assert rounds < 1000, "the scheduler does not terminate"
    return sched, log


LENGTHS = [3, 9, 1, 5, 2, 7, 4, 6, 2, 8, 3]


@pytest.mark.parametrize("G", [1, 2, 3, 4])
def test_scheduler_releases_fixed_width_groups(G):
    R, S = 11, 4
    sched, log = _drive(R, S, G, LENGTHS)
    served = [r for g, _ in log for _, r in g]
    assert served == list(range(R))  # exactly once, FIFO
    assert sorted(r for r, _ in sched.retired) == list(range(R))
    assert not sched.busy() and sched.live() == 0 and sched.next_request == R
    assert all(len(g) <= G for g, _ in log)
    # at the start S // G full groups go at once
    first = [g for g, at in log if at == 0]
    assert len(first) == S // G and all(len(g) == G for g in first)
    assert [s for g in first for s, _ in g] == list(range(S // G * G))
    # every group but possibly the last is full; the tail (R % G requests) is admitted
    assert all(len(g) == G for g, _ in log[:-1]) and len(log[-1][0]) == (R % G or G)
    assert len(log) == -(-R // G)


def test_group_one_is_todays_admission_sequence():
    from tcavt_amd.pool import SlotScheduler

    R, S = 11, 4
    a, b = SlotScheduler(R, S), SlotScheduler(R, S, 1)
    left_a, left_b = [0] * S, [0] * S
    for _ in range(200):
        x = a.admissions()
        y = b.admission_groups()
        assert all(len(g) == 1 for g in y) and x == [g[0] for g in y]
        for s, r in x:
            left_a[s] = left_b[s] = LENGTHS[r]
        if not a.busy():
            break
        left_a = [max(v - 1, 0) for v in left_a]
        fin = [int(v == 0) for v in left_a]
        assert a.retire(fin) == b.retire(fin)
    assert not a.busy() and not b.busy() and a.retired == b.retired and len(a.retired) == R


def test_scheduler_refuses_a_group_wider_than_the_pool():
    from tcavt_amd.pool import SlotScheduler

    with pytest.raises(ValueError, match="group"):
        SlotScheduler(5, 3, 4)
    with pytest.raises(ValueError, match="group"):
        SlotScheduler(5, 3, 0)
    assert SlotScheduler(5, 3, 3).admission_groups() == [[(0, 0), (1, 1), (2, 2)]]
    s = SlotScheduler(2, 4, 3)  # a queue shorter than the group goes at once
    assert s.admission_groups() == [[(0, 0), (1, 1)]] and s.admission_groups() == []


def test_pool_module_stays_free_of_torch():
    src = open(os.path.join(ROOT, "traffic-context-augmented-vehicle-trajectory-prediction-framework-using-multimodal-llm_amd",
                            "pool.py")).read()
    assert not [ln for ln in src.splitlines() if ln.lstrip().startswith(("import ", "from "))]


# ------------------------------------------------------------------------------------------------
# ABI surface
# ------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_abi_version_stays():
    from tcavt_amd import capi

    header = open(os.path.join(ROOT, "include", "tcavt.h")).read()
    for n in NEW:
        assert f"int {n}(" in header
    assert "} tcavt_slot_admit_group_args;" in header
    assert set(NEW) <= set(capi.EXPORTED_SYMBOLS)
    handle = ctypes.CDLL(capi.LIB_PATH)
    assert all(hasattr(handle, n) for n in NEW)
    assert capi.lib().tcavt_abi_version() == capi.ABI_VERSION == 5


def test_admit_group_mirror_matches_header_layout(tmp_path):
    from tcavt_amd import capi

    cls, cname = capi.SlotAdmitGroupArgs, "tcavt_slot_admit_group_args"
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


def test_rows_sampler_prototype_matches_the_header():
    """The header's parameter list, in order, against the ctypes prototype: pointers, ints and the one int64."""
    import re

    from tcavt_amd import capi

    header = open(os.path.join(ROOT, "include", "tcavt.h")).read()
    m = re.search(r"int tcavt_sample_logits_rows\((.*?)\);", header, re.S)
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["logits", "G", "V", "slot_of_row", "S", "history", "hist_cap", "hist_len", "params", "step", "max_new", "out_row",
                     "cur_tok", "pos", "finished", "out_tokens", "out_cap", "advance_pos", "workspace", "workspace_bytes", "stream"]
    kinds = ["p" if ("*" in p or "tcavt_stream_t" in p) else ("q" if "int64_t" in p else "i") for p in params]
    proto = capi._SIGNATURES["tcavt_sample_logits_rows"]
    got = ["q" if t is ctypes.c_int64 else ("i" if t is ctypes.c_int else "p") for t in proto]
    assert got == kinds


F16_PTRS = ("src_k", "src_v", "dst_k", "dst_v")
KV8_PTRS = ("src_k_codes", "src_k_scales", "src_v_codes", "src_v_scales", "dst_k_codes", "dst_k_scales", "dst_v_codes", "dst_v_scales")
ROW_PTRS = ("slot", "kv_len", "max_new_value", "out_row_value", "prompt_ids", "bad_slot_flag")
STATE_PTRS = ("history", "hist_len", "step", "max_new", "out_row", "pos", "finished", "cur_tok")


def _admit_args(capi, form):
    """Arguments that would launch (fake, aligned pointers: every call below is refused first)."""
    a = capi.SlotAdmitGroupArgs()
    for n in (F16_PTRS if form == "f16" else KV8_PTRS) + ROW_PTRS + STATE_PTRS:
        setattr(a, n, 256)
    a.n_layers, a.S, a.G, a.rows, a.src_lmax, a.kv_lmax, a.nkv, a.dtype16 = 2, 4, 3, 5, 5, 9, 2, capi.F16
    a.n_ids, a.hist_cap, a.n_image = 20, 32, 16
    return a


def test_slot_admit_group_refuses_bad_arguments_without_a_device():
    from tcavt_amd import capi

    lib = capi.lib()

    def refused(a, msg):
        rc = lib.tcavt_slot_admit_group(ctypes.byref(a), None) if a is not None else lib.tcavt_slot_admit_group(None, None)
        err = lib.tcavt_last_error()
        assert rc == 1 and err.startswith(b"slot_admit_group:") and msg in err, (rc, err, msg)

    refused(None, b"args")
    for form in ("f16", "kv8"):
        for rows in (0, 6):  # outside [1, src_lmax]
            a = _admit_args(capi, form)
            a.rows = rows
            refused(a, b"rows = %d" % rows)
        a = _admit_args(capi, form)
        a.kv_lmax = 4  # rows > kv_lmax
        refused(a, b"rows = 5")
        for G in (0, -2):
            a = _admit_args(capi, form)
            a.G = G
            refused(a, b"G = %d" % G)
        for n_ids in (-1, 33):
            a = _admit_args(capi, form)
            a.n_ids = n_ids
            refused(a, b"n_ids = %d" % n_ids)
        for n in ROW_PTRS + STATE_PTRS:
            a = _admit_args(capi, form)
            setattr(a, n, None)
            refused(a, n.encode() + b" is a null pointer")
        for n in (F16_PTRS if form == "f16" else KV8_PTRS):  # one pointer of the form missing
            a = _admit_args(capi, form)
            setattr(a, n, None)
            refused(a, b"null pointer")
        for n in (KV8_PTRS if form == "f16" else F16_PTRS):  # one pointer of the other form on top
            a = _admit_args(capi, form)
            setattr(a, n, 256)
            refused(a, b"exclude each other")
        a = _admit_args(capi, form)
        a.dtype16 = capi.F32
        refused(a, b"dtype16")
    for n in ("src_k_codes", "src_v_codes", "dst_k_codes", "dst_v_codes"):
        a = _admit_args(capi, "kv8")
        setattr(a, n, 264)
        refused(a, b"code planes must be 16-byte aligned")
    a = _admit_args(capi, "kv8")
    a.src_k_scales = 257
    refused(a, b"scale planes")
    a = _admit_args(capi, "f16")
    a.src_v = 264
    refused(a, b"16-byte aligned")


def test_sample_logits_rows_refuses_bad_arguments_without_a_device():
    from tcavt_amd import capi

    lib = capi.lib()
    names = ["logits", "G", "V", "slot_of_row", "S", "history", "hist_cap", "hist_len", "params", "step", "max_new", "out_row", "cur_tok",
             "pos", "finished", "out_tokens", "out_cap", "advance_pos", "workspace", "workspace_bytes", "stream"]
    sp = capi.SampleParams(0.9, 0.9, 1.2, 40, 3, 1, -1, 0, 1)

    def call(**kw):
        v = dict(logits=256, G=2, V=512, slot_of_row=256, S=3, history=256, hist_cap=8, hist_len=256, params=ctypes.byref(sp), step=256,
                 max_new=256, out_row=256, cur_tok=256, pos=256, finished=256, out_tokens=256, out_cap=4, advance_pos=1, workspace=None,
                 workspace_bytes=0, stream=None)
        v.update(kw)
        rc = lib.tcavt_sample_logits_rows(*[v[n] for n in names])
        return rc, lib.tcavt_last_error()

    for n in ("logits", "slot_of_row", "history", "hist_len", "params", "step", "max_new", "out_row", "cur_tok", "pos", "finished",
              "out_tokens"):
        rc, err = call(**{n: None})
        assert rc == 1 and err.startswith(b"sample_logits_rows:") and n.encode() in err and b"null" in err, (n, rc, err)
    for n in ("G", "S", "V", "hist_cap", "out_cap"):
        rc, err = call(**{n: 0})
        assert rc == 1 and err.startswith(b"sample_logits_rows:") and n.encode() + b" = 0" in err, (n, rc, err)
    p2 = capi.SampleParams(0.9, 0.9, 1.2, 257, 3, 1, -1, 0, 1)
    rc, err = call(params=ctypes.byref(p2))
    assert rc == 1 and err.startswith(b"sample_logits_rows:") and b"top_k" in err
    rc, err = call(workspace=264, workspace_bytes=1 << 30)  # a workspace that is large enough and misaligned
    assert rc == 1 and b"workspace must be 16-byte aligned" in err


# ------------------------------------------------------------------------------------------------
# generate_pool's host side
# ------------------------------------------------------------------------------------------------
def test_generate_pool_refuses_a_bad_admit_group_without_a_device():
    from tcavt_amd import config, model
    from tcavt_amd.weights import make_weights

    cfg = config.tiny()
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(make_weights(cfg, 0)).eval()
    ids = torch.zeros(2, 4, dtype=torch.int64)
    mask = torch.ones_like(ids)
    vis = torch.zeros(2, 1, 8)
    for slots, G in ((4, 0), (4, 5), (4, -1), (1, 2)):
        with pytest.raises(ValueError, match=r"admit_group must be in \[1, slots"):
            m.mllm.generate_pool(vis, ids, mask, slots=slots, admit_group=G)
    out = m.mllm.generate_pool(vis[:0], ids[:0], mask[:0], max_new_tokens=5, slots=4, admit_group=4)  # legal, and nothing to do
    assert tuple(out.shape) == (0, 5) and m.mllm.pool_stats["groups"] == []


def test_grouped_call_sequence_against_a_stub_library(monkeypatch):
    """The host side of the grouped admission end to end on the CPU, as test_generate_pool_call_sequence_against_a_stub_library does
    for admit_group = 1: the stub plays the device's part in the slot bookkeeping from the STAGING buffers the launch names, so
    the staging, every wrapper's host guard and the loop are exercised with the real shapes."""
    from tcavt_amd import capi, config, model, ops
    from tcavt_amd.weights import make_weights

    calls, passes = [], []
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)

    class Stub:
        def __getattr__(self, name):
            if not name.startswith("tcavt_"):
                raise AttributeError(name)

            def fn(*args):
                calls.append(name)
                if name == "tcavt_slot_admit_group":
                    a = args[0]._obj
                    slot, budget = ctypes.cast(a.slot, i32p), ctypes.cast(a.max_new_value, i32p)
                    rows, ids = ctypes.cast(a.out_row_value, i64p), ctypes.cast(a.prompt_ids, i64p)
                    passes.append(dict(G=a.G, S=a.S, rows=a.rows, src_lmax=a.src_lmax, kv_lmax=a.kv_lmax, n_ids=a.n_ids,
                                       slot=[slot[g] for g in range(a.G)], budget=[budget[g] for g in range(a.G)],
                                       out_row=[rows[g] for g in range(a.G)], first_id=[ids[g * a.n_ids] for g in range(a.G)]))
                    for g in range(a.G):
                        if slot[g] >= 0:
                            ctypes.cast(a.step, i32p)[slot[g]] = 0
                            ctypes.cast(a.finished, i32p)[slot[g]] = 0
                            ctypes.cast(a.max_new, i32p)[slot[g]] = budget[g]
                            ctypes.cast(a.out_row, i64p)[slot[g]] = rows[g]
                if name in ("tcavt_sample_logits_slots", "tcavt_sample_logits_rows"):
                    if name == "tcavt_sample_logits_rows":
                        m_ = ctypes.cast(args[3], i32p)
                        live = [m_[g] for g in range(args[1]) if m_[g] >= 0]
                        step, max_new, fin = (ctypes.cast(args[i], i32p) for i in (9, 10, 14))
                    else:
                        live = range(args[1])
                        step, max_new, fin = (ctypes.cast(args[i], i32p) for i in (7, 8, 12))
                    for s in live:
                        if not fin[s]:
                            step[s] += 1
                            fin[s] = int(step[s] == max_new[s])
                return 0

            return fn

    monkeypatch.setattr(ops, "lib", lambda: Stub())
    monkeypatch.setattr(ops, "stream_ptr", lambda: None)
    monkeypatch.setattr(ops, "_ALLOW_CPU", True)
    monkeypatch.setenv("TCAVT_DECODE_ROWMAJOR", "1")  # (packing the fragment-major weight copies needs a device stream)
    cfg = config.tiny()
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(make_weights(cfg, 0)).eval()
    R, Lt, S, G = 7, 6, 4, 2
    ids = torch.arange(R)[:, None] * 10 + torch.arange(Lt)[None]
    mask = torch.ones_like(ids)
    vis = torch.zeros(R, 1, cfg.vision_dim) if hasattr(cfg, "vision_dim") else torch.zeros(R, 1, 8)
    budgets = [3, 1, 6, 2, 4, 5, 2]
    for kv in ("fp16", "fp8"):
        calls.clear()
        passes.clear()
        out = m.mllm.generate_pool(vis, ids, mask, max_new_tokens=budgets, slots=S, poll_every=1, use_graph=False, pad_token_id=7, kv_cache=kv,
                                   admit_group=G)
        st = m.mllm.pool_stats
        assert tuple(out.shape) == (R, 6)
        assert len(passes) == len(st["groups"]) == 4  # 2 + 2 + 2 + the tail of one
        assert calls.count("tcavt_slot_admit_group") == calls.count("tcavt_llama_stack_forward") == calls.count("tcavt_gather_last") == 4
        assert calls.count("tcavt_sample_logits_rows") == 4 and calls.count("tcavt_slot_admit") == 0
        assert calls.count("tcavt_llama_decode_step") == calls.count("tcavt_sample_logits_slots") == st["steps"]
        for p, (reqs, slots, _) in zip(passes, st["groups"]):
            assert (p["G"], p["S"], p["rows"], p["src_lmax"], p["kv_lmax"], p["n_ids"]) == (G, S, 16 + Lt, 16 + Lt, 16 + Lt + 6, Lt)
            pad = G - len(reqs)
            assert p["slot"] == list(slots) + [-1] * pad  # a pad row is admitted nowhere ...
            want = list(reqs) + [reqs[0]] * pad  # ... and repeats the group's first request
            assert p["out_row"] == want and p["budget"] == [budgets[r] for r in want] and p["first_id"] == [10 * r for r in want]
            assert len(set(slots)) == len(slots)
        assert [r for reqs, _, _ in st["groups"] for r in reqs] == list(range(R))
        assert [a[0] for a in st["admitted"]] == list(range(R)) and sorted(a[0] for a in st["retired"]) == list(range(R))
        assert len(st["groups"][-1][0]) == 1
