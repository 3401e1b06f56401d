"""CPU-side checks of n continuations per prompt (generate_batch(num_return_sequences=n), tcavt_kv_fanout): the entry is
declared and bound, the ctypes mirror of tcavt_kv_fanout_args matches the header (compiled with the host C compiler), n = 1 is
launch for launch the call without the argument (the golden trace of tests/test_generation_trace_cpu.py), n = 3 prefills once at
B rows, fans out once and decodes at B * n rows, and illegal values are refused before any entry is called."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import generation_stub
from tests.test_lm_loss_abi_cpu import ROOT, _struct_fields

GOLDEN = os.path.join(ROOT, "tests", "golden", "generation_trace.json")
LT = 6  # generation_stub._requests


def _record(R, **kw):
    """generation_stub.record for generate_batch with keyword arguments of the test's own: -> (result, calls, workspace)."""
    with generation_stub.stubbed() as stub:
        cfg, m = generation_stub.tiny_model()
        vis, ids, mask = generation_stub._requests(cfg, R)
        res = m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, pad_token_id=7, **kw)
    bufs = [[n, list(shape), str(dt)] for ws in (m.mllm._ws, m.mllm.llama_wrapper._ws) for n, shape, dt in ws._bufs]
    return res, json.loads(json.dumps(stub.calls)), json.loads(json.dumps(bufs))


def test_entry_is_declared_and_bound():
    from tcavt_amd import capi, ops

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tcavt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tcavt_[a-z0-9_]+)\s*\(", text))
    assert "tcavt_kv_fanout" in declared and "tcavt_kv_fanout" in capi.EXPORTED_SYMBOLS
    sig = capi._SIGNATURES["tcavt_kv_fanout"]
    assert sig[0]._type_ is capi.KvFanoutArgs and sig[1] is ctypes.c_void_p and len(sig) == 2
    assert capi.lib().tcavt_abi_version() == capi.ABI_VERSION == 5  # an additive change
    assert callable(ops.kv_fanout)
    getattr(capi.lib(), "tcavt_kv_fanout")


def test_kv_fanout_args_mirror_matches_header_layout(tmp_path):
    from tcavt_amd import capi

    cls, cname = capi.KvFanoutArgs, "tcavt_kv_fanout_args"
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


@pytest.mark.parametrize("kv_cache", ["fp16", "fp8"])
def test_one_sequence_is_the_golden_trace(kv_cache):
    """num_return_sequences=1, and the keyword absent: launch for launch, buffer for buffer the trace recorded before it existed."""
    with open(GOLDEN) as f:
        want = json.load(f)[f"batch_n5/{kv_cache}"]
    for kw in (dict(num_return_sequences=1), dict()):
        res, calls, bufs = _record(3, max_new_tokens=5, kv_cache=kv_cache, **kw)
        assert tuple(res.shape) == (3, 5)
        assert [c[0] for c in calls] == [c[0] for c in want["calls"]]
        assert calls == want["calls"]
        assert bufs == want["workspace"]


@pytest.mark.parametrize("kv_cache", ["fp16", "fp8"])
def test_three_sequences_prefill_once_fan_out_once_and_decode_at_nine_rows(kv_cache):
    res, calls, bufs = _record(3, max_new_tokens=5, kv_cache=kv_cache, num_return_sequences=3)
    assert tuple(res.shape) == (9, 5)
    by = {}
    for name, scalars in calls:
        by.setdefault(name, []).append(scalars)
    # one decoder pass, at the prompts' 3 rows over 16 + Lt positions
    (stack,) = by["tcavt_llama_stack_forward"]
    assert stack[0]["B"] == 3 and stack[0]["L"] == 16 + LT
    # one fan-out: 3 prompts x 3, the whole source, into a cache of 16 + Lt + 5 rows
    (fan,) = by["tcavt_kv_fanout"]
    f = fan[0]
    assert (f["B"], f["n"], f["rows"], f["src_lmax"], f["kv_lmax"]) == (3, 3, 16 + LT, 16 + LT, 16 + LT + 5)
    assert (f["n_ids"], f["hist_cap"], f["n_image"]) == (LT, LT + 5, 16)
    names = [c[0] for c in calls]
    assert names.index("tcavt_llama_stack_forward") < names.index("tcavt_kv_fanout") < min(
        i for i, n in enumerate(names) if n.startswith("tcavt_sample_"))
    # every decode step and every sampler call at 9 rows
    steps = by["tcavt_llama_decode_step"]
    assert len(steps) == 4 and all(s[0]["B"] == 9 for s in steps)
    samplers = [(n, s) for n, s in calls if n.startswith("tcavt_sample_")]
    assert len(samplers) == 5 and all(n == "tcavt_sample_logits" and s[0] == 9 for n, s in samplers)
    # the prefill's buffers under its own tag, the decode batch's under "gen"
    shapes = {n: s for n, s, _ in bufs}
    assert shapes["gen.src.logits"][0] == 3 and shapes["gen.logits"][0] == 9 and shapes["gen.src.kvlen"] == [3]
    if kv_cache == "fp16":
        assert shapes["gen.src.kc"][1:3] == [3, 16 + LT] and shapes["gen.kc"][1:3] == [9, 16 + LT + 5]
    else:
        assert shapes["gen.src.kv8.kc"][1:4:2] == [3, 16 + LT] and shapes["gen.kv8.kc"][1:4:2] == [9, 16 + LT + 5]


@pytest.mark.parametrize("kv_cache", ["fp16", "fp8"])
def test_three_sequences_with_rules_return_nine_records(kv_cache):
    (out, info), calls, _ = _record(3, max_new_tokens=5, kv_cache=kv_cache, num_return_sequences=3, **generation_stub.RULES)
    assert tuple(out.shape) == (9, 5)
    assert info["finish_reason"].shape == info["n_generated"].shape == (9,)
    samplers = [s for n, s in calls if n == "tcavt_sample_tokens"]
    assert len(samplers) == 5 and all(s[0]["rows"] == 9 and s[0]["n_state"] == 9 for s in samplers)
    assert not any(n in ("tcavt_sample_logits", "tcavt_sample_logits_slots", "tcavt_sample_logits_rows") for n, _ in calls)


@pytest.mark.parametrize("bad", [0, -1, 2.5, True, "2", None])
def test_illegal_counts_are_refused_before_any_entry(bad):
    with generation_stub.stubbed() as stub:
        cfg, m = generation_stub.tiny_model()
        vis, ids, mask = generation_stub._requests(cfg, 3)
        with pytest.raises(ValueError, match="num_return_sequences"):
            m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, max_new_tokens=5, num_return_sequences=bad)
    assert stub.calls == []


def test_fp8_weights_limit_applies_to_the_decode_rows():
    with generation_stub.stubbed() as stub:
        cfg, m = generation_stub.tiny_model()
        vis, ids, mask = generation_stub._requests(cfg, 11)
        with pytest.raises(ValueError, match="<= 32"):  # B * n = 33
            m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, max_new_tokens=5, num_return_sequences=3,
                                  decode_weights="fp8")
    assert stub.calls == []


def _good_args(capi):
    a = capi.KvFanoutArgs()
    for n in ("src_k", "src_v", "dst_k", "dst_v", "prompt_ids", "kv_len", "logits_src", "logits_dst", "history", "hist_len", "pos",
              "finished"):
        setattr(a, n, 256)  # (never dereferenced: every call below is refused first)
    a.n_layers, a.B, a.n, a.rows, a.src_lmax, a.kv_lmax, a.nkv, a.dtype16 = 2, 3, 3, 5, 7, 11, 2, capi.F16
    a.n_ids, a.hist_cap, a.n_image, a.V = 4, 9, 2, 48
    return a


def test_argument_errors_are_reported_without_a_device():
    from tcavt_amd import capi

    lib = capi.lib()

    def refused(a, msg):
        rc = lib.tcavt_kv_fanout(ctypes.byref(a) if a is not None else None, None)
        err = lib.tcavt_last_error()
        assert rc != 0 and msg in err, (rc, err)

    refused(None, b"args is a null pointer")
    for field in ("prompt_ids", "kv_len", "logits_src", "logits_dst", "history", "hist_len", "pos", "finished"):
        a = _good_args(capi)
        setattr(a, field, None)
        refused(a, field.encode() + b" is a null pointer")
    a = _good_args(capi)
    a.dst_v = None
    refused(a, b"src_k, src_v, dst_k and dst_v come together")
    a = _good_args(capi)
    a.src_k_codes = 256
    refused(a, b"exclude each other")
    a = _good_args(capi)
    a.src_k = a.src_v = a.dst_k = a.dst_v = None
    refused(a, b"null pointer (src_k / src_v / dst_k / dst_v, or the eight kv8 planes)")
    for field, val, msg in (("rows", 0, b"rows = 0"), ("rows", 8, b"rows = 8"), ("B", 0, b"B = 0"), ("n", 0, b"n = 0"), ("n", -2, b"n = -2"),
                            ("n_ids", -1, b"n_ids = -1"), ("n_ids", 10, b"n_ids = 10"), ("V", 0, b"V = 0"), ("dst_k", 264, b"16-byte aligned"),
                            ("logits_dst", 260, b"logits_src and logits_dst must be 16-byte aligned"), ("dtype16", capi.F32, b"dtype16")):
        a = _good_args(capi)
        setattr(a, field, val)
        refused(a, msg)
    a = _good_args(capi)
    a.kv_lmax = 4  # rows = 5 > min(src_lmax, kv_lmax)
    refused(a, b"rows = 5")
