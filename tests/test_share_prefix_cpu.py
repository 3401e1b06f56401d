"""CPU-side checks of generate_batch(share_prefix=True): the three entries (tcavt_attn_decode_shared, tcavt_state_fanout,
tcavt_llama_decode_step_shared) are declared, exported and bound; the ctypes mirrors of tcavt_kv_prefix and
tcavt_state_fanout_args match the header (compiled with the host C compiler) and tcavt_decode_args is what it was; share_prefix
False or absent is launch for launch the golden trace; True prefills once at the prompts' rows, runs one state fan-out and no
cache fan-out, and decodes at B * n rows on a suffix cache of max_new_tokens - 1 rows; illegal values are refused before any
entry is called, and the C entries refuse bad arguments without a device."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import generation_stub
from tests.test_lm_loss_abi_cpu import ROOT, _struct_fields
from tests.test_nsamples_cpu import GOLDEN, LT, _record

NEW = ("tcavt_attn_decode_shared", "tcavt_state_fanout", "tcavt_llama_decode_step_shared")


def test_entries_are_declared_exported_and_bound():
    from tcavt_amd import capi, ops

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tcavt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tcavt_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in capi.EXPORTED_SYMBOLS
        getattr(capi.lib(), name)
    sig = capi._SIGNATURES["tcavt_state_fanout"]
    assert sig[0]._type_ is capi.StateFanoutArgs and sig[1] is ctypes.c_void_p and len(sig) == 2
    sig = capi._SIGNATURES["tcavt_llama_decode_step_shared"]
    assert sig[0]._type_ is capi.DecodeArgs and sig[1]._type_ is capi.KvPrefix and sig[2] is ctypes.c_void_p and len(sig) == 3
    assert len(capi._SIGNATURES["tcavt_attn_decode_shared"]) == 18
    assert capi.lib().tcavt_abi_version() == capi.ABI_VERSION == 5  # an additive change
    assert callable(ops.attn_decode_shared) and callable(ops.state_fanout) and callable(ops.llama_decode_step_shared)
    # the prefix travels next to tcavt_decode_args, whose fields -- the integers the golden trace records -- are what they were
    assert "prefix" not in [f[0] for f in capi.DecodeArgs._fields_]
    m = re.search(r"#define\s+TCAVT_ATTN_DECODE_SHARED_MAX_SUFFIX\s+(\d+)", text)
    assert m and int(m.group(1)) == 1152


@pytest.mark.parametrize("cname,mirror", [("tcavt_kv_prefix", "KvPrefix"), ("tcavt_state_fanout_args", "StateFanoutArgs")])
def test_mirror_matches_header_layout(tmp_path, cname, mirror):
    from tcavt_amd import capi

    cls = getattr(capi, mirror)
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


def test_state_fanout_args_are_the_non_cache_fields_of_kv_fanout_args():
    kv = _struct_fields("tcavt_kv_fanout_args")
    cache = [n for n in kv if n.startswith(("src_", "dst_"))] + ["n_layers", "rows", "src_lmax", "kv_lmax", "nkv", "dtype16"]
    assert _struct_fields("tcavt_state_fanout_args") == [n for n in kv if n not in cache]


@pytest.mark.parametrize("kv_cache", ["fp16", "fp8"])
def test_share_prefix_off_is_the_golden_trace(kv_cache):
    with open(GOLDEN) as f:
        want = json.load(f)[f"batch_n5/{kv_cache}"]
    for kw in (dict(share_prefix=False), dict(num_return_sequences=1, share_prefix=False), dict()):
        res, calls, bufs = _record(3, max_new_tokens=5, kv_cache=kv_cache, **kw)
        assert tuple(res.shape) == (3, 5)
        assert calls == want["calls"]
        assert bufs == want["workspace"]


def test_off_with_three_sequences_is_the_call_without_the_keyword():
    a = _record(3, max_new_tokens=5, num_return_sequences=3)
    b = _record(3, max_new_tokens=5, num_return_sequences=3, share_prefix=False)
    assert a[1] == b[1] and a[2] == b[2]


@pytest.mark.parametrize("n", [3, 1])
def test_shared_prefills_once_fans_out_the_state_and_decodes_on_a_suffix_cache(n):
    res, calls, bufs = _record(3, max_new_tokens=5, num_return_sequences=n, share_prefix=True)
    R = 3 * n
    assert tuple(res.shape) == (R, 5)
    by = {}
    for name, scalars in calls:
        by.setdefault(name, []).append(scalars)
    # one decoder pass, at the prompts' 3 rows over 16 + Lt positions
    (stack,) = by["tcavt_llama_stack_forward"]
    assert stack[0]["B"] == 3 and stack[0]["L"] == 16 + LT
    # no cache fan-out; exactly one state fan-out: 3 prompts x n
    assert "tcavt_kv_fanout" not in by and "tcavt_llama_decode_step" not in by
    (fan,) = by["tcavt_state_fanout"]
    f = fan[0]
    assert (f["B"], f["n"]) == (3, n)
    assert (f["n_ids"], f["hist_cap"], f["n_image"]) == (LT, LT + 5, 16)
    names = [c[0] for c in calls]
    assert names.index("tcavt_llama_stack_forward") < names.index("tcavt_state_fanout") < min(
        i for i, nm in enumerate(names) if nm.startswith("tcavt_sample_"))
    # every decode step at R rows on 4 suffix rows, the prefix struct next to it; RoPE tables over prompt + suffix
    steps = by["tcavt_llama_decode_step_shared"]
    assert len(steps) == 4
    for args, prefix in steps:
        assert args["B"] == R and args["kv_lmax"] == 4 and args["rope_L"] >= 16 + LT + 4
        assert prefix == {"n": n, "lmax": 16 + LT}
    samplers = [(nm, s) for nm, s in calls if nm.startswith("tcavt_sample_")]
    assert len(samplers) == 5 and all(nm == "tcavt_sample_logits" and s[0] == R for nm, s in samplers)
    # the prefill's buffers under its own tag, the suffix cache under gen.sfx, and no cache of Lmax rows
    shapes = {nm: s for nm, s, _ in bufs}
    assert shapes["gen.src.kc"][1:3] == [3, 16 + LT] and shapes["gen.src.vc"][1:3] == [3, 16 + LT]
    assert shapes["gen.sfx.kc"][1:3] == [R, 4] and shapes["gen.sfx.vc"][1:3] == [R, 4]
    assert "gen.kc" not in shapes and "gen.vc" not in shapes and not any(nm.startswith("gen.kv8") for nm in shapes)
    assert shapes["gen.src.logits"][0] == 3 and shapes["gen.logits"][0] == R


def test_one_new_token_needs_no_decode_step():
    res, calls, bufs = _record(3, max_new_tokens=1, num_return_sequences=3, share_prefix=True)
    assert tuple(res.shape) == (9, 1)
    names = [c[0] for c in calls]
    assert names.count("tcavt_state_fanout") == 1 and "tcavt_llama_decode_step_shared" not in names
    assert {nm: s for nm, s, _ in bufs}["gen.sfx.kc"][1:3] == [9, 1]


def test_shared_with_rules_returns_nine_records():
    (out, info), calls, _ = _record(3, max_new_tokens=5, num_return_sequences=3, share_prefix=True, **generation_stub.RULES)
    assert tuple(out.shape) == (9, 5)
    assert info["finish_reason"].shape == info["n_generated"].shape == (9,)
    samplers = [s for nm, s in calls if nm == "tcavt_sample_tokens"]
    assert len(samplers) == 5 and all(s[0]["rows"] == 9 and s[0]["n_state"] == 9 for s in samplers)


@pytest.mark.parametrize("kw,msg", [(dict(share_prefix=1), "share_prefix must be a bool"), (dict(share_prefix="yes"), "share_prefix must be a bool"),
                                    (dict(share_prefix=None), "share_prefix must be a bool"),
                                    (dict(share_prefix=True, kv_cache="fp8"), "kv_cache='fp8'"),
                                    (dict(share_prefix=True, kv_cache="fp8", num_return_sequences=3), "kv_cache='fp8'")])
def test_illegal_values_are_refused_before_any_entry(kw, msg):
    with generation_stub.stubbed() as stub:
        cfg, m = generation_stub.tiny_model()
        vis, ids, mask = generation_stub._requests(cfg, 3)
        with pytest.raises(ValueError, match=msg):
            m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, max_new_tokens=5, **kw)
    assert stub.calls == []


def test_fp8_weights_limit_applies_to_the_decode_rows():
    with generation_stub.stubbed() as stub:
        cfg, m = generation_stub.tiny_model()
        vis, ids, mask = generation_stub._requests(cfg, 11)
        with pytest.raises(ValueError, match="<= 32"):  # B * n = 33
            m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, max_new_tokens=5, num_return_sequences=3, share_prefix=True,
                                  decode_weights="fp8")
    assert stub.calls == []


def test_argument_errors_are_reported_without_a_device():
    from tcavt_amd import capi

    lib = capi.lib()

    def fan(**kw):
        a = capi.StateFanoutArgs()
        for n in ("prompt_ids", "kv_len", "logits_src", "logits_dst", "history", "hist_len", "pos", "finished"):
            setattr(a, n, 256)  # (never dereferenced: every call below is refused first)
        a.B, a.n, a.n_ids, a.hist_cap, a.n_image, a.V = 3, 3, 4, 9, 2, 48
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(rc, msg):
        err = lib.tcavt_last_error()
        assert rc != 0 and msg in err, (rc, err)

    refused(lib.tcavt_state_fanout(None, None), b"state_fanout: args is a null pointer")
    for field in ("prompt_ids", "kv_len", "logits_src", "logits_dst", "history", "hist_len", "pos", "finished"):
        refused(lib.tcavt_state_fanout(ctypes.byref(fan(**{field: None})), None), b"state_fanout: " + field.encode() + b" is a null pointer")
    for field, val, msg in (("B", 0, b"B = 0"), ("n", 0, b"n = 0"), ("n", -2, b"n = -2"), ("n_ids", -1, b"n_ids = -1"), ("n_ids", 10, b"n_ids = 10"),
                            ("V", 0, b"V = 0"), ("n_image", -1, b"n_image = -1"), ("hist_cap", 0, b"hist_cap = 0"),
                            ("logits_dst", 260, b"logits_src and logits_dst must be 16-byte aligned")):
        refused(lib.tcavt_state_fanout(ctypes.byref(fan(**{field: val})), None), msg)

    def att(qkv=256, pk=256, pv=256, plen=256, sk=256, sv=256, pos=256, out=256, B=2, n=2, nq=4, nkv=1, plmax=8, slmax=4, dt=None, layout=0):
        return lib.tcavt_attn_decode_shared(qkv, pk, pv, plen, sk, sv, pos, out, B, n, nq, nkv, plmax, slmax, 0.125,
                                            capi.F16 if dt is None else dt, layout, None)

    for nm in ("qkv", "pk", "pv", "plen", "sk", "sv", "pos", "out"):
        refused(att(**{nm: None}), b"attn_decode_shared: null pointer")
    for kw, msg in ((dict(dt=capi.F32), b"dtype16"), (dict(nq=5, nkv=2), b"bad shape"), (dict(nq=9), b"bad shape"), (dict(B=0), b"bad shape"),
                    (dict(n=0), b"n = 0"), (dict(plmax=0), b"prefix_lmax"), (dict(slmax=0), b"suffix_lmax must be >= 1"),
                    (dict(slmax=1153), b"exceeds TCAVT_ATTN_DECODE_SHARED_MAX_SUFFIX"), (dict(layout=3), b"out_layout"), (dict(layout=1, B=11, n=3), b"out_layout"),
                    (dict(layout=2, B=3, n=3), b"out_layout"), (dict(layout=1, nq=6, nkv=2), b"out_layout"), (dict(sk=264), b"16-byte aligned"),
                    (dict(pk=264), b"16-byte aligned"), (dict(out=264), b"16-byte aligned")):
        refused(att(**kw), b"attn_decode_shared: ")
        refused(att(**kw), msg)

    refused(lib.tcavt_llama_decode_step_shared(ctypes.byref(capi.DecodeArgs()), None, None), b"llama_decode_step_shared: prefix is a null pointer")


def test_ops_wrappers_guard_the_extents_before_the_entry():
    import torch

    from tcavt_amd import capi, ops

    with generation_stub.stubbed() as stub:
        B, n, nq, nkv, pl, sl = 2, 3, 4, 1, 8, 4
        R = B * n
        h = lambda *s: torch.zeros(*s, dtype=torch.float16)
        i32 = lambda k: torch.zeros(k, dtype=torch.int32)
        good = dict(qkv=h(R, (nq + 2 * nkv) * 64), prefix_k=h(B, pl, nkv * 64), prefix_v=h(B, pl, nkv * 64), prefix_len=i32(B),
                    suffix_k=h(R, sl, nkv * 64), suffix_v=h(R, sl, nkv * 64), pos=i32(R), out=h(R, nq * 64))
        ops.attn_decode_shared(**good, B=B, n=n, nq=nq, nkv=nkv, prefix_lmax=pl, suffix_lmax=sl, scale=0.125)
        assert [c[0] for c in stub.calls] == ["tcavt_attn_decode_shared"]
        for name, short in (("suffix_k", h(R, sl - 1, nkv * 64)), ("prefix_v", h(B, pl - 1, nkv * 64)), ("pos", i32(R - 1)),
                            ("prefix_len", i32(B - 1)), ("out", h(R - 1, nq * 64)), ("qkv", h(R - 1, (nq + 2 * nkv) * 64))):
            with pytest.raises(capi.TcavtError, match="kernel needs"):
                ops.attn_decode_shared(**dict(good, **{name: short}), B=B, n=n, nq=nq, nkv=nkv, prefix_lmax=pl, suffix_lmax=sl, scale=0.125)
        with pytest.raises(capi.TcavtError, match="expected"):
            ops.attn_decode_shared(**dict(good, suffix_v=good["suffix_v"].to(torch.bfloat16)), B=B, n=n, nq=nq, nkv=nkv, prefix_lmax=pl,
                                   suffix_lmax=sl, scale=0.125)
        V, cap, n_ids = 48, 9, 4
        st = dict(prompt_ids=torch.zeros(B, n_ids, dtype=torch.int64), kv_len=i32(B), logits_src=torch.zeros(B, V),
                  logits_dst=torch.zeros(R, V), history=torch.zeros(R, cap, dtype=torch.int64), hist_len=i32(R), pos=i32(R), finished=i32(R))
        ops.state_fanout(n, st["prompt_ids"], st["kv_len"], 16, st["logits_src"], st["logits_dst"], st["history"], st["hist_len"], st["pos"],
                         st["finished"])
        assert stub.calls[-1][0] == "tcavt_state_fanout" and stub.calls[-1][1][0] == dict(B=B, n=n, n_ids=n_ids, hist_cap=cap, n_image=16, V=V)
        with pytest.raises(capi.TcavtError, match="kernel needs"):
            ops.state_fanout(n, st["prompt_ids"], st["kv_len"], 16, st["logits_src"], st["logits_dst"], st["history"], st["hist_len"],
                             i32(R - 1), st["finished"])
        with pytest.raises(capi.TcavtError, match="history"):
            ops.state_fanout(n, st["prompt_ids"], st["kv_len"], 16, st["logits_src"], st["logits_dst"], st["history"][:-1], st["hist_len"],
                             st["pos"], st["finished"])
        assert len(stub.calls) == 2  # nothing reached an entry after a guard raised
