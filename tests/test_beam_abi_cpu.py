"""The boundary of beam search without a GPU: tcavt_beam_select / tcavt_beam_reorder refuse every bad argument before a launch and
name it (tcavt_last_error); generate_batch raises its ValueErrors before anything touches a device; the ctypes mirrors of the two
argument structs match the header (the method of tests/test_abi_cpu.py)."""
import ctypes
import dataclasses
import math

import pytest

import generation_stub
from test_abi_cpu import test_struct_mirrors_match_header_layout as _layout_check

FAKE = 4096  # a 16-byte aligned address that is never dereferenced: every call below is refused before the launch
SELECT_PTRS = ("logits", "history", "hist_len", "run_score", "live", "fin_tokens", "fin_score", "fin_flag", "fin_len", "unsat", "done",
               "cur_tok", "pos", "finished", "step", "prefix_len", "len_pow", "parent", "plan", "workspace")
REORDER_PTRS = ("parent", "plan", "cur_tok", "history", "hist_len", "pos", "step", "suffix_k", "suffix_v")


def _select_args(capi, **over):
    a = capi.BeamArgs()
    for nm in SELECT_PTRS:
        setattr(a, nm, FAKE)
    a.R, a.n, a.V, a.N, a.hist_cap = 8, 4, 48, 6, 16
    a.repetition_penalty, a.pad_token_id, a.eos_token_id = 1.2, 0, 5
    a.workspace_bytes = capi.lib().tcavt_beam_workspace_bytes(8)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _reorder_args(capi, **over):
    a = capi.BeamReorderArgs()
    for nm in REORDER_PTRS:
        setattr(a, nm, FAKE)
    a.R, a.n, a.hist_cap, a.n_layers, a.nkv, a.suffix_lmax = 8, 4, 16, 2, 1, 5
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _refused(capi, fn, args, *words):
    rc = fn(ctypes.byref(args), None)
    msg = capi.lib().tcavt_last_error().decode()
    assert rc == 1, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_workspace_query():
    from tcavt_amd import capi

    q = capi.lib().tcavt_beam_workspace_bytes
    assert q(0) == 0 and q(-3) == 0
    assert 0 < q(2) < q(32) and q(32) % 16 == 0


def test_beam_select_refuses_bad_arguments_before_a_launch():
    from tcavt_amd import capi

    sel = capi.lib().tcavt_beam_select
    assert sel(None, None) == 1 and b"null" in capi.lib().tcavt_last_error()
    for nm in SELECT_PTRS:
        _refused(capi, sel, _select_args(capi, **{nm: None}), "beam_select", nm, "null pointer")
    for n in (0, 1, 17, 64):
        _refused(capi, sel, _select_args(capi, n=n, R=8 * max(n, 1)), "n =", "[2, 16]")
    _refused(capi, sel, _select_args(capi, R=9), "R = 9", "multiple of n")
    _refused(capi, sel, _select_args(capi, R=0), "R = 0")
    _refused(capi, sel, _select_args(capi, V=7), "V = 7", ">= 2 n")
    _refused(capi, sel, _select_args(capi, V=262145), "V = 262145")
    _refused(capi, sel, _select_args(capi, N=0), "N = 0")
    _refused(capi, sel, _select_args(capi, hist_cap=0), "hist_cap")
    _refused(capi, sel, _select_args(capi, no_repeat_ngram_size=-1), "no_repeat_ngram_size")
    _refused(capi, sel, _select_args(capi, repetition_penalty=0.0), "repetition_penalty")
    _refused(capi, sel, _select_args(capi, workspace_bytes=capi.lib().tcavt_beam_workspace_bytes(8) - 1), "workspace_bytes", "needs")
    _refused(capi, sel, _select_args(capi, workspace=FAKE + 8), "workspace", "16-byte aligned")


def test_beam_reorder_refuses_bad_arguments_before_a_launch():
    from tcavt_amd import capi

    reo = capi.lib().tcavt_beam_reorder
    assert reo(None, None) == 1 and b"null" in capi.lib().tcavt_last_error()
    for nm in REORDER_PTRS:
        _refused(capi, reo, _reorder_args(capi, **{nm: None}), "beam_reorder", nm, "null pointer")
    for n in (1, 17):
        _refused(capi, reo, _reorder_args(capi, n=n, R=8 * n), "n =", "[2, 16]")
    _refused(capi, reo, _reorder_args(capi, R=10), "R = 10", "multiple of n")
    for nm in ("n_layers", "nkv", "suffix_lmax"):
        _refused(capi, reo, _reorder_args(capi, **{nm: 0}), "bad shape")
    _refused(capi, reo, _reorder_args(capi, hist_cap=0), "hist_cap")
    for nm in ("suffix_k", "suffix_v"):
        _refused(capi, reo, _reorder_args(capi, **{nm: FAKE + 8}), "16-byte aligned")


@pytest.mark.parametrize("cname,mirror", [("tcavt_beam_args", "BeamArgs"), ("tcavt_beam_reorder_args", "BeamReorderArgs")])
def test_beam_struct_mirrors_match_header_layout(cname, mirror, tmp_path):
    _layout_check(cname, mirror, tmp_path)


BAD = [(dict(do_sample=True), "do_sample"), (dict(kv_cache="fp8"), "kv_cache"), (dict(stop_token_ids=[3]), "stop_token_ids"),
       (dict(stop_sequences=[[3, 4]]), "stop_sequences"), (dict(min_new_tokens=2, eos_token_id=5), "min_new_tokens"),
       (dict(return_logprobs=True), "return_logprobs"), (dict(early_stopping="never"), "early_stopping"),
       (dict(num_beams=2.0), "num_beams"), (dict(num_beams=True), "num_beams"), (dict(num_beams=0), "num_beams"),
       (dict(num_beams=17), "num_beams"), (dict(length_penalty=math.inf), "length_penalty"),
       (dict(length_penalty=math.nan), "length_penalty"), (dict(num_return_sequences=4), "num_return_sequences"),
       (dict(num_return_sequences=0), "num_return_sequences")]


@pytest.mark.parametrize("kw,name", BAD)
def test_generate_batch_refuses_before_a_device_is_touched(kw, name):
    with generation_stub.stubbed() as stub:
        cfg, m = generation_stub.tiny_model()
        vis, ids, mask = generation_stub._requests(cfg, 2)
        args = dict(dict(input_ids=ids, attention_mask=mask, max_new_tokens=4, do_sample=False, num_beams=3), **kw)
        with pytest.raises(ValueError, match=name):
            m.mllm.generate_batch(vis, **args)
        assert stub.calls == []


def test_generate_batch_refuses_a_vocabulary_below_two_beams_each(monkeypatch):
    with generation_stub.stubbed() as stub:
        cfg, m = generation_stub.tiny_model()
        vis, ids, mask = generation_stub._requests(cfg, 2)
        n = 16
        shape = m.mllm.llama_wrapper.shape
        small = dataclasses.replace(shape, vocab=2 * n - 1)
        monkeypatch.setattr(m.mllm.llama_wrapper, "shape", small)
        with pytest.raises(ValueError, match="num_beams"):
            m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, max_new_tokens=4, do_sample=False, num_beams=n)
        assert stub.calls == []


def test_generate_pool_does_not_take_the_arguments():
    import inspect

    from tcavt_amd import mllm

    pool = inspect.signature(mllm.LlamaMultiModal.generate_pool).parameters
    assert not {"num_beams", "length_penalty", "early_stopping"} & set(pool)
    batch = list(inspect.signature(mllm.LlamaMultiModal.generate_batch).parameters)
    assert batch[-4:] == ["return_logprobs", "num_beams", "length_penalty", "early_stopping"]
