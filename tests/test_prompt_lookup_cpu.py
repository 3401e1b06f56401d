"""CPU side of prompt-lookup speculative decoding (generate_batch(prompt_lookup_num_tokens=k)).

- prompt_lookup_ref.draft -- the reference the draft kernel is tested against -- equals HF's
  PromptLookupCandidateGenerator(num_output_tokens=k, max_matching_ngram_size=m, max_length=10**9) row by row: random ids over
  vocabularies of 4 .. 8 (matches are common), lengths 1 .. 40, k 1 .. 7, m 1 .. 8, and the no-match, self-match-only and
  match-at-the-very-end cases.
- prompt_lookup_ref.speculative returns prompt_lookup_ref.sequential's tokens for every draft source (prompt lookup, always
  wrong, always right, random), commits exactly accepted + 1 tokens per step, and with the always-right source needs
  ceil((N - 1) / (k + 1)) steps.
- Argument errors of generate_batch are raised before a device is touched (the stub library records no call).
- The four new symbols are declared in the header and bound in capi; the struct mirror matches the header's layout.
- The launch sequence and the workspace buffers of a call with k set are pinned (tests/golden/prompt_lookup_trace.json,
  recorded with ``python tests/prompt_lookup_stub.py``); k = None stays pinned by test_generation_trace_cpu.py.
"""
import ctypes
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

import generation_stub
import prompt_lookup_ref as R
import prompt_lookup_stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "prompt_lookup_trace.json")
NEW = ("tcavt_ngram_draft", "tcavt_attn_decode_multi", "tcavt_llama_decode_step_multi", "tcavt_spec_verify")


# ---------------------------------------------------------------------------------------------------------------------------
# the draft rule

def _hf(hist, k, m):
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator

    gen = PromptLookupCandidateGenerator(num_output_tokens=k, max_matching_ngram_size=m, max_length=10 ** 9)
    ids = torch.tensor([hist], dtype=torch.int64)
    cand, _ = gen.get_candidates(ids)
    assert cand[0, :len(hist)].tolist() == list(hist)
    return cand[0, len(hist):].tolist()


def test_draft_reference_equals_hf_on_random_histories():
    rng = random.Random(0)
    n_match = 0
    for case in range(600):
        V, L, k, m = rng.randint(4, 8), rng.randint(1, 40), rng.randint(1, 7), rng.randint(1, 8)
        hist = [rng.randrange(V) for _ in range(L)]
        want = _hf(hist, k, m)
        assert R.draft(hist, k, m) == want, (hist, k, m)
        n_match += bool(want)
    assert n_match > 300  # matches are common at these vocabularies


@pytest.mark.parametrize("hist,k,m,want", [
    ([1, 2, 3, 4, 5], 3, 2, []),                    # no match
    ([7], 3, 2, []),                                # length 1: no n-gram at all
    ([1, 2, 3, 9, 9], 3, 1, [9]),                   # n = 1 matches the id right before the end: its continuation is the last id
    ([5, 6, 7, 8], 2, 4, []),                       # the only window that equals the tail is the tail itself
    ([4, 4], 5, 2, [4]),                            # match at the very end: one id behind the window, cut at len
    ([1, 2, 3, 1, 2], 7, 2, [3, 1, 2]),             # cut at the end of the history
    ([1, 2, 8, 1, 2, 9, 1, 2], 1, 2, [8]),          # the earliest of two matches
    ([3, 1, 2, 0, 2], 2, 2, [0, 2]),                # no 2-gram match: falls back to n = 1
    ([-5, 2 ** 40, 6, -5, 2 ** 40], 2, 2, [6, -5]),  # ids outside [0, 2^31)
])
def test_draft_reference_edge_cases(hist, k, m, want):
    assert R.draft(hist, k, m) == want
    if all(0 <= t for t in hist):
        assert _hf(hist, k, m) == want


def test_draft_rows_layout():
    hist = np.array([[1, 2, 3, 1, 2, 0, 0], [9, 9, 9, 9, 0, 0, 0]], np.int64)
    nd, cur, pos = R.draft_rows(hist, [5, 4], [2, 9], [20, 30], [0, 1], 3, 2, pad=77)
    assert nd.tolist() == [3, 0]  # (a finished row drafts nothing)
    assert cur.tolist() == [2, 3, 1, 2, 9, 77, 77, 77] and pos.tolist() == [20, 21, 22, 23, 30, 31, 32, 33]


# ---------------------------------------------------------------------------------------------------------------------------
# the speculative loop

def _next_token(seed, V):
    def f(hist, step):
        h = hash((seed, step, tuple(hist[-3:]), len(hist))) & 0xFFFF
        return hist[h % len(hist)] if h % 3 else h % V  # copies from the history two times in three: drafts do match
    return f


@pytest.mark.parametrize("k", [1, 3, 7])
def test_speculative_loop_returns_the_sequential_tokens(k):
    rng = random.Random(k)
    for case in range(40):
        V, N = rng.randint(4, 9), rng.randint(1, 30)
        prompt = [rng.randrange(V) for _ in range(rng.randint(1, 12))]
        nt = _next_token(case, V)
        ends = (V - 1,) if case % 2 else ()
        want = R.sequential(nt, prompt, N, ends)

        def right(hist, k_, _w=want, _p=len(prompt)):
            return _w[len(hist) - _p:len(hist) - _p + k_]

        sources = dict(lookup=lambda h, k_: R.draft(h, k_, 2), wrong=lambda h, k_: [V + 5] * k_, right=right,
                       random=lambda h, k_: [rng.randrange(V) for _ in range(rng.randint(0, k_))], none=lambda h, k_: [])
        for name, src in sources.items():
            got, log = R.speculative(nt, prompt, N, src, k, ends)
            assert got == want, (name, case)
            assert all(c == a + 1 and a <= d <= k for d, a, c in log), (name, log)
            assert 1 + sum(c for _, _, c in log) == len(want)
            if name in ("wrong", "none"):
                assert all(a == 0 for _, a, _ in log) and len(log) == len(want) - 1  # the plain step count
            if name == "right" and not ends:
                assert len(log) == -(-(N - 1) // (k + 1))


# ---------------------------------------------------------------------------------------------------------------------------
# the boundary

def test_new_symbols_are_declared_and_bound():
    from tcavt_amd import capi

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tcavt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tcavt_[a-z0-9_]+)\s*\(", text))
    handle = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in declared and name in capi.EXPORTED_SYMBOLS and hasattr(handle, name), name
    assert capi.lib().tcavt_abi_version() == capi.ABI_VERSION == 5  # an additive change


def test_spec_verify_args_mirror_matches_header(tmp_path):
    from tcavt_amd import capi

    names = [f[0] for f in capi.SpecVerifyArgs._fields_]
    assert names == ["sample", "n_draft", "cur_rows", "slot_of_row", "drafted", "accepted", "S", "T"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tcavt.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(tcavt_spec_verify_args));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(tcavt_spec_verify_args, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(capi.SpecVerifyArgs)
    assert out[1:] == [getattr(capi.SpecVerifyArgs, n).offset for n in names]


def test_entries_refuse_bad_arguments_before_any_launch():
    from tcavt_amd import capi

    lib = capi.lib()
    err = lambda: lib.tcavt_last_error().decode()
    p = 64  # (fake, 16-byte aligned, never dereferenced)
    assert lib.tcavt_ngram_draft(None, 8, p, p, p, p, 1, 3, 2, 0, p, p, p, None) == 1 and "history" in err()
    assert lib.tcavt_ngram_draft(p, 8, p, p, p, p, 1, 0, 2, 0, p, p, p, None) == 1 and "k = 0" in err()
    assert lib.tcavt_ngram_draft(p, 8, p, p, p, p, 1, 256, 2, 0, p, p, p, None) == 1 and "k = 256" in err()
    assert lib.tcavt_ngram_draft(p, 8, p, p, p, p, 1, 3, 0, 0, p, p, p, None) == 1 and "max_matching_ngram_size" in err()
    assert lib.tcavt_ngram_draft(p, 8, p, p, p, p, 0, 3, 2, 0, p, p, p, None) == 1 and "S = 0" in err()
    multi = lambda S, T, nq=8, nkv=2, lmax=200, dt=capi.F16, layout=0, q=p: lib.tcavt_attn_decode_multi(
        q, p, p, p, p, S, T, nq, nkv, lmax, 0.125, dt, layout, None)
    assert multi(2, 0) == 1 and "T = 0" in err()
    assert multi(2, 201) == 1 and "T = 201" in err()
    assert multi(0, 2) == 1 and "bad shape" in err()
    assert multi(2, 2, nq=6, nkv=4) == 1 and "bad shape" in err()
    assert multi(2, 2, dt=capi.F32) == 1 and "dtype16" in err()
    assert multi(2, 2, q=None) == 1 and "null" in err()
    assert multi(2, 2, q=72) == 1 and "aligned" in err()
    assert multi(3, 3, layout=2) == 1 and "out_layout" in err()  # 9 rows > 8
    assert multi(5, 7, layout=1) == 1 and "out_layout" in err()  # 35 rows > 32
    assert multi(2, 2, lmax=20000) == 1 and "score buffer" in err()
    a = capi.DecodeArgs()
    assert lib.tcavt_llama_decode_step_multi(ctypes.byref(a), 0, None) == 1 and "T = 0" in err()
    assert lib.tcavt_llama_decode_step_multi(None, 2, None) == 1 and "null" in err()
    for f in ("layers", "gamma_final", "rope_cos", "rope_sin", "table", "txt_mod", "cur_tok", "pos", "h16", "part", "qkv", "att", "act",
              "x16", "logits", "bad_id_flag", "k_cache", "v_cache"):
        setattr(a, f, ctypes.cast(p, type(getattr(a, f))) if f == "layers" else p)
    a.n_layers, a.H, a.I, a.nq, a.nkv, a.V, a.dtype16, a.kv_lmax, a.rope_L = 2, 256, 512, 8, 2, 512, capi.F16, 200, 200
    a.B = 9
    assert lib.tcavt_llama_decode_step_multi(ctypes.byref(a), 2, None) == 1 and "multiple of T" in err()
    a.B = 36
    assert lib.tcavt_llama_decode_step_multi(ctypes.byref(a), 4, None) == 1 and "exceed 32" in err()
    a.B, a.rope_L = 8, 199
    assert lib.tcavt_llama_decode_step_multi(ctypes.byref(a), 4, None) == 1 and "rope_L" in err()
    a.rope_L = 200
    a.k_cache = a.v_cache = None
    a.kv8_k_codes = a.kv8_k_scales = a.kv8_v_codes = a.kv8_v_scales = p
    assert lib.tcavt_llama_decode_step_multi(ctypes.byref(a), 4, None) == 1 and "kv8" in err()
    v = capi.SpecVerifyArgs()
    assert lib.tcavt_spec_verify(ctypes.byref(v), None) == 1 and "sample" in err()
    assert lib.tcavt_spec_verify(None, None) == 1 and "null" in err()
    sa = capi.SampleArgs()
    v.sample = ctypes.pointer(sa)
    assert lib.tcavt_spec_verify(ctypes.byref(v), None) == 1 and "n_draft" in err()


# ---------------------------------------------------------------------------------------------------------------------------
# generate_batch: argument errors, launch sequence

BAD = [
    (dict(prompt_lookup_num_tokens=0), "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=8), "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=True), "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=2.0), "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=0), "max_matching_ngram_size"),
    (dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=9), "max_matching_ngram_size"),
    (dict(prompt_lookup_num_tokens=3, kv_cache="fp8"), "kv_cache='fp8'"),
    (dict(prompt_lookup_num_tokens=3, share_prefix=True), "share_prefix"),
    (dict(prompt_lookup_num_tokens=3, num_beams=2, do_sample=False), "num_beams"),
    (dict(prompt_lookup_num_tokens=3, return_logprobs=True), "return_logprobs"),
    (dict(prompt_lookup_num_tokens=3, stop_sequences=[[1, 2]]), "stop_sequences"),
    (dict(prompt_lookup_num_tokens=7), "decode rows"),                               # 5 * 8 rows
    (dict(prompt_lookup_num_tokens=3, num_return_sequences=2), "decode rows"),       # 10 * 4 rows
    (dict(prompt_lookup_num_tokens=3, pad_token_id=512), "pad_token_id"),
    (dict(prompt_lookup_num_tokens=3, pad_token_id=-1), "pad_token_id"),
]


@pytest.mark.parametrize("kw,match", BAD, ids=[str(i) for i in range(len(BAD))])
def test_argument_errors_before_a_device_is_touched(kw, match):
    with prompt_lookup_stub.stubbed() as stub:
        cfg, m = generation_stub.tiny_model()
        vis, ids, mask = generation_stub._requests(cfg, 5)
        n_before = len(stub.calls)  # (loading the weights casts them)
        with pytest.raises(ValueError, match=match):
            m.mllm.generate_batch(vis, input_ids=ids, attention_mask=mask, use_graph=False, **dict(dict(pad_token_id=7, max_new_tokens=4), **kw))
        assert len(stub.calls) == n_before


def test_generate_pool_does_not_take_the_argument():
    import inspect

    from tcavt_amd import mllm

    assert "prompt_lookup_num_tokens" not in inspect.signature(mllm.LlamaMultiModal.generate_pool).parameters
    sig = inspect.signature(mllm.LlamaMultiModal.generate_batch).parameters
    assert sig["prompt_lookup_num_tokens"].default is None and sig["max_matching_ngram_size"].default == 2


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(prompt_lookup_stub.SCENARIOS))
def test_launch_sequence_and_workspace_match_the_golden_trace(golden, name):
    assert sorted(golden) == sorted(prompt_lookup_stub.SCENARIOS)
    got = json.loads(json.dumps(prompt_lookup_stub.record(name)[0]))
    want = golden[name]
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    assert got["calls"] == want["calls"]
    assert got["workspace"] == want["workspace"]


def test_launch_sequence_shape():
    """what the golden file pins, stated: the first token through the existing slots sampler on the prefill's logits, then at most
    N - 1 steps of draft -> decode_step_multi -> spec_verify at S * (k + 1) rows on a cache of Nq + Lt + N + k rows"""
    rec, res = prompt_lookup_stub.record("k3_n7")
    names = [c[0] for c in rec["calls"]]
    i = names.index("tcavt_sample_logits_slots")
    assert "tcavt_llama_decode_step" not in names and names.count("tcavt_sample_logits_slots") == 1
    assert names[i + 1:] == ["tcavt_ngram_draft", "tcavt_llama_decode_step_multi", "tcavt_spec_verify"] * 6
    step = rec["calls"][i + 2]
    assert step[1][0]["B"] == 12 and step[1][1] == 4 and step[1][0]["kv_lmax"] == step[1][0]["rope_L"] == 16 + 6 + 7 + 3
    assert rec["calls"][i + 1][1] == [6 + 7, 3, 3, 2, 7]  # hist_cap, S, k, max_matching_ngram_size, pad
    assert rec["calls"][i + 3][1] == [dict(S=3, T=4)]
    rec, res = prompt_lookup_stub.record("k1_m4_poll2_rules")
    info = res[1]
    assert info["steps"] == 5 and info["drafted"].tolist() == [0, 0] and info["accepted"].tolist() == [0, 0]
    assert info["n_generated"].tolist() == [6, 6]
    rec, _ = prompt_lookup_stub.record("k7_nret2")
    names = [c[0] for c in rec["calls"]]
    assert names.index("tcavt_kv_fanout") < names.index("tcavt_sample_logits_slots") < names.index("tcavt_ngram_draft")
