"""Ending rules of text generation without a GPU: tcavt_sample_tokens is declared, exported and bound and its two structs are laid
out as the header's; every refusal of the C entry names its argument before any launch; stopping.StopRules validates, builds the
bitmap and states the rules on a token list (first_end: known answers); generate_batch / generate_pool refuse bad values before
anything touches a device; and the tests' own ban helper and first_end agree with transformers' MinNewTokensLengthLogitsProcessor
and EosTokenCriteria."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.stop_util import ban_scores, cut_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------
# symbols and layout
# ------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound():
    from tcavt_amd import capi

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tcavt.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+tcavt_sample_tokens\s*\(\s*const\s+tcavt_sample_args\s*\*\s*\w+\s*,\s*tcavt_stream_t\s+\w+\s*\)\s*;", header)
    assert "#define TCAVT_ABI_VERSION 5" in header
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "tcavt_sample_tokens")
    assert "tcavt_sample_tokens" in capi.EXPORTED_SYMBOLS
    fn = capi.lib().tcavt_sample_tokens
    assert fn.argtypes == [ctypes.POINTER(capi.SampleArgs), ctypes.c_void_p] and fn.restype is ctypes.c_int
    assert capi.lib().tcavt_abi_version() == capi.ABI_VERSION == 5
    # the three existing entries keep their prototypes
    for name, n_args in (("tcavt_sample_logits", 17), ("tcavt_sample_logits_slots", 19), ("tcavt_sample_logits_rows", 21)):
        assert len(getattr(capi.lib(), name).argtypes) == n_args


def _struct_fields(name):
    text = open(os.path.join(ROOT, "include", "tcavt.h")).read()
    body = text[text.index("typedef struct %s {" % name):text.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.split("{")[-1].strip()
        if not decl:
            continue
        decl = re.sub(r"^(const\s+)?[A-Za-z0-9_]+(\s+const)?\s*\**(\s*const)?", "", decl)
        names += [p.strip().lstrip("*").strip() for p in decl.split(",") if p.strip()]
    return names


@pytest.mark.parametrize("cname,mirror", [("tcavt_stop_rules", "StopRules"), ("tcavt_sample_args", "SampleArgs")])
def test_struct_mirrors_match_header_layout(cname, mirror, tmp_path):
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


# ------------------------------------------------------------------------------------------------
# refusals of the C entry (fake, aligned pointers: every call below is refused before a launch)
# ------------------------------------------------------------------------------------------------
def _args(capi, sp, mode, stop=None, **kw):
    a = capi.SampleArgs()
    for n in ("logits", "history", "hist_len", "step", "cur_tok", "pos", "finished", "out_tokens"):
        setattr(a, n, 256)
    if mode in ("slots", "rows"):
        a.max_new = a.out_row = 256
    if mode == "rows":
        a.slot_of_row = 256
    a.params = ctypes.pointer(sp)
    a.rows, a.V, a.n_state, a.hist_cap, a.out_cap, a.advance_pos = 2, 512, 3, 8, 4, 1
    if stop is not None:
        a.stop = ctypes.pointer(stop)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("mode", ["batch", "slots", "rows"])
def test_sample_tokens_refuses_bad_stop_rules_without_a_device(mode):
    from tcavt_amd import capi

    lib = capi.lib()
    sp = capi.SampleParams(0.9, 0.9, 1.2, 40, 3, 1, -1, 0, 1)       # no EOS
    sp_eos = capi.SampleParams(0.9, 0.9, 1.2, 40, 3, 1, 7, 0, 1)

    def call(params=sp, **fields):
        r = capi.StopRules()
        for k, v in fields.items():
            setattr(r, k, v)
        a = _args(capi, params, mode, stop=r)
        rc = lib.tcavt_sample_tokens(ctypes.byref(a), None)
        return rc, lib.tcavt_last_error()

    for n in (-1, 17):
        rc, err = call(n_seqs=n, stop_seqs=256, stop_seq_len=256)
        assert rc == 1 and err.startswith(b"sample_tokens:") and b"n_seqs = %d" % n in err, (n, rc, err)
    rc, err = call(n_seqs=2, stop_seqs=None, stop_seq_len=256)
    assert rc == 1 and b"stop_seqs" in err and b"null" in err, err
    rc, err = call(n_seqs=2, stop_seqs=256, stop_seq_len=None)
    assert rc == 1 and b"stop_seq_len" in err and b"null" in err, err
    rc, err = call(min_new_tokens=-1, stop_bitmap=256)
    assert rc == 1 and b"min_new_tokens = -1" in err, err
    rc, err = call(min_new_tokens=3)  # neither EOS nor a bitmap
    assert rc == 1 and b"min_new_tokens = 3" in err and b"nothing to ban" in err, err
    for bad in (258, 257, 259):
        rc, err = call(params=sp_eos, min_new_tokens=3, stop_bitmap=bad)
        assert rc == 1 and b"stop_bitmap" in err and b"4-byte aligned" in err, err


def test_sample_tokens_refuses_bad_arguments_without_a_device():
    from tcavt_amd import capi

    lib = capi.lib()
    sp = capi.SampleParams(0.9, 0.9, 1.2, 40, 3, 1, -1, 0, 1)
    assert lib.tcavt_sample_tokens(None, None) == 1 and b"args" in lib.tcavt_last_error()
    for mode, ptrs in (("batch", ()), ("slots", ("max_new", "out_row")), ("rows", ("max_new", "out_row"))):
        for n in ("logits", "history", "hist_len", "step", "cur_tok", "pos", "finished", "out_tokens") + ptrs:
            a = _args(capi, sp, mode, **{n: None})
            rc, err = lib.tcavt_sample_tokens(ctypes.byref(a), None), lib.tcavt_last_error()
            assert rc == 1 and err.startswith(b"sample_tokens:") and n.encode() in err and b"null" in err, (mode, n, rc, err)
        for n in ("rows", "V", "hist_cap", "out_cap"):
            a = _args(capi, sp, mode, **{n: 0})
            rc, err = lib.tcavt_sample_tokens(ctypes.byref(a), None), lib.tcavt_last_error()
            assert rc == 1 and n.encode() + b" = 0" in err, (mode, n, rc, err)
    a = _args(capi, sp, "rows", n_state=0)
    assert lib.tcavt_sample_tokens(ctypes.byref(a), None) == 1 and b"n_state = 0" in lib.tcavt_last_error()
    a = _args(capi, sp, "batch")
    a.params = None
    assert lib.tcavt_sample_tokens(ctypes.byref(a), None) == 1 and b"params" in lib.tcavt_last_error()


# ------------------------------------------------------------------------------------------------
# StopRules: validation, arrays, first_end
# ------------------------------------------------------------------------------------------------
def test_stop_rules_validate_on_the_host():
    from tcavt_amd.stopping import StopRules

    V = 100
    for bad in ([-1], [V], [3, V + 5]):
        with pytest.raises(ValueError, match="stop token id"):
            StopRules(V, stop_token_ids=bad)
    with pytest.raises(ValueError, match="at most 16"):
        StopRules(V, stop_sequences=[[1]] * 17)
    with pytest.raises(ValueError, match="1 .. 8 ids"):
        StopRules(V, stop_sequences=[[1, 2], []])
    with pytest.raises(ValueError, match="1 .. 8 ids"):
        StopRules(V, stop_sequences=[list(range(9))])
    with pytest.raises(ValueError, match="stop sequence id"):
        StopRules(V, stop_sequences=[[1, V]])
    with pytest.raises(ValueError, match="min_new_tokens"):
        StopRules(V, min_new_tokens=-1)
    assert StopRules(V).empty and not StopRules(V, min_new_tokens=1).empty
    r = StopRules(V, stop_sequences=[[1]] * 16 + [], stop_token_ids=[0, V - 1])
    assert len(r.stop_sequences) == 16 and not r.empty


def test_stop_rules_arrays():
    from tcavt_amd.stopping import StopRules

    V = 1003
    assert V % 32 != 0
    r = StopRules(V, stop_token_ids=[0, 31, 32, V - 1, 31], stop_sequences=[[5], [7, 8, 9], list(range(10, 18))], min_new_tokens=2)
    bm = r.bitmap.numpy().view(np.uint32)
    assert r.bitmap.dtype == torch.int32 and bm.shape == ((V + 31) // 32,)
    want = np.zeros_like(bm)
    want[0] = (1 << 0) | (1 << 31)
    want[1] = 1 << 0
    want[(V - 1) >> 5] |= 1 << ((V - 1) & 31)
    assert np.array_equal(bm, want)
    bits = [i for i in range(32 * bm.size) if (int(bm[i >> 5]) >> (i & 31)) & 1]
    assert bits == [0, 31, 32, V - 1]
    assert r.seqs.dtype == torch.int64 and tuple(r.seqs.shape) == (3, 8) and r.seq_len.dtype == torch.int32
    assert r.seq_len.tolist() == [1, 3, 8]
    assert r.seqs.tolist() == [[5] + [0] * 7, [7, 8, 9] + [0] * 5, list(range(10, 18))]
    assert r.min_new_tokens == 2


def test_first_end_known_answers():
    from tcavt_amd.stopping import StopRules

    V, EOS = 64, 9
    r = StopRules(V, stop_token_ids=[20, 21], stop_sequences=[[4, 5, 6], [30]])
    # each reason on its own
    assert r.first_end([1, 2, 9, 3], EOS) == (3, 1)
    assert r.first_end([1, 2, 21, 9], EOS) == (3, 2)
    assert r.first_end([1, 4, 5, 6, 9], EOS) == (4, 3)
    assert r.first_end([1, 2, 30, 9], EOS) == (3, 3)
    assert r.first_end([1, 2, 3, 4], EOS, budget=3) == (3, 4)
    assert r.first_end([1, 2, 3, 4], EOS) == (4, 0) and r.first_end([1, 2, 3, 4], None, budget=9) == (4, 0)
    assert r.first_end([9, 9], None) == (2, 0) and r.first_end([9, 9], -1) == (2, 0)  # no EOS given
    # precedence 1 > 2 > 3 > 4 when two rules fire on one token
    assert StopRules(V, stop_token_ids=[EOS]).first_end([1, EOS], EOS) == (2, 1)
    assert StopRules(V, stop_sequences=[[EOS]]).first_end([1, EOS], EOS) == (2, 1)
    assert StopRules(V, stop_token_ids=[6], stop_sequences=[[5, 6]]).first_end([5, 6], EOS) == (2, 2)
    assert StopRules(V, stop_token_ids=[6]).first_end([5, 6], EOS, budget=2) == (2, 2)
    assert StopRules(V, stop_sequences=[[5, 6]]).first_end([5, 6], EOS, budget=2) == (2, 3)
    assert StopRules(V).first_end([5, EOS], EOS, budget=2) == (2, 1)
    # a sequence that would only match by using a prompt token does not match: the list holds generated tokens only, and
    # [4, 5, 6] with the 4 in the prompt leaves [5, 6, ...] here
    assert r.first_end([5, 6, 1, 2], EOS) == (4, 0)
    # ... and it matches at exactly step + 1 == n
    assert r.first_end([4, 5, 6, 1], EOS) == (3, 3)
    assert r.first_end([30], EOS) == (1, 3)
    # one sequence a suffix of another: the shorter one fires wherever the longer one would, and also on its own
    s = StopRules(V, stop_sequences=[[1, 2, 3], [2, 3]])
    assert s.first_end([7, 1, 2, 3, 4], EOS) == (4, 3) and s.first_end([7, 7, 2, 3, 4], EOS) == (4, 3)
    assert s.first_end([2, 3], EOS) == (2, 3) and s.first_end([3, 2, 7], EOS) == (3, 0)
    # cut_row: pad behind the end; an unended row ran out
    assert cut_row(r, [1, 2, 21, 3, 4], EOS, pad=0) == ([1, 2, 21, 0, 0], 3, 2)
    assert cut_row(r, [1, 2, 3], EOS, pad=0) == ([1, 2, 3], 3, 4)


# ------------------------------------------------------------------------------------------------
# the generate entries refuse bad values before anything touches a device
# ------------------------------------------------------------------------------------------------
def test_generate_entries_refuse_bad_rules_without_a_device():
    from tcavt_amd import config, model
    from tcavt_amd.weights import make_weights

    cfg = config.tiny()
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(make_weights(cfg, 0)).eval()
    V = cfg.llama.vocab
    ids = torch.zeros(2, 4, dtype=torch.int64)
    mask = torch.ones_like(ids)
    vis = torch.zeros(2, 1, 8)
    bad = [(dict(stop_token_ids=[V]), "stop token id"), (dict(stop_token_ids=[-1]), "stop token id"),
           (dict(stop_sequences=[[1]] * 17), "at most 16"), (dict(stop_sequences=[[]]), "1 .. 8 ids"),
           (dict(stop_sequences=[list(range(9))]), "1 .. 8 ids"), (dict(stop_sequences=[[V]]), "stop sequence id"),
           (dict(min_new_tokens=-1, eos_token_id=3), "min_new_tokens"), (dict(min_new_tokens=2), "nothing to ban")]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            m.mllm.generate_batch(vis, None, max_new_tokens=4, input_ids=ids, attention_mask=mask, **kw)
        with pytest.raises(ValueError, match=msg):
            m.mllm.generate_pool(vis, ids, mask, max_new_tokens=4, slots=2, **kw)
    for pe in (0, -3):
        with pytest.raises(ValueError, match="poll_every"):
            m.mllm.generate_batch(vis, None, max_new_tokens=4, input_ids=ids, attention_mask=mask, poll_every=pe)
    # legal, and nothing to do: the stats carry the two (empty) records
    out, stats = m.mllm.generate_pool(vis[:0], ids[:0], mask[:0], max_new_tokens=5, slots=4, stop_token_ids=[1], return_info=True)
    assert tuple(out.shape) == (0, 5) and stats["finish_reason"].numel() == 0 and stats["n_generated"].dtype == torch.int32


# ------------------------------------------------------------------------------------------------
# HF parity of the tests' own helpers
# ------------------------------------------------------------------------------------------------
def test_ban_helper_matches_transformers_min_new_tokens_processor():
    from transformers import MinNewTokensLengthLogitsProcessor

    V, prompt_len, m, eos, stop_ids = 97, 5, 4, 11, [0, 31, 32, 96]
    g = torch.Generator().manual_seed(3)
    scores = torch.randn(1, V, generator=g)
    proc = MinNewTokensLengthLogitsProcessor(prompt_len, m, eos_token_id=[eos, *stop_ids], device="cpu")
    for step in (0, m - 1, m, m + 3):
        ids = torch.zeros(1, prompt_len + step, dtype=torch.int64)  # the prompt and `step` generated tokens
        ref = proc(ids, scores.clone())[0].numpy()
        got = ban_scores(scores[0].numpy(), step, m, eos, stop_ids)
        assert np.array_equal(np.isinf(got), np.isinf(ref)), step
        assert np.array_equal(got[np.isfinite(got)], ref[np.isfinite(ref)])
        banned = sorted(np.flatnonzero(np.isinf(got)).tolist())
        assert banned == (sorted([eos, *stop_ids]) if step < m else []), step


def test_first_end_matches_transformers_eos_token_criteria():
    from tcavt_amd.stopping import StopRules
    from transformers.generation.stopping_criteria import EosTokenCriteria

    V, eos, stop_ids = 50, 7, [3, 31, 49]
    crit = EosTokenCriteria(eos_token_id=[eos, *stop_ids])
    rules = StopRules(V, stop_token_ids=stop_ids)
    g = torch.Generator().manual_seed(5)
    prompt = torch.tensor([3, 7, 49, 2])  # ending ids inside the prompt do not count: only generated tokens are walked
    fired = 0
    for _ in range(40):
        toks = torch.randint(0, V, (12,), generator=g)
        want = len(toks), 0
        for i in range(len(toks)):
            seq = torch.cat([prompt, toks[:i + 1]])[None]
            if bool(crit(seq, None)[0]):
                want = i + 1, (1 if int(toks[i]) == eos else 2)
                break
        assert rules.first_end(toks.tolist(), eos) == want
        fired += want[1] != 0
    assert 10 < fired  # (4 ending ids of 50 over 12 tokens: most rows end)
