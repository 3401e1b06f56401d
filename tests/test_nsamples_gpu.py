"""n continuations per prompt on the GPU: tcavt_kv_fanout as a byte copy (both cache forms, sentinels around everything it may
not write), its refusals, and generate_batch(num_return_sequences=3) on the tiny generation fixture -- greedy rows against the
reference model's continuation (tests/golden/tiny_generation.npz), the decode cache against the prefill's, sampling (seed, graph,
Philox rows), ending rules, and what a call leaves behind for the next one."""
import ctypes

import numpy as np
import pytest
import torch

from tests.stop_util import cut_row
from tests.util import load_generation_case

pytestmark = pytest.mark.gpu

# the byte-copy shape
NL, B, NKV, SRC_L, KV_L, V, CAP, N_IDS, N_IMG = 2, 3, 2, 7, 11, 48, 9, 4, 2
KV_LEN = [7, 3, 5]
GUARD = 64  # elements in front of and behind every buffer (a multiple of 16 bytes for every dtype used)
BYTE_SENT, INT_SENT, F_SENT = 0xA5, -7, -123.5
PLANES = ("k_codes", "k_scales", "v_codes", "v_scales")


def _guarded(shape, dtype, fill, dev):
    """A buffer with GUARD sentinel elements on either side: -> (the whole allocation, the buffer)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n].view(shape)


def _case(form, n, dev, seed=0):
    """Source (random bytes), destination / state / logits (sentinels) of one fan-out: dicts name -> (whole, buffer)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    R = B * n
    bufs = {}
    if form == "16-bit":
        shapes = {"k": (NKV * 128,), "v": (NKV * 128,)}
        for nm, tail in shapes.items():
            bufs["src_" + nm] = _guarded((NL, B, SRC_L) + tail, torch.uint8, 0, dev)
            bufs["dst_" + nm] = _guarded((NL, R, KV_L) + tail, torch.uint8, BYTE_SENT, dev)
    else:
        for nm in PLANES:
            per = 64 if nm.endswith("codes") else 2
            bufs["src_" + nm] = _guarded((NL, B, NKV, SRC_L, per), torch.uint8, 0, dev)
            bufs["dst_" + nm] = _guarded((NL, R, NKV, KV_L, per), torch.uint8, BYTE_SENT, dev)
    for nm, (whole, buf) in bufs.items():
        if nm.startswith("src_"):
            buf.copy_(rnd(*buf.shape))
    bufs["prompt_ids"] = _guarded((B, N_IDS), torch.int64, 0, dev)
    bufs["prompt_ids"][1].copy_(torch.randint(0, 1000, (B, N_IDS), generator=g))
    bufs["kv_len"] = _guarded((B,), torch.int32, 0, dev)
    bufs["kv_len"][1].copy_(torch.tensor(KV_LEN, dtype=torch.int32))
    bufs["logits_src"] = _guarded((B, V), torch.float32, 0.0, dev)
    bufs["logits_src"][1].view(torch.uint8).copy_(rnd(B, V * 4))  # (any bits: every comparison below is of bytes)
    bufs["logits_dst"] = _guarded((R, V), torch.float32, F_SENT, dev)
    bufs["history"] = _guarded((R, CAP), torch.int64, INT_SENT, dev)
    for nm in ("hist_len", "pos", "finished"):
        bufs[nm] = _guarded((R,), torch.int32, INT_SENT, dev)
    bufs["cur_tok"] = _guarded((R,), torch.int64, INT_SENT, dev)  # the sampler's: no argument of the entry
    bufs["step"] = _guarded((1,), torch.int32, INT_SENT, dev)
    return bufs


def _caches(bufs, form, side):
    names = ("k", "v") if form == "16-bit" else PLANES
    out = tuple(bufs[f"{side}_{nm}"][1] for nm in names)
    return tuple(t.view(torch.float16) for t in out) if form == "16-bit" else out


def _snapshot(bufs):
    torch.cuda.synchronize()
    return {nm: whole.clone().cpu() for nm, (whole, _) in bufs.items()}


def _expected(before, form, n, rows):
    """What the allocations hold after the fan-out, from their content before it."""
    R = B * n
    exp = {nm: t.clone() for nm, t in before.items()}
    inner = lambda t, shape: t[GUARD:GUARD + int(np.prod(shape))].view(shape)
    for nm in (("k", "v") if form == "16-bit" else PLANES):
        if form == "16-bit":
            s, d = inner(exp["src_" + nm], (NL, B, SRC_L, NKV * 128)), inner(exp["dst_" + nm], (NL, R, KV_L, NKV * 128))
        else:
            per = 64 if nm.endswith("codes") else 2
            s, d = inner(exp["src_" + nm], (NL, B, NKV, SRC_L, per)), inner(exp["dst_" + nm], (NL, R, NKV, KV_L, per))
        for b in range(B):
            for j in range(n):
                if form == "16-bit":
                    d[:, b * n + j, :rows] = s[:, b, :rows]
                else:
                    d[:, b * n + j, :, :rows] = s[:, b, :, :rows]
    ids, ls = inner(exp["prompt_ids"], (B, N_IDS)), inner(exp["logits_src"], (B, V))
    hist, ld = inner(exp["history"], (R, CAP)), inner(exp["logits_dst"], (R, V))
    for b in range(B):
        for j in range(n):
            r = b * n + j
            hist[r, :N_IDS] = ids[b]
            ld[r] = ls[b]
            inner(exp["hist_len"], (R,))[r] = KV_LEN[b] - N_IMG
            inner(exp["pos"], (R,))[r] = KV_LEN[b]
            inner(exp["finished"], (R,))[r] = 0
    return exp


def _same_bits(a, b):
    return torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a, b.view(torch.uint8) if b.dtype != torch.uint8 else b)


@pytest.mark.parametrize("rows", [1, 5, 7])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("form", ["16-bit", "KV8"])
def test_fanout_is_a_byte_copy_and_writes_nothing_else(gpu, form, n, rows):
    from tcavt_amd import ops

    dev = gpu["device"]
    bufs = _case(form, n, dev)
    before = _snapshot(bufs)
    ops.kv_fanout(_caches(bufs, form, "src"), _caches(bufs, form, "dst"), n, rows, SRC_L, KV_L, NL, NKV, bufs["prompt_ids"][1],
                  bufs["kv_len"][1], N_IMG, bufs["logits_src"][1], bufs["logits_dst"][1], bufs["history"][1], bufs["hist_len"][1],
                  bufs["pos"][1], bufs["finished"][1])
    after = _snapshot(bufs)
    want = _expected(before, form, n, rows)
    for nm in before:
        assert _same_bits(after[nm], want[nm]), nm
    for nm in before:  # the source, the prompts, kv_len, the sampler's cur_tok and step: as they were
        if nm.startswith("src_") or nm in ("prompt_ids", "kv_len", "logits_src", "cur_tok", "step"):
            assert _same_bits(after[nm], before[nm]), nm
    # the copy is there at all: a destination sample's rows differ from the sentinel, and rows >= rows still hold it
    first = "dst_k" if form == "16-bit" else "dst_k_codes"
    d = bufs[first][1].cpu()
    assert bool((d[:, :, :rows] != BYTE_SENT).any()) if form == "16-bit" else bool((d[:, :, :, :rows] != BYTE_SENT).any())
    assert bool((d[:, :, rows:] == BYTE_SENT).all()) if form == "16-bit" else bool((d[:, :, :, rows:] == BYTE_SENT).all())


def _args(bufs, form, n, rows):
    from tcavt_amd import capi

    a = capi.KvFanoutArgs()
    for nm in (("k", "v") if form == "16-bit" else PLANES):
        for side in ("src", "dst"):
            setattr(a, f"{side}_{nm}", bufs[f"{side}_{nm}"][1].data_ptr())
    for nm in ("prompt_ids", "kv_len", "logits_src", "logits_dst", "history", "hist_len", "pos", "finished"):
        setattr(a, nm, bufs[nm][1].data_ptr())
    a.n_layers, a.B, a.n, a.rows, a.src_lmax, a.kv_lmax, a.nkv, a.dtype16 = NL, B, n, rows, SRC_L, KV_L, NKV, capi.F16
    a.n_ids, a.hist_cap, a.n_image, a.V = N_IDS, CAP, N_IMG, V
    return a


@pytest.mark.parametrize("form", ["16-bit", "KV8"])
def test_fanout_refusals_name_the_argument_and_write_nothing(gpu, form):
    from tcavt_amd import capi, ops

    dev = gpu["device"]
    lib = capi.lib()
    bufs = _case(form, 3, dev)
    before = _snapshot(bufs)
    cache0 = "src_k" if form == "16-bit" else "src_k_codes"
    other = "src_k_codes" if form == "16-bit" else "src_k"
    cases = [(nm, None, nm.encode() + b" is a null pointer") for nm in
             ("prompt_ids", "kv_len", "logits_src", "logits_dst", "history", "hist_len", "pos", "finished")]
    cases += [("dst_v" if form == "16-bit" else "dst_v_scales", None, b"come together"),
              (other, bufs[cache0][1].data_ptr(), b"exclude each other"),
              (cache0, bufs[cache0][1].data_ptr() + 8, b"16-byte aligned"),
              ("dst_k" if form == "16-bit" else "dst_v_codes", bufs[cache0][1].data_ptr() + 4, b"16-byte aligned"),
              ("logits_src", bufs["logits_src"][1].data_ptr() + 4, b"logits_src and logits_dst must be 16-byte aligned"),
              ("logits_dst", bufs["logits_dst"][1].data_ptr() + 8, b"logits_src and logits_dst must be 16-byte aligned"),
              ("rows", 0, b"rows = 0"), ("rows", SRC_L + 1, b"rows = 8"), ("rows", -1, b"rows = -1"),
              ("B", 0, b"B = 0"), ("n", 0, b"n = 0"), ("n", -1, b"n = -1"),
              ("n_ids", -1, b"n_ids = -1"), ("n_ids", CAP + 1, b"n_ids = 10"), ("V", 0, b"V = 0"), ("V", -4, b"V = -4")]
    if form == "KV8":
        cases.append(("dst_k_scales", bufs["dst_k_scales"][1].data_ptr() + 1, b"scale planes must be 2-byte aligned"))
    for field, value, msg in cases:
        a = _args(bufs, form, 3, 5)
        setattr(a, field, value)
        rc = lib.tcavt_kv_fanout(ctypes.byref(a), ops.stream_ptr())
        err = lib.tcavt_last_error()
        assert rc != 0 and msg in err, (field, value, rc, err)
    a = _args(bufs, form, 3, 5)
    a.kv_lmax = 4  # rows = 5 > min(src_lmax, kv_lmax)
    assert lib.tcavt_kv_fanout(ctypes.byref(a), ops.stream_ptr()) != 0 and b"rows = 5" in lib.tcavt_last_error()
    assert lib.tcavt_kv_fanout(None, ops.stream_ptr()) != 0 and b"args is a null pointer" in lib.tcavt_last_error()
    after = _snapshot(bufs)
    for nm in before:
        assert _same_bits(after[nm], before[nm]), nm
    # ops.kv_fanout's own extent guards: a destination one sample short, a history one row short
    short = tuple(t[:, :-1].contiguous() for t in _caches(bufs, form, "dst"))
    tail = (bufs["prompt_ids"][1], bufs["kv_len"][1], N_IMG, bufs["logits_src"][1], bufs["logits_dst"][1])
    state = (bufs["hist_len"][1], bufs["pos"][1], bufs["finished"][1])
    with pytest.raises(capi.TcavtError, match="kernel needs"):
        ops.kv_fanout(_caches(bufs, form, "src"), short, 3, 5, SRC_L, KV_L, NL, NKV, *tail, bufs["history"][1], *state)
    with pytest.raises(capi.TcavtError, match="history"):
        ops.kv_fanout(_caches(bufs, form, "src"), _caches(bufs, form, "dst"), 3, 5, SRC_L, KV_L, NL, NKV, *tail,
                      bufs["history"][1][:-1], *state)


# --------------------------------------------------------------------------------------
# the model
# --------------------------------------------------------------------------------------
_MODEL = {}
NSEQ = 3
SEED = 5  # the sampling tests' seed: test_sampling_... asserts that it spreads at least one prompt's rows


def _setup(dev):
    """The fixture model, built once for the module."""
    if "m" not in _MODEL:
        from tcavt_amd import model

        fx, cfg, weights, t = load_generation_case()
        m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights, device=dev).eval()
        _MODEL.update(m=m, fx=fx, cfg=cfg, weights=weights, t=t, g={k: v.to(dev) for k, v in t.items()})
    return _MODEL


def _batch(M, **kw):
    g = M["g"]
    res = M["m"].mllm.generate_batch(g["vision_emb"], None, input_ids=g["input_ids"], attention_mask=g["attention_mask"], **kw)
    torch.cuda.synchronize()
    M["m"].mllm.check_flags()
    return res


@pytest.mark.parametrize("use_graph", [False, True])
def test_greedy_rows_are_the_reference_continuation_three_times(gpu, use_graph):
    M = _setup(gpu["device"])
    fx = M["fx"]
    assert fx["greedy_tokens"].shape[0] == 3
    N = fx["greedy_tokens"].shape[1]
    kw = dict(max_new_tokens=N, do_sample=False, use_graph=use_graph)
    out = _batch(M, num_return_sequences=NSEQ, repetition_penalty=1.0, no_repeat_ngram_size=0, **kw).cpu().numpy()
    assert out.dtype == np.int64 and out.shape == (3 * NSEQ, N)
    for b in range(3):
        for j in range(NSEQ):
            assert np.array_equal(out[NSEQ * b + j], out[NSEQ * b]), (b, j)
            assert np.array_equal(out[NSEQ * b + j], fx["greedy_tokens"][b]), (b, j)
    # the reference's processors on (1.2, 3-gram): against the n = 1 call's own output
    one = _batch(M, repetition_penalty=1.2, no_repeat_ngram_size=3, **kw).cpu().numpy()
    out2 = _batch(M, num_return_sequences=NSEQ, repetition_penalty=1.2, no_repeat_ngram_size=3, **kw).cpu().numpy()
    assert np.array_equal(one, fx["greedy_proc_tokens"])
    assert np.array_equal(out2, np.repeat(one, NSEQ, axis=0))


@pytest.mark.parametrize("kv", ["fp16", "fp8"])
def test_decode_cache_holds_the_prefills_rows(gpu, kv):
    dev = gpu["device"]
    M = _setup(dev)
    mm, ll, t = M["m"].mllm, M["cfg"].llama, M["t"]
    Lt, N = t["input_ids"].shape[1], 4
    L, Lmax, nkv = 16 + Lt, 16 + Lt + N, ll.n_kv_heads
    st = mm.llama_wrapper.storage
    _batch(M, max_new_tokens=N, num_return_sequences=NSEQ, do_sample=True, seed=SEED, kv_cache=kv)
    names = [("kc", 0), ("vc", 0)] if kv == "fp16" else [("kv8.kc", 64), ("kv8.ks", 2), ("kv8.vc", 64), ("kv8.vs", 2)]
    for nm, per in names:
        if kv == "fp16":
            src = mm._ws.get(f"gen.src.{nm}", (ll.layers, 3, L, nkv * ll.head_dim), st, dev).view(torch.uint8).cpu()
            dst = mm._ws.get(f"gen.{nm}", (ll.layers, 3 * NSEQ, Lmax, nkv * ll.head_dim), st, dev).view(torch.uint8).cpu()
        else:
            src = mm._ws.get(f"gen.src.{nm}", (ll.layers, 3, nkv, L, per), torch.uint8, dev).transpose(2, 3).cpu()
            dst = mm._ws.get(f"gen.{nm}", (ll.layers, 3 * NSEQ, nkv, Lmax, per), torch.uint8, dev).transpose(2, 3).cpu()
        for b in range(3):
            kvl = 16 + int(t["attention_mask"][b].sum())
            assert bool(src[:, b, :kvl].any()), nm
            for j in range(NSEQ):
                assert torch.equal(dst[:, NSEQ * b + j, :kvl], src[:, b, :kvl]), (nm, b, j)


def test_sampling_is_a_function_of_the_seed_and_row_r_draws_from_philox_row_r(gpu):
    from tcavt_amd import generation, ops

    dev = gpu["device"]
    M = _setup(dev)
    mm, g, vocab = M["m"].mllm, M["g"], M["cfg"].llama.vocab
    N = 10
    kw = dict(max_new_tokens=N, num_return_sequences=NSEQ, do_sample=True)
    a = _batch(M, seed=SEED, **kw).cpu()
    b = _batch(M, seed=SEED, **kw).cpu()
    e = _batch(M, seed=SEED, use_graph=False, **kw).cpu()
    c = _batch(M, seed=SEED + 1, **kw).cpu()
    assert tuple(a.shape) == (3 * NSEQ, N)
    assert torch.equal(a, b) and torch.equal(a, e) and not torch.equal(a, c)  # two runs equal, eager == graph, another seed differs
    assert bool(((a >= 0) & (a < vocab)).all())
    spread = [len({tuple(r) for r in a[NSEQ * p:NSEQ * p + NSEQ].tolist()}) for p in range(3)]
    print("distinct rows per prompt:", spread)
    assert max(spread) > 1, spread  # (a condition on the fixture and SEED: the continuations of a prompt are not all one row)
    # Philox rows: the prefill's own logits (an n = 1 call that leaves them untouched: greedy, no penalty, no ban), replicated to
    # 9 rows, through the sampler with the prompts' histories at step 0
    _batch(M, max_new_tokens=1, do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0)
    logits = mm._ws.get("gen.logits", (3, vocab), torch.float32, dev).repeat_interleave(NSEQ, 0).contiguous()
    ids, mask = g["input_ids"], g["attention_mask"]
    Lt, R = ids.shape[1], 3 * NSEQ
    hist = torch.zeros(R, Lt + N, dtype=torch.int64, device=dev)
    hist[:, :Lt] = ids.repeat_interleave(NSEQ, 0)
    hist_len = mask.sum(1).to(torch.int32).repeat_interleave(NSEQ, 0).contiguous()
    out = torch.full((R, N), -1, dtype=torch.int64, device=dev)
    sp = generation.sample_params(0.9, 0.9, 1.2, 40, 3, True, None, 0, SEED)  # generate_batch's defaults
    ops.sample_logits(logits, hist, hist_len, sp, torch.zeros(1, dtype=torch.int32, device=dev),
                      torch.zeros(R, dtype=torch.int64, device=dev), torch.zeros(R, dtype=torch.int32, device=dev),
                      torch.zeros(R, dtype=torch.int32, device=dev), out, advance_pos=False)
    torch.cuda.synchronize()
    assert torch.equal(out[:, 0].cpu(), a[:, 0])


def test_rules_cut_the_unruled_run_and_polling_returns_the_same_tokens(gpu):
    from tests.test_stop_rules_gpu import PAD, _rules_from

    M = _setup(gpu["device"])
    vocab, N = M["cfg"].llama.vocab, 16
    kw = dict(max_new_tokens=N, num_return_sequences=NSEQ, do_sample=True, seed=SEED, pad_token_id=PAD)
    plain = _batch(M, **kw).cpu()
    rows = plain.tolist()
    assert len(rows) == 3 * NSEQ
    rules = _rules_from(rows, vocab, 0, 5, 4, 7)  # row 0's step-5 token as a stop token, row 4's steps 7 .. 9 as a sequence
    want = [cut_row(rules, r, None, PAD) for r in rows]
    reasons = [w[2] for w in want]
    assert 2 in reasons and 3 in reasons, reasons  # (a condition on the input: both rules fire somewhere)
    rk = dict(stop_token_ids=rules.stop_token_ids, stop_sequences=rules.stop_sequences, return_info=True)
    outs = []
    for use_graph, poll in ((True, None), (True, 2), (False, 2)):
        out, info = _batch(M, use_graph=use_graph, poll_every=poll, **kw, **rk)
        assert out.cpu().tolist() == [w[0] for w in want], (use_graph, poll)
        assert info["finish_reason"].shape == info["n_generated"].shape == (3 * NSEQ,)
        assert info["finish_reason"].tolist() == reasons and info["n_generated"].tolist() == [w[1] for w in want]
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(_batch(M, poll_every=2, **kw).cpu(), plain)  # unruled: polled == unpolled


def test_a_fanned_out_call_leaves_nothing_behind(gpu):
    M = _setup(gpu["device"])
    fx = M["fx"]
    N = fx["greedy_tokens"].shape[1]
    greedy = dict(max_new_tokens=N, do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0)
    before = _batch(M, **greedy).cpu()
    sampled = _batch(M, max_new_tokens=N, do_sample=True, seed=3).cpu()
    _batch(M, max_new_tokens=N, num_return_sequences=NSEQ, do_sample=True, seed=3)
    assert torch.equal(_batch(M, **greedy).cpu(), before) and np.array_equal(before.numpy(), fx["greedy_tokens"])
    assert torch.equal(_batch(M, max_new_tokens=N, do_sample=True, seed=3).cpu(), sampled)
    # FP8 weights at B * n = 9 rows: bit-reproducible, flags clean (_batch checks them)
    w8 = dict(max_new_tokens=N, num_return_sequences=NSEQ, do_sample=True, seed=3, decode_weights="fp8")
    x = _batch(M, **w8).cpu()
    y = _batch(M, **w8).cpu()
    assert tuple(x.shape) == (3 * NSEQ, N) and torch.equal(x, y)
