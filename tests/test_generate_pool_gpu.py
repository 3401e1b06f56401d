"""The slot pool on the GPU: tcavt_sample_logits_slots against the oracle and against tcavt_sample_logits, inert and ending
slots, tcavt_slot_admit as a byte copy, and LlamaMultiModal.generate_pool on the tiny generation fixture -- the reference
model's own continuation through a refill, independence from the schedule, a refilled slot's logits against the oracle, and
generate_batch untouched.  Token ids are held bit-exact, as in tests/test_generation_gpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.util import GOLDEN, load_generation_case, rel_err

pytestmark = pytest.mark.gpu

_MODEL = {}


def _setup(dev):
    """The fixture model, built once for the module."""
    if "m" not in _MODEL:
        from tcavt_amd import model

        fx, cfg, weights, t = load_generation_case()
        m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights, device=dev).eval()
        _MODEL.update(m=m, fx=fx, cfg=cfg, weights=weights, t=t, g={k: v.to(dev) for k, v in t.items()})
    return _MODEL


def _pool(M, **kw):
    g = M["g"]
    out = M["m"].mllm.generate_pool(g["vision_emb"], g["input_ids"], g["attention_mask"], **kw)
    torch.cuda.synchronize()
    return out.cpu()


def _state(dev, R, cap, hist, hist_len, step, out_rows=None, out_cap=64, sentinel=-1):
    """Device state of R slots: (history, hist_len, step, max_new, out_row, cur, pos, finished, out)."""
    i32, i64 = torch.int32, torch.int64
    h = torch.zeros(R, cap, dtype=i64, device=dev)
    h[:, : hist.shape[1]] = torch.as_tensor(hist).to(dev)
    n_out = R if out_rows is None else max(out_rows) + 1
    return dict(history=h, hist_len=torch.as_tensor(hist_len).to(i32).to(dev), step=torch.tensor(step, dtype=i32, device=dev),
                max_new=torch.full((R,), 1 << 20, dtype=i32, device=dev),
                out_row=torch.tensor(list(range(R)) if out_rows is None else out_rows, dtype=i64, device=dev),
                cur=torch.zeros(R, dtype=i64, device=dev), pos=torch.zeros(R, dtype=i32, device=dev),
                finished=torch.zeros(R, dtype=i32, device=dev), out=torch.full((n_out, out_cap), sentinel, dtype=i64, device=dev))


def _slots_call(ops, logits, sp, st, advance_pos=True, workspace=None):
    ops.sample_logits_slots(logits, st["history"], st["hist_len"], sp, st["step"], st["max_new"], st["out_row"], st["cur"], st["pos"],
                            st["finished"], st["out"], advance_pos=advance_pos, workspace=workspace)


# ------------------------------------------------------------------------------------------------
# 1. the sampler against the oracle, every slot at its own step and output row
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_stage", [False, True], ids=["one_stage", "two_stage"])
def test_slots_sampler_matches_oracle_at_mixed_steps(gpu, two_stage):
    from oracle import generation as G
    from tcavt_amd import capi, ops

    dev = gpu["device"]
    fx = dict(np.load(os.path.join(GOLDEN, "tiny_generation.npz"), allow_pickle=False))
    R, V = fx["scores"].shape
    steps, rows = [0, 5, 11, 40, 5, 0], [3, 0, 7, 2, 9, 1]
    assert R == 6
    cap = fx["hist"].shape[1] + 4
    wsp = ops.sample_workspace(R, dev) if two_stage else None
    for seed in (1, 2, 3):
        logits = torch.from_numpy(fx["scores"]).to(dev).clone()
        st = _state(dev, R, cap, np.maximum(fx["hist"], 0), fx["hist_len"], steps, rows)
        sp = capi.SampleParams(0.9, 0.9, 1.2, 40, 3, 1, -1, 0, seed)
        _slots_call(ops, logits, sp, st, workspace=wsp)
        torch.cuda.synchronize()
        assert st["step"].tolist() == [s + 1 for s in steps] and (st["pos"] == 1).all() and not st["finished"].any()
        assert (st["hist_len"].cpu().numpy() == fx["hist_len"] + 1).all()
        out = st["out"].cpu()
        for r in range(R):
            h = fx["hist"][r, : int(fx["hist_len"][r])]
            x = G.process_logits(fx["scores"][r], h, 1.2, 3)
            want = G.select_token(x, True, 0.9, 40, 0.9, seed=seed, step=steps[r], row=rows[r])
            got = int(out[rows[r], steps[r]])
            assert got == want, (seed, r, got, want)
            assert np.isfinite(fx["warped"][r][got])
            assert got == int(st["cur"][r]) == int(st["history"][r, int(fx["hist_len"][r])])
        assert int((out != -1).sum()) == R  # one element per slot, nothing else
        proc = logits.cpu().numpy()
        assert np.array_equal(np.isinf(proc), np.isinf(fx["processed"]))
        assert np.allclose(proc[np.isfinite(proc)], fx["processed"][np.isfinite(proc)], rtol=1e-6)
        if two_stage:
            assert int(wsp[:64 + 4 * R].sum().item()) == 0


# ------------------------------------------------------------------------------------------------
# 2. equal to tcavt_sample_logits when every slot is at the same step and writes its own row
# ------------------------------------------------------------------------------------------------
def _awkward_rows(V):
    """The rows of test_two_stage_token_selection_equals_the_one_stage_form (tests/test_generation_gpu.py)."""
    g = torch.Generator().manual_seed(V)
    R = 6
    base = torch.randn(R, V, generator=g) * 3.0
    base[1] = torch.round(base[1] * 2) / 2
    base[2] = 1.25
    base[3] = float("-inf"); base[3, [5, V // 2, V - 1]] = torch.tensor([0.5, 2.0, 2.0])
    base[4] = float("-inf"); base[4, V - 3] = -7.0
    base[5, V // 3: V // 3 + 300] = base[5].max() + 1.0
    cap = 40
    hist0 = torch.randint(0, V, (R, cap), generator=g)
    hist0[:, 30:] = 0
    hist0[0, :30] = torch.arange(30) % 7 + (V - 8)
    return R, cap, base, hist0, torch.full((R,), 30, dtype=torch.int32)


@pytest.mark.parametrize("two_stage", [False, True], ids=["one_stage", "two_stage"])
@pytest.mark.parametrize("V", [512, 50000])
def test_slots_sampler_equals_the_existing_entry(gpu, V, two_stage):
    from tcavt_amd import capi, ops

    dev = gpu["device"]
    R, cap, base, hist0, hl0 = _awkward_rows(V)
    wsp = ops.sample_workspace(R, dev) if two_stage else None  # ONE workspace: the two entries alternate on it
    for do_sample, top_k, rep, ngram in ((1, 40, 1.2, 3), (1, 1, 1.0, 0), (1, 256, 1.3, 2), (0, 40, 1.2, 3), (0, 40, 1.0, 0)):
        sp = capi.SampleParams(0.9, 0.9, rep, top_k, ngram, do_sample, -1, 0, 1234)
        res = []
        for slots in (False, True):
            logits = base.clone().to(dev)
            st = _state(dev, R, cap, hist0, hl0, [3] * R, out_cap=8)
            step1 = torch.full((1,), 3, dtype=torch.int32, device=dev)
            for _ in range(2):
                if slots:
                    _slots_call(ops, logits, sp, st, workspace=wsp)
                else:
                    ops.sample_logits(logits, st["history"], st["hist_len"], sp, step1, st["cur"], st["pos"], st["finished"], st["out"],
                                      advance_pos=True, workspace=wsp)
            torch.cuda.synchronize()
            assert (st["step"].tolist() == [5] * R) if slots else (step1.item() == 5)
            if two_stage:
                assert int(wsp[:64 + 4 * R].sum().item()) == 0  # ticket and overflow words back to zero
            res.append([logits.cpu()] + [st[k].cpu() for k in ("history", "hist_len", "cur", "pos", "out", "finished")])
        a, b = res
        assert torch.equal(torch.isinf(a[0]), torch.isinf(b[0]))
        assert torch.equal(torch.nan_to_num(a[0], neginf=0.0), torch.nan_to_num(b[0], neginf=0.0)), (do_sample, top_k)
        for x, y, nm in zip(a[1:], b[1:], ("history", "hist_len", "cur", "pos", "out", "finished")):
            assert torch.equal(x, y), (nm, do_sample, top_k, rep, ngram)
        assert not b[6].any() and (b[4] == 2).all()


# ------------------------------------------------------------------------------------------------
# 3. inert and ending slots
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_stage", [False, True], ids=["one_stage", "two_stage"])
def test_inert_and_ending_slots(gpu, two_stage):
    from tcavt_amd import capi, ops

    dev = gpu["device"]
    fx = dict(np.load(os.path.join(GOLDEN, "tiny_generation.npz"), allow_pickle=False))
    R, V = fx["scores"].shape
    cap = fx["hist"].shape[1] + 4
    greedy = fx["scores"].argmax(1)
    eos, pad = int(greedy[2]), 9
    assert int((greedy == eos).sum()) == 1 and pad not in greedy.tolist()  # slot 2 alone draws EOS
    steps = [4, 4, 0, 7, 2, 1]
    st = _state(dev, R, cap, np.maximum(fx["hist"], 0), fx["hist_len"], steps, out_cap=16, sentinel=-5)
    st["finished"][0] = 1            # slot 0: inert from the start
    st["max_new"][1] = 5             # slot 1: step + 1 == max_new -> writes its token, then ends
    st["pos"] += torch.arange(R, dtype=torch.int32, device=dev) * 3 + 2
    before = {k: v.clone() for k, v in st.items()}
    sp = capi.SampleParams(0.9, 0.9, 1.0, 40, 0, 0, eos, pad, 1)  # greedy, processors off
    wsp = ops.sample_workspace(R, dev) if two_stage else None
    _slots_call(ops, torch.from_numpy(fx["scores"]).to(dev).clone(), sp, st, workspace=wsp)
    torch.cuda.synchronize()
    # slot 0: only cur_tok is written
    assert int(st["cur"][0]) == pad and (st["out"][0] == -5).all()
    for k in ("history", "hist_len", "step", "pos"):
        assert torch.equal(st[k][0], before[k][0]), k
    # slots 1 .. 5 draw their arg-max; 1 ends on its budget, 2 on EOS, the others go on
    for s in range(1, R):
        hl = int(fx["hist_len"][s])
        assert int(st["out"][s, steps[s]]) == int(st["cur"][s]) == int(st["history"][s, hl]) == int(greedy[s])
        assert int(st["step"][s]) == steps[s] + 1 and int(st["hist_len"][s]) == hl + 1 and int(st["pos"][s]) == int(before["pos"][s]) + 1
    assert st["finished"].tolist() == [1, 1, 1, 0, 0, 0]
    # the next call leaves the two ended slots untouched as well
    mid = {k: v.clone() for k, v in st.items()}
    _slots_call(ops, torch.from_numpy(fx["scores"]).to(dev).clone(), sp, st, workspace=wsp)
    torch.cuda.synchronize()
    for s in (0, 1, 2):
        assert int(st["cur"][s]) == pad
        for k in ("history", "hist_len", "step", "pos", "out", "finished"):
            assert torch.equal(st[k][s], mid[k][s]), (s, k)
    for s in (3, 4, 5):
        assert int(st["step"][s]) == steps[s] + 2 and int(st["out"][s, steps[s] + 1]) == int(st["cur"][s])
    assert int((st["out"] != -5).sum()) == 2 + 2 * 3
    if two_stage:
        assert int(wsp[:64 + 4 * R].sum().item()) == 0


# ------------------------------------------------------------------------------------------------
# 4. admission is a byte copy
# ------------------------------------------------------------------------------------------------
GUARD = 256


def _guarded(dev, shape, fill=None, gen=None):
    """uint8 tensor of `shape` inside a buffer with GUARD bytes in front and behind -> (whole buffer, view of the middle)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    if gen is not None:
        buf[GUARD:GUARD + n] = torch.randint(0, 256, (n,), generator=gen, dtype=torch.uint8).to(dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


@pytest.mark.parametrize("form", ["fp16", "bf16", "kv8"])
def test_admit_is_a_byte_copy(gpu, form):
    from tcavt_amd import capi, ops

    dev = gpu["device"]
    layers, S, nkv, src_lmax, kv_lmax, rows, slot = 2, 3, 2, 40, 72, 36, 1
    gen = torch.Generator().manual_seed(7)
    if form == "kv8":
        per = (64, 2, 64, 2)
        src = [_guarded(dev, (layers, 1, nkv, src_lmax, p), gen=gen) for p in per]
        dst = [_guarded(dev, (layers, S, nkv, kv_lmax, p)) for p in per]
        src_t, dst_t = [v for _, v in src], [v for _, v in dst]
    else:
        dt = torch.float16 if form == "fp16" else torch.bfloat16
        src = [_guarded(dev, (layers, 1, src_lmax, nkv * 64 * 2), gen=gen) for _ in range(2)]
        dst = [_guarded(dev, (layers, S, kv_lmax, nkv * 64 * 2)) for _ in range(2)]
        src_t, dst_t = [v.view(dt) for _, v in src], [v.view(dt) for _, v in dst]
    want = []
    for (db, dv), (_, sv) in zip(dst, src):
        w = dv.clone()
        if form == "kv8":
            w[:, slot, :, :rows] = sv[:, 0, :, :rows]
        else:
            w[:, slot, :rows] = sv[:, 0, :rows]
        full = db.clone()
        full[GUARD:GUARD + w.numel()] = w.reshape(-1)
        want.append(full)
    i32, i64 = torch.int32, torch.int64
    n_ids, cap = 20, 33
    prompt = torch.randint(0, 512, (n_ids,), generator=gen).to(dev)
    kv_len = torch.tensor([27], dtype=i32, device=dev)
    st = dict(history=torch.full((S, cap), -3, dtype=i64, device=dev), hist_len=torch.full((S,), 11, dtype=i32, device=dev),
              step=torch.full((S,), 12, dtype=i32, device=dev), max_new=torch.full((S,), 13, dtype=i32, device=dev),
              out_row=torch.full((S,), 14, dtype=i64, device=dev), pos=torch.full((S,), 15, dtype=i32, device=dev),
              finished=torch.full((S,), 1, dtype=i32, device=dev), cur_tok=torch.full((S,), 17, dtype=i64, device=dev))
    before = {k: v.clone() for k, v in st.items()}
    ops.slot_admit(src_t, dst_t, slot, rows, src_lmax, kv_lmax, layers, S, nkv, prompt, kv_len, 16, 50, 123456789012, **st)
    torch.cuda.synchronize()
    for (db, _), w in zip(dst, want):
        assert torch.equal(db, w)  # the copied rows are the source's; every other byte, guards included, is unchanged
    assert torch.equal(st["history"][slot, :n_ids], prompt) and (st["history"][slot, n_ids:] == -3).all()
    got = {k: int(st[k][slot]) for k in ("hist_len", "pos", "step", "finished", "max_new", "out_row", "cur_tok")}
    assert got == dict(hist_len=27 - 16, pos=27, step=0, finished=0, max_new=50, out_row=123456789012, cur_tok=17)
    for k in st:
        for s in (0, 2):
            assert torch.equal(st[k][s], before[k][s]), (k, s)
    # the two forms together are refused, and nothing is written
    other = [_guarded(dev, (64,))[1] for _ in range(8)]
    a = capi.SlotAdmitArgs()
    names16 = ("src_k", "src_v", "dst_k", "dst_v")
    names8 = ("src_k_codes", "src_k_scales", "src_v_codes", "src_v_scales", "dst_k_codes", "dst_k_scales", "dst_v_codes", "dst_v_scales")
    if form == "kv8":
        mine = dict(zip(names8, [src_t[0], src_t[1], src_t[2], src_t[3], dst_t[0], dst_t[1], dst_t[2], dst_t[3]]))
        extra = dict(zip(names16, other))
    else:
        mine = dict(zip(names16, src_t + dst_t))
        extra = dict(zip(names8, other))
    for k, v in {**mine, **extra}.items():
        setattr(a, k, v.data_ptr())
    for k, v in st.items():
        setattr(a, k, v.data_ptr())
    a.prompt_ids, a.kv_len = prompt.data_ptr(), kv_len.data_ptr()
    a.n_layers, a.S, a.slot, a.rows, a.src_lmax, a.kv_lmax, a.nkv, a.dtype16 = layers, S, 2, rows, src_lmax, kv_lmax, nkv, capi.F16
    a.n_ids, a.hist_cap, a.n_image, a.max_new_value, a.out_row_value = n_ids, cap, 16, 5, 1
    after = {k: v.clone() for k, v in st.items()}
    assert capi.lib().tcavt_slot_admit(ctypes.byref(a), capi.stream_ptr()) == 1
    assert b"exclude each other" in capi.lib().tcavt_last_error()
    torch.cuda.synchronize()
    for (db, _), w in zip(dst, want):
        assert torch.equal(db, w)
    for k in st:
        assert torch.equal(st[k], after[k]), k


# ------------------------------------------------------------------------------------------------
# 5. the reference model's own continuation, through a refill
# ------------------------------------------------------------------------------------------------
def test_pool_reproduces_the_reference_continuation_through_a_refill(gpu):
    M = _setup(gpu["device"])
    fx, N, EOS, PAD = M["fx"], 12, 268, 7
    for key in ("greedy_tokens", "greedy_proc_tokens"):
        ref = fx[key]
        assert ref.shape[1] >= N and int(ref[0, 2]) == EOS and EOS not in ref[0, :2].tolist()
        assert EOS not in ref[1].tolist() and EOS not in ref[2].tolist() and PAD not in ref.reshape(-1).tolist()
    for key, proc in (("greedy_tokens", dict(repetition_penalty=1.0, no_repeat_ngram_size=0)),
                      ("greedy_proc_tokens", dict(repetition_penalty=1.2, no_repeat_ngram_size=3))):
        want = fx[key][:, :N].copy()
        want[0, 3:] = PAD
        outs = []
        for use_graph in (False, True):
            for poll_every in (1, 5):
                out = _pool(M, max_new_tokens=N, slots=2, poll_every=poll_every, do_sample=False, eos_token_id=EOS, pad_token_id=PAD,
                            use_graph=use_graph, **proc)
                M["m"].mllm.check_flags()
                stats = M["m"].mllm.pool_stats
                assert out.dtype == torch.int64 and tuple(out.shape) == (3, N)
                # request 0 ends after three tokens and request 2 takes its slot while request 1 is mid-answer
                adm = {r: (s, at) for r, s, at in stats["admitted"]}
                assert adm[0] == (0, 0) and adm[1] == (1, 0) and adm[2][0] == 0 and 2 <= adm[2][1] < N - 1, (stats, poll_every)
                outs.append(out)
        for out in outs:
            assert np.array_equal(out.numpy(), want), key  # margins >= 0.1 against a 2e-3 logit bar: bit-equality


# ------------------------------------------------------------------------------------------------
# 6. independence from the schedule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(), dict(kv_cache="fp8"), dict(decode_weights="fp8", kv_cache="fp8")],
                         ids=["fp16", "kv8", "w8_kv8"])
def test_a_request_does_not_depend_on_the_schedule(gpu, opts):
    M = _setup(gpu["device"])
    kw = dict(slots=2, do_sample=True, seed=5, **opts)
    a = _pool(M, max_new_tokens=[12, 12, 12], **kw)
    adm_a = list(M["m"].mllm.pool_stats["admitted"])
    b = _pool(M, max_new_tokens=[3, 12, 12], **kw)
    adm_b = list(M["m"].mllm.pool_stats["admitted"])
    M["m"].mllm.check_flags()
    # request 2 enters at another time, and in the second run beside request 1 mid-answer instead of an ended one
    assert adm_a[2][0] == adm_b[2][0] == 2 and adm_b[2][2] < adm_a[2][2] and adm_b[2][2] < 11 <= adm_a[2][2]
    assert tuple(a.shape) == tuple(b.shape) == (3, 12)
    assert torch.equal(a[1:], b[1:])
    assert torch.equal(a[0, :3], b[0, :3]) and (b[0, 3:] == 0).all()
    assert ((a >= 0) & (a < M["cfg"].llama.vocab)).all()
    a2 = _pool(M, max_new_tokens=[12, 12, 12], **kw)
    assert torch.equal(a, a2)
    c = _pool(M, max_new_tokens=[12, 12, 12], **{**kw, "seed": 6})
    assert not torch.equal(a, c)


# ------------------------------------------------------------------------------------------------
# 7. a refilled slot against the oracle
# ------------------------------------------------------------------------------------------------
def test_refilled_slot_logits_match_oracle(gpu):
    """Budgets [2, 9, 7] on two slots, poll_every = 1: request 0 ends in step 1 (the eager, unpolled one), is seen ended after
    step 2, request 2 takes slot 0 and chooses its tokens 2 .. 7 in steps 3 .. 8 -- it ends last, together with request 1 (tokens
    2 .. 9 in steps 1 .. 8), so its slot's logits row is the one its 7th token was chosen from.  The bar is that of
    test_decode_step_logits_match_oracle_on_growing_sequence (tests/test_generation_gpu.py)."""
    from oracle import generation as G

    dev = gpu["device"]
    M = _setup(dev)
    cfg, weights, t = M["cfg"], M["weights"], M["t"]
    out = _pool(M, max_new_tokens=[2, 9, 7], slots=2, poll_every=1, do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0)
    M["m"].mllm.check_flags()
    stats = M["m"].mllm.pool_stats
    adm = {r: (s, at) for r, s, at in stats["admitted"]}
    assert adm[2][0] == adm[0][0] and adm[2][1] > 0  # a reused slot
    ret = {r: at for r, s, at in stats["retired"]}
    assert ret[2] == stats["steps"] == max(ret.values()) and ret[0] < ret[2]  # it ends last
    assert np.array_equal(out[2, :7].numpy(), M["fx"]["greedy_tokens"][2, :7]) and (out[2, 7:] == 0).all() and (out[0, 2:] == 0).all()
    logits = M["m"].mllm._ws.get("pool.logits", (2, cfg.llama.vocab), torch.float32, dev).cpu()
    b = 2
    n_text = int(t["attention_mask"][b].sum())
    seq = G.prefix_embeds(weights, cfg, t["vision_emb"], t["input_ids"], "fp16", b, n_text)
    for tok in out[b, :6]:
        seq = torch.cat([seq, G.token_embed(weights, tok, "fp16")[None, None]], dim=1)
    with torch.no_grad():
        ref = G.next_logits(weights, cfg, seq, "fp16")
    e = rel_err(logits[adm[2][0]], ref)
    print(f"refilled slot logits vs oracle: rel_err = {e:.3e}")
    assert e < 2e-3, e
    assert int(ref.argmax()) == int(out[b, 6])


# ------------------------------------------------------------------------------------------------
# 8. generate_batch is untouched
# ------------------------------------------------------------------------------------------------
def test_generate_batch_after_a_pool_run_is_unchanged(gpu):
    M = _setup(gpu["device"])
    g, fx = M["g"], M["fx"]
    _pool(M, max_new_tokens=[4, 6, 5], slots=2, do_sample=True, seed=3)
    N = fx["greedy_tokens"].shape[1]
    out = M["m"].mllm.generate_batch(g["vision_emb"], None, max_new_tokens=N, input_ids=g["input_ids"], attention_mask=g["attention_mask"],
                                     do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0)
    torch.cuda.synchronize()
    M["m"].mllm.check_flags()
    assert np.array_equal(out.cpu().numpy(), fx["greedy_tokens"])
