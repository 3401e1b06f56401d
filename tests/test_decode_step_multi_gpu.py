"""tcavt_llama_decode_step_multi called directly (capi.DecodeArgs, buffers owned by the test): R = S * T rows, T consecutive
positions of each of S sequences on one cache per sequence.

Model, caches and habits of test_decode_step_gpu.py (its helpers are imported): hidden 256, inter 512, 2 layers, 8 / 2 heads, vocab
512, LoRA r 8, kv_lmax = 200; per sequence base from {0, 63, 64, 130, 200 - T}; cache rows below base random, every row from base on
a decoy (K = 4 * a real row, V = +-30000); NaN guard rows around both caches and the logits.  Cases (S, T): (1, 2), (2, 4) -- 8 rows:
the 8-row activation block --, (3, 5), (4, 8) and (8, 4) -- 32 rows --, each on row-major and on fragment-major weights and
activations; FP8 weights at (2, 4) and (4, 8).

Asserted per case:
- logits of row (s, j) within LOGIT_BAR = 2e-3 (relative to the row's norm) of oracle/decode.py in float64 stepped j + 1 times with
  the drafts teacher-forced (every step appends its k | v to the oracle's cache); arg-max equal wherever the reference's top-two gap
  exceeds twice the bar -- that set comes from the reference alone and covers >= 90 % of the rows;
- bit-equality with the plain step at the same row count: T calls of tcavt_llama_decode_step at B = R on a cache [layers, R, ...] in
  which the T rows of a sequence are copies of its cache, call j feeding every row of s the token of offset j at base + j: call j's
  logits of every row of s are the bits of multi row (s, j), and after the T calls the copies' cache rows are the multi cache's;
- in every layer's cache the rows outside base .. base + T - 1 and all guards keep their bits; flags stay 0; cur_tok / pos unchanged.

Measured, not asserted (test_row_count_independence): whether a row's plain-step logits are bit-independent of the row count, B = S
against B = R with the same token in the same row.  The answer is printed and recorded in profiles/generate_prompt_lookup.txt; the
sampled end-to-end comparison of test_prompt_lookup_generate_gpu.py rests on it.
"""
import ctypes

import pytest
import torch

import test_decode_step_gpu as DS

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
KV_LMAX, LOGIT_BAR, GUARD = DS.KV_LMAX, DS.LOGIT_BAR, DS._GUARD
CASES = [(1, 2), (2, 4), (3, 5), (4, 8), (8, 4)]
_cache = {}


def _bases(S, T):
    all_b = [0, 63, 64, 130, KV_LMAX - T]
    return [all_b[(s + T) % 5] for s in range(S)]


def _inputs(S, T):
    """tokens [S, T], bases [S] and the caches [layers, S, KV_LMAX, w] (CPU, fp16)"""
    ll = DS._cfg().llama
    w = ll.n_kv_heads * ll.head_dim
    g = torch.Generator().manual_seed(500 + 10 * S + T)
    tok = torch.randint(0, ll.vocab, (S, T), generator=g)
    base = torch.tensor(_bases(S, T))
    kc = torch.randn(ll.layers, S, KV_LMAX, w, generator=g)
    vc = torch.randn(ll.layers, S, KV_LMAX, w, generator=g)
    j = torch.arange(KV_LMAX)
    behind = (j[None, :] >= base[:, None])[None, :, :, None]
    src = j[None, :] % base.clamp_min(1)[:, None]
    kc = torch.where(behind, 4 * torch.gather(kc, 2, src[None, :, :, None].expand_as(kc)), kc)
    sign = (torch.randint(0, 2, vc.shape, generator=g) * 2 - 1).float()
    vc = torch.where(behind, 30000.0 * sign, vc)
    return tok, base, kc.to(F16), vc.to(F16)


def _reference(S, T, fp8=False):
    """float64 logits [S * T, V]: the oracle stepped T times, teacher-forced, appending to its own cache -- computed once"""
    from oracle import decode as D

    key = ("ref", S, T, fp8)
    if key not in _cache:
        cfg = DS._cfg()
        ll = cfg.llama
        pkey = ("wp", "fp16", fp8)
        if pkey not in DS._cache:
            DS._cache[pkey] = D.prepare(DS._weights(cfg), cfg, "fp16", weight_map=DS._fp8_map if fp8 else None)
        Wp = DS._cache[pkey]
        tok, base, kc, vc = _inputs(S, T)
        view = lambda c: [c[li].double().view(S, KV_LMAX, ll.n_kv_heads, ll.head_dim).clone() for li in range(ll.layers)]
        kv, vv = view(kc), view(vc)
        rows = []
        ar = torch.arange(S)
        with torch.no_grad():
            for j in range(T):
                logits, new_kv = D.decode_step(Wp, cfg, D.token_embeds(Wp, tok[:, j]), base + j, kv, vv, "fp16")
                rows.append(logits)
                for li, (k, v) in enumerate(new_kv):
                    kv[li][ar, base + j] = k
                    vv[li][ar, base + j] = v
        _cache[key] = torch.stack(rows, 1).reshape(S * T, -1)
    return _cache[key]


def _run(dev, B, T, tok, pos, kbuf, kc, vbuf, vc, wl, al, fp8, what):
    """one decode step at B rows on the given (guarded) caches: T = 0 the plain entry, else the multi entry.  -> logits [B, V]"""
    from tcavt_amd import capi

    m = DS._model("fp16", dev)
    ll = DS._cfg().llama
    LW = m.mllm.llama_wrapper
    PL, P = LW._prepared(), m.mllm._prepared()
    st = LW.storage
    H, I, nq, nkv, V, nL = ll.hidden, ll.inter, ll.n_q_heads, ll.n_kv_heads, ll.vocab, ll.layers
    nqkv = (nq + 2 * nkv) * 64
    tok_d, pos_d = tok.to(dev), pos.to(torch.int32).to(dev)
    tok0, pos0 = tok_d.clone(), pos_d.clone()
    Br = B if al == 0 else 8 if al == 2 else 16 if B <= 16 else 32
    z = lambda *shape, dt=st: torch.zeros(*shape, dtype=dt, device=dev)
    bufs = dict(h16=z(Br, H), part=z(B, H // 16, dt=F32), qkv=z(B, nqkv), att=z(Br, nq * 64), act=z(Br, I), t=z(B, 64), x16=z(Br, H))
    logits = torch.full((B + 2, V), float("nan"), dtype=F32, device=dev)
    flags = torch.zeros(3, dtype=torch.int32, device=dev)
    cos, sin = LW._rope_tables(KV_LMAX, dev)
    a = capi.DecodeArgs()
    for k_, v_ in bufs.items():
        setattr(a, k_, v_.data_ptr())
    a.layers, a.gamma_final = PL.carr, PL.g_final.data_ptr()
    keep = None
    if wl != 0:
        keep = LW.decode_weights("fp8" if fp8 else "fp16")
        assert keep is not None
        a.layers, a.table_packed, a.w_layout = keep.carr, keep.table.data_ptr(), wl
    a.act_layout = al
    a.rope_cos, a.rope_sin, a.rope_L = cos.data_ptr(), sin.data_ptr(), KV_LMAX
    a.table, a.txt_mod = PL.table.data_ptr(), P.txt.data_ptr()
    a.cur_tok, a.pos = tok_d.data_ptr(), pos_d.data_ptr()
    a.k_cache, a.v_cache, a.kv_lmax = kc.data_ptr(), vc.data_ptr(), KV_LMAX
    a.logits, a.bad_id_flag, a.nonfinite_flag = logits[1:].data_ptr(), flags.data_ptr(), flags[2:3].data_ptr()
    lp = torch.zeros(B * H, dtype=F32, device=dev)
    a.lora_part, a.lora_rank = lp.data_ptr(), LW.lora_r
    a.n_layers, a.B, a.H, a.I, a.nq, a.nkv, a.V = nL, B, H, I, nq, nkv, V
    a.dtype16 = capi.F16
    a.rms_eps, a.lora_scale = ll.rms_eps, LW.lora_alpha / LW.lora_r
    a.stream_scale = float(LW.stream_scale)
    k_guard, v_guard = (kbuf[:GUARD].clone(), kbuf[-GUARD:].clone()), (vbuf[:GUARD].clone(), vbuf[-GUARD:].clone())
    if T:
        rc = capi.lib().tcavt_llama_decode_step_multi(ctypes.byref(a), T, capi.stream_ptr())
    else:
        rc = capi.lib().tcavt_llama_decode_step(ctypes.byref(a), capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, what)
    assert flags.tolist() == [0, 0, 0], f"{what}: bad_id / nonfinite flags {flags.tolist()}"
    assert torch.equal(tok_d, tok0) and torch.equal(pos_d, pos0), f"{what}: cur_tok / pos modified"
    assert bool(torch.isnan(logits[0]).all()) and bool(torch.isnan(logits[B + 1]).all()), f"{what}: write outside logits"
    for buf, (lo, hi), nm in ((kbuf, k_guard, "k_cache"), (vbuf, v_guard, "v_cache")):
        assert torch.equal(DS._bits(buf[:GUARD]), DS._bits(lo)) and torch.equal(DS._bits(buf[-GUARD:]), DS._bits(hi)), \
            f"{what}: write into the guard rows of {nm}"
    got = logits[1:B + 1].clone()
    assert torch.isfinite(got).all(), f"{what}: non-finite logits"
    del keep, lp
    return got


def _caches(dev, kc0, vc0):
    nL, n, _, w = kc0.shape
    kbuf, kc = DS._guarded(kc0.reshape(nL * n * KV_LMAX, w).to(dev))
    vbuf, vc = DS._guarded(vc0.reshape(nL * n * KV_LMAX, w).to(dev))
    return kbuf, kc, vbuf, vc


def _multi(dev, S, T, wl, al, fp8=False):
    tok, base, kc0, vc0 = _inputs(S, T)
    kbuf, kc, vbuf, vc = _caches(dev, kc0, vc0)
    pos_rows = (base[:, None] + torch.arange(T)[None, :]).reshape(-1)
    what = f"multi S={S} T={T}{' fp8' if fp8 else ''} w_layout={wl} act_layout={al}"
    got = _run(dev, S * T, T, tok.reshape(-1), pos_rows, kbuf, kc, vbuf, vc, wl, al, fp8, what)
    nL, w = kc0.shape[0], kc0.shape[-1]
    kc, vc = kc.view(nL, S, KV_LMAX, w), vc.view(nL, S, KV_LMAX, w)
    for s, b in enumerate(base.tolist()):  # the rows outside base .. base + T - 1 keep their bits
        keep = torch.ones(KV_LMAX, dtype=torch.bool, device=dev)
        keep[b:b + T] = False
        for c, c0, nm in ((kc, kc0, "k_cache"), (vc, vc0, "v_cache")):
            assert torch.equal(DS._bits(c[:, s][:, keep]), DS._bits(c0.to(dev)[:, s][:, keep])), f"{what}: {nm} of sequence {s}: a row outside the block was written"
            assert torch.isfinite(c[:, s, b:b + T]).all(), f"{what}: {nm} rows of the block"
    return got, kc.clone(), vc.clone(), what


def _plain_same_row_count(dev, S, T, wl, al, fp8=False):
    """T plain steps at B = R on T copies of every sequence's cache -> ([T] logits [R, V], k cache, v cache [layers, R, ...])"""
    tok, base, kc0, vc0 = _inputs(S, T)
    kbuf, kc, vbuf, vc = _caches(dev, kc0.repeat_interleave(T, dim=1), vc0.repeat_interleave(T, dim=1))
    outs = []
    for j in range(T):
        what = f"plain call {j} at B={S * T} w_layout={wl} act_layout={al}"
        outs.append(_run(dev, S * T, 0, tok[:, j].repeat_interleave(T), (base + j).repeat_interleave(T), kbuf, kc, vbuf, vc, wl, al, fp8, what))
    nL, w = kc0.shape[0], kc0.shape[-1]
    return outs, kc.view(nL, S * T, KV_LMAX, w), vc.view(nL, S * T, KV_LMAX, w)


def _pairs(R, fp8):
    from tcavt_amd import capi

    al = 2 if R <= 8 else 1
    return [(capi.W_FRAG8, al)] if fp8 else [(0, 0), (capi.W_FRAG16, al)]


def _check(dev, S, T, fp8):
    ref = _reference(S, T, fp8)
    qual, amax = DS._qualifying(ref)
    R = S * T
    assert float(qual.sum()) >= 0.9 * R, (S, T, int(qual.sum()))
    for wl, al in _pairs(R, fp8):
        got, kc, vc, what = _multi(dev, S, T, wl, al, fp8)
        g = got.cpu().double()
        e = (g - ref).norm(dim=-1) / ref.norm(dim=-1)
        print(f"[decode step multi] {what}: logits rel worst {e.max().item():.2e} (bar {LOGIT_BAR:.0e}); {int(qual.sum())} of {R} rows qualify")
        assert bool((e < LOGIT_BAR).all()), f"{what}: logits rel {e.tolist()}"
        assert torch.equal(g.argmax(-1)[qual], amax[qual]), f"{what}: arg-max differs on a qualifying row"
        outs, kcp, vcp = _plain_same_row_count(dev, S, T, wl, al, fp8)
        for j in range(T):
            want = outs[j].view(S, T, -1)  # every copy of sequence s computed offset j
            have = got.view(S, T, -1)[:, j]
            for c in range(T):
                bad = DS._bits(want[:, c]) != DS._bits(have)
                assert not bool(bad.any()), f"{what}: row (s, {j}) differs from plain call {j}, copy {c}, at (s, column) {tuple(bad.nonzero()[0].tolist())}"
        for c in range(T):
            assert torch.equal(DS._bits(kcp[:, c::T]), DS._bits(kc)) and torch.equal(DS._bits(vcp[:, c::T]), DS._bits(vc)), \
                f"{what}: the caches differ from the plain calls' (copy {c})"


def test_reference_gaps_cover_the_rows():
    """from the reference alone"""
    for S, T in CASES:
        qual, _ = DS._qualifying(_reference(S, T))
        assert float(qual.sum()) >= 0.9 * S * T, (S, T, int(qual.sum()))
        assert all(b + T <= KV_LMAX for b in _bases(S, T))
    assert {b for S, T in CASES for b in _bases(S, T)} >= {0, 63, 64, 130, KV_LMAX - 8, KV_LMAX - 4}


@pytest.mark.parametrize("S,T", CASES)
def test_fp16(gpu, S, T):
    _check(gpu["device"], S, T, False)


@pytest.mark.parametrize("S,T", [(2, 4), (4, 8)])
def test_fp8_weights(gpu, S, T):
    _check(gpu["device"], S, T, True)


def test_row_count_independence(gpu):
    """measured, not asserted: plain-step logits of a row at B = S against the same token in the same row at B = S * T"""
    from tcavt_amd import capi

    dev = gpu["device"]
    for S, T in [(1, 4), (2, 4), (4, 4), (8, 4), (1, 8), (4, 8)]:
        for wl, al_of in ((0, lambda B: 0), (capi.W_FRAG16, lambda B: 2 if B <= 8 else 1)):
            tok, base, kc0, vc0 = _inputs(S, T)
            R = S * T
            g = torch.Generator().manual_seed(S * 100 + T)
            tok_R = torch.cat([tok[:, 0], torch.randint(0, 512, (R - S,), generator=g)])
            pos_R = torch.cat([base, base.repeat(T)[:R - S]])
            kR = torch.cat([kc0] + [kc0] * (T - 1), dim=1)
            vR = torch.cat([vc0] + [vc0] * (T - 1), dim=1)
            small = _run(dev, S, 0, tok[:, 0], base, *_caches(dev, kc0, vc0), wl, al_of(S), False, f"B={S}")
            large = _run(dev, R, 0, tok_R, pos_R, *_caches(dev, kR, vR), wl, al_of(R), False, f"B={R}")[:S]
            same = torch.equal(DS._bits(small), DS._bits(large))
            d = (small.double() - large.double()).norm(dim=-1) / small.double().norm(dim=-1)
            print(f"[row count] w_layout={wl}: B={S} vs B={R}: logits {'bit-equal' if same else 'DIFFER'}; rel worst {d.max().item():.2e}; "
                  f"arg-max equal on {int((small.argmax(-1) == large.argmax(-1)).sum())} of {S} rows")
