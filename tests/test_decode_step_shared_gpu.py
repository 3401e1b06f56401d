"""tcavt_llama_decode_step_shared called directly (capi.DecodeArgs + capi.KvPrefix, buffers owned by the test) against the float64
reference of tests/test_decode_step_gpu.py, whose model (hidden 256, inter 512, 2 layers, 8 / 2 heads, vocab 512, LoRA r 8), bar
and helpers it imports.

The rows are n continuations of each of Bp prompts.  The prompts' cache [layers, Bp, PL = 70, nkv * 64] holds random rows below a
ragged prefix_len (70, 33, 1, 64: full, across a 32-key tile edge, one key, a tile edge) and decoys (K = 4 * a real row, V =
+-30000) behind it; every row's suffix cache [layers, R, SL = 6, nkv * 64] holds random rows below its slot t (ragged: 0, 5, 1, 3,
...) and decoys from t on; pos = prefix_len + t.  NaN guard rows lie around all four buffers.

Reference: oracle/decode.py in float64 on the concatenated cache, row r = [prefix rows < prefix_len | suffix rows < t], from the
CPU alone, computed once per shape.  Asserted per form: every row's logits within LOGIT_BAR = 2e-3 of the row norm; arg-max equal
wherever the reference's own top-two gap exceeds twice the bar (that set covers >= 90 % of the rows: test_reference_gaps_cover_the
_rows, which needs no GPU code); at fixed shape, logits and suffix caches bit-equal across the legal (w_layout, act_layout) pairs;
the prefix and all guards keep their bits; in every layer's suffix cache all rows but t keep their bits and the last layer's row t
is the qkv buffer's k | v; flags stay 0; pos and cur_tok are unchanged.  Shapes (prompts x n): 2 x 4, 3 x 3, 4 x 8 on their legal
pairs, FP8 weights at 4 x 8, and the three refusals of the entry (kv8 planes, B % n, rope_L) plus a null prefix.

Measured on an MI355X: worst per-row logit error 9.7e-4 (2 x 4), 7.8e-4 (3 x 3), 9.1e-4 (4 x 8), 1.07e-3 with FP8 weights, the
same on every layout pair; every row qualifies for the arg-max check.  (The unshared step sits at 5.5e-4 .. 6.9e-4 against the same
oracle: the oracle rounds a probability relative to the final sum, as tcavt_attn_decode does, this kernel relative to the running
maximum, as the prefill kernels do.)
"""
import ctypes

import pytest
import torch

import test_decode_step_gpu as ds
from test_decode_step_gpu import F16, F32, LOGIT_BAR, _bits, _cfg, _guarded, _model, _pairs, _qualifying

pytestmark = pytest.mark.gpu

PL, SL = 70, 6
_GUARD = ds._GUARD
_cache = {}
SHAPES = [(2, 4), (3, 3), (4, 8)]


def _plen(Bp):
    return [70, 33, 1, 64][:Bp]


def _slots(R):
    base = [0, SL - 1, 1, 3]
    return [base[r] if r < len(base) else (r * 3 + 1) % SL for r in range(R)]


def _inputs(Bp, n, dt):
    """tokens, prefix_len, slots and the four caches (CPU): random rows where valid, decoys behind"""
    ll = _cfg().llama
    w, R = ll.n_kv_heads * ll.head_dim, Bp * n
    g = torch.Generator().manual_seed(700 + 10 * Bp + n)
    tok = torch.randint(0, ll.vocab, (R,), generator=g)
    plen, t = torch.tensor(_plen(Bp)), torch.tensor(_slots(R))

    def cache(rows, lmax, valid):
        k = torch.randn(ll.layers, rows, lmax, w, generator=g)
        v = torch.randn(ll.layers, rows, lmax, w, generator=g)
        j = torch.arange(lmax)
        behind = (j[None, :] >= valid[:, None])[None, :, :, None]
        src = j[None, :] % valid.clamp_min(1)[:, None]
        k = torch.where(behind, 4 * torch.gather(k, 2, src[None, :, :, None].expand_as(k)), k)
        sign = (torch.randint(0, 2, v.shape, generator=g) * 2 - 1).float()
        return k.to(dt), torch.where(behind, 30000.0 * sign, v).to(dt)

    pk, pv = cache(Bp, PL, plen)
    sk, sv = cache(R, SL, t)
    return tok, plen, t, pk, pv, sk, sv


def _reference(Bp, n, fp8=False):
    """float64 logits [R, V] from the CPU alone, computed once"""
    from oracle import decode as D

    key = (Bp, n, fp8)
    if key not in _cache:
        cfg = _cfg()
        st, ss, contract = ds.CONTRACTS["fp16"]
        Wp = ds._reference("fp16", 1, fp8)[2]  # the prepared weights of the unshared test (cached there)
        tok, plen, t, pk, pv, sk, sv = _inputs(Bp, n, st)
        ll, R = cfg.llama, Bp * n
        pos = plen.repeat_interleave(n) + t
        kc = torch.zeros(ll.layers, R, PL + SL, ll.n_kv_heads * ll.head_dim, dtype=st)
        vc = torch.zeros_like(kc)
        for r in range(R):
            b, p, tr = r // n, int(plen[r // n]), int(t[r])
            kc[:, r, :p], vc[:, r, :p] = pk[:, b, :p], pv[:, b, :p]
            kc[:, r, p:p + tr], vc[:, r, p:p + tr] = sk[:, r, :tr], sv[:, r, :tr]
        view = lambda c: [c[li].double().view(R, PL + SL, ll.n_kv_heads, ll.head_dim) for li in range(ll.layers)]
        with torch.no_grad():
            logits, _ = D.decode_step(Wp, cfg, D.token_embeds(Wp, tok), pos, view(kc), view(vc), contract)
        _cache[key] = logits
    return _cache[key]


def test_reference_gaps_cover_the_rows():
    """from the reference alone: at every shape the rows with a top-two gap above twice the bar are >= 90 %"""
    for Bp, n, fp8 in [(b, n, False) for b, n in SHAPES] + [(4, 8, True)]:
        qual, _ = _qualifying(_reference(Bp, n, fp8))
        assert float(qual.sum()) >= 0.9 * Bp * n, (Bp, n, fp8, int(qual.sum()))
        t = _slots(Bp * n)
        assert 0 in t and SL - 1 in t and all(1 <= p <= PL for p in _plen(Bp))


def _args(dev, Bp, n, wl, al, fp8=False):
    """capi.DecodeArgs + capi.KvPrefix on fresh guarded buffers; -> (a, px, everything that must stay alive / be inspected)"""
    from tcavt_amd import capi

    m = _model("fp16", dev)
    ll = _cfg().llama
    LW = m.mllm.llama_wrapper
    PLd, P = LW._prepared(), m.mllm._prepared()
    st = LW.storage
    H, I, nq, nkv, V, nL = ll.hidden, ll.inter, ll.n_q_heads, ll.n_kv_heads, ll.vocab, ll.layers
    w, nqkv, B = nkv * 64, (nq + 2 * nkv) * 64, Bp * n
    tok, plen, t, pk0, pv0, sk0, sv0 = _inputs(Bp, n, st)
    k = dict(tok=tok.to(dev), plen=plen.to(torch.int32).to(dev), t=t.to(dev))
    k["pos"] = (plen.repeat_interleave(n) + t).to(torch.int32).to(dev)
    for nm, c, rows in (("pk", pk0, Bp * PL), ("pv", pv0, Bp * PL), ("sk", sk0, B * SL), ("sv", sv0, B * SL)):
        k[nm + "_buf"], k[nm] = _guarded(c.view(nL * rows, w).to(dev))
    Br = B if al == 0 else 8 if al == 2 else 16 if B <= 16 else 32
    z = lambda *shape, dt=st: torch.zeros(*shape, dtype=dt, device=dev)
    bufs = dict(h16=z(Br, H), part=z(B, H // 16, dt=F32), qkv=z(B, nqkv), att=z(Br, nq * 64), act=z(Br, I), t=z(B, 64), x16=z(Br, H))
    k["bufs"] = bufs
    k["logits"] = torch.full((B + 2, V), float("nan"), dtype=F32, device=dev)
    k["flags"] = torch.zeros(3, dtype=torch.int32, device=dev)
    cos, sin = LW._rope_tables(PL + SL, dev)
    k["rope"] = (cos, sin)
    a = capi.DecodeArgs()
    for k_, v_ in bufs.items():
        setattr(a, k_, v_.data_ptr())
    a.layers, a.gamma_final = PLd.carr, PLd.g_final.data_ptr()
    if wl != 0:
        k["keep"] = LW.decode_weights("fp8" if fp8 else "fp16")
        a.layers, a.table_packed, a.w_layout = k["keep"].carr, k["keep"].table.data_ptr(), wl
    a.act_layout = al
    a.rope_cos, a.rope_sin, a.rope_L = cos.data_ptr(), sin.data_ptr(), PL + SL
    a.table, a.txt_mod = PLd.table.data_ptr(), P.txt.data_ptr()
    a.cur_tok, a.pos = k["tok"].data_ptr(), k["pos"].data_ptr()
    a.k_cache, a.v_cache, a.kv_lmax = k["sk"].data_ptr(), k["sv"].data_ptr(), SL
    a.logits, a.bad_id_flag, a.nonfinite_flag = k["logits"][1:].data_ptr(), k["flags"].data_ptr(), k["flags"][2:3].data_ptr()
    k["lp"] = torch.zeros(B * H, dtype=F32, device=dev)
    a.lora_part, a.lora_rank = k["lp"].data_ptr(), LW.lora_r
    a.n_layers, a.B, a.H, a.I, a.nq, a.nkv, a.V = nL, B, H, I, nq, nkv, V
    a.dtype16 = capi.F16 if st == F16 else capi.BF16
    a.rms_eps, a.lora_scale = ll.rms_eps, LW.lora_alpha / LW.lora_r
    a.stream_scale = float(LW.stream_scale)
    px = capi.KvPrefix(k["pk"].data_ptr(), k["pv"].data_ptr(), k["plen"].data_ptr(), n, PL)
    return a, px, k


def _step(dev, Bp, n, wl, al, fp8=False):
    from tcavt_amd import capi

    ll = _cfg().llama
    nq, nkv, nL, B = ll.n_q_heads, ll.n_kv_heads, ll.layers, Bp * n
    w = nkv * 64
    what = f"{Bp} x {n}{' fp8' if fp8 else ''} w_layout={wl} act_layout={al}"
    a, px, k = _args(dev, Bp, n, wl, al, fp8)
    before = {nm: k[nm].clone() for nm in ("pk_buf", "pv_buf", "sk_buf", "sv_buf", "tok", "pos", "plen")}
    rc = capi.lib().tcavt_llama_decode_step_shared(ctypes.byref(a), ctypes.byref(px), capi.stream_ptr())
    torch.cuda.synchronize()
    capi.check(rc, what)
    assert k["flags"].tolist() == [0, 0, 0], f"{what}: bad_id / nonfinite flags {k['flags'].tolist()}"
    for nm in ("tok", "pos", "plen"):
        assert torch.equal(k[nm], before[nm]), f"{what}: {nm} modified"
    for nm in ("pk_buf", "pv_buf"):
        assert torch.equal(_bits(k[nm]), _bits(before[nm])), f"{what}: the prefix ({nm}) was written"
    logits = k["logits"]
    assert bool(torch.isnan(logits[0]).all()) and bool(torch.isnan(logits[B + 1]).all()), f"{what}: write outside logits"
    got = logits[1:B + 1]
    assert torch.isfinite(got).all(), f"{what}: non-finite logits"
    at = torch.zeros(B, SL, dtype=torch.bool, device=dev)
    at[torch.arange(B, device=dev), k["t"]] = True
    at = at.view(1, B * SL).expand(nL, B * SL).reshape(-1)
    qkv = k["bufs"]["qkv"]
    for nm, col in (("sk", nq * 64), ("sv", (nq + nkv) * 64)):
        buf, b0, c = k[nm + "_buf"], before[nm + "_buf"], k[nm]
        assert torch.equal(_bits(buf[:_GUARD]), _bits(b0[:_GUARD])) and torch.equal(_bits(buf[-_GUARD:]), _bits(b0[-_GUARD:])), \
            f"{what}: write into the guard rows of {nm}"
        same = (_bits(c) == _bits(b0[_GUARD:-_GUARD])).all(-1)
        assert bool(same[~at].all()), f"{what}: a {nm} row other than t was written"
        rows_t = c.view(nL, B, SL, w)[:, torch.arange(B, device=dev), k["t"]]
        assert torch.isfinite(rows_t).all(), f"{what}: {nm} row t"
        assert torch.equal(_bits(rows_t[nL - 1]), _bits(qkv[:, col:col + w])), f"{what}: the last layer's {nm} row t is not the qkv buffer's bits"
    return dict(logits=got.clone(), sk=k["sk"].clone(), sv=k["sv"].clone(), what=what)


def _check_logits(res, Bp, n, fp8):
    ref = _reference(Bp, n, fp8)
    got = res["logits"].cpu().double()
    e = (got - ref).norm(dim=-1) / ref.norm(dim=-1)
    qual, amax = _qualifying(ref)
    print(f"[decode step shared] {res['what']}: logits rel worst {e.max().item():.2e} (bar {LOGIT_BAR:.0e}); {int(qual.sum())} of {Bp * n} rows qualify")
    assert bool((e < LOGIT_BAR).all()), f"{res['what']}: logits rel {e.tolist()}"
    assert float(qual.sum()) >= 0.9 * Bp * n
    assert torch.equal(got.argmax(-1)[qual], amax[qual]), f"{res['what']}: arg-max differs on a qualifying row"


def _run_pairs(dev, Bp, n, pairs, fp8=False):
    base = None
    for wl, al in pairs:
        res = _step(dev, Bp, n, wl, al, fp8=fp8)
        _check_logits(res, Bp, n, fp8)
        if base is None:
            base = res
            continue
        for nm in ("logits", "sk", "sv"):
            assert torch.equal(_bits(res[nm]), _bits(base[nm])), f"{res['what']}: {nm} differs from {base['what']}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fp16_every_layout_pair(gpu, shape):
    Bp, n = shape
    _run_pairs(gpu["device"], Bp, n, _pairs(Bp * n))


def test_fp8_weights(gpu):
    from tcavt_amd import capi

    _run_pairs(gpu["device"], 4, 8, [(capi.W_FRAG8, al) for wl, al in _pairs(32) if wl == 0], fp8=True)


def test_refusals(gpu):
    """the entry's own refusals: nothing is launched (logits, the caches and the flags keep their bits)"""
    from tcavt_amd import capi

    dev = gpu["device"]
    lib = capi.lib()

    def refused(msg, edit, null_prefix=False):
        a, px, k = _args(dev, 2, 4, 0, 0)
        edit(a, px)
        before = {nm: k[nm].clone() for nm in ("pk_buf", "pv_buf", "sk_buf", "sv_buf", "logits")}
        rc = lib.tcavt_llama_decode_step_shared(ctypes.byref(a), None if null_prefix else ctypes.byref(px), capi.stream_ptr())
        torch.cuda.synchronize()
        err = lib.tcavt_last_error().decode()
        assert rc == 1 and msg in err, (msg, rc, err)
        for nm, b0 in before.items():
            assert torch.equal(_bits(k[nm]), _bits(b0)), f"{msg}: a refused call wrote {nm}"
        assert bool((k["bufs"]["h16"] == 0).all()) and k["flags"].tolist() == [0, 0, 0]

    def kv8(a, px):
        a.kv8_k_codes = a.kv8_k_scales = a.kv8_v_codes = a.kv8_v_scales = a.k_cache
        a.k_cache = a.v_cache = None

    refused("prefix and the kv8 planes exclude each other", kv8)
    refused("must be a multiple of n = 3", lambda a, px: setattr(px, "n", 3))
    refused("rope_L = 75 must be >= lmax + kv_lmax = 76", lambda a, px: setattr(a, "rope_L", PL + SL - 1))
    refused("prefix: null pointer", lambda a, px: setattr(px, "len", None))
    refused("n = 0", lambda a, px: setattr(px, "n", 0))
    refused("prefix is a null pointer", lambda a, px: None, null_prefix=True)
