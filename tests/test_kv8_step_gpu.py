"""The FP8 KV cache ("KV8") through the decode step, the decoder stack and generate_batch.

Model and inputs: those of test_decode_step_gpu.py (hidden 256, inter 512, 2 layers, 8 / 2 heads, vocab 512, LoRA r 8; kv_lmax 200; pos
ragged over 0, 63, 64, 130, 199, ...; random rows below pos[b], decoys at and behind it), the 16-bit caches pushed through
quant.kv8_quantize into guarded uint8 planes [layers][B][nkv][kv_lmax][64 | 2].

Single step: tcavt_llama_decode_step with the kv8 fields at B in {1, 8, 17, 32, 33}, each on one legal (w_layout, act_layout) pair, plus
FP8 weights at B = 8 and bf16 storage at B = 8.  Reference: oracle.decode.decode_step in float64 on kv8_dequantize of the test's planes
(the oracle takes cache rows "values as stored" and the new k / v from its own arithmetic -- the semantics of the FP8 cache).  Logits
within LOGIT_BAR = 2e-3 of the row norm; arg-max equal wherever the reference's own top-two gap exceeds twice the bar (>= 90 % of the
rows, from the reference alone: test_reference_gaps_cover_the_rows); every layer's planes unchanged except row pos[b]; the last layer's
row pos[b] byte for byte quantize_mx of the qkv buffer's k | v; both flags 0.

Consecutive steps: three steps on the same planes, fixed tokens, pos advanced by the test; one sample starts at pos 62, so rows 62, 63,
64 are appended and then read across the 64-key edge; the oracle is fed the planes as the GPU left them.  Same bars.

Stack and model: the kv8 fields together with k_cache are refused by the step and the stack; decoder_stack with a 16-bit and with an
8-bit cache on the same inputs -- planes == kv8_quantize of the 16-bit cache for rows l < L, rows beyond untouched, the stack's output
bit-equal; generate_batch(kv_cache="fp8"): token 1 equals the fp16-cache run's, eager == hipGraph, two runs equal, decode_weights="fp8"
runs, kv_cache="fp4" raises.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_decode_step_gpu as S

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
LOGIT_BAR, KV_LMAX = S.LOGIT_BAR, S.KV_LMAX
_GB = 256  # guard bytes around every plane
_PER = (64, 2, 64, 2)
_NAMES = ("k_codes", "k_scales", "v_codes", "v_scales")
_cache = {}
_MEASURED = []


def _forms():
    """(kind, B, w_layout, act_layout, fp8 weights)"""
    from tcavt_amd import capi

    return [("fp16", 1, capi.W_FRAG16, 2, False), ("fp16", 8, capi.W_FRAG16, 2, False), ("fp16", 17, capi.W_FRAG16, 1, False),
            ("fp16", 32, 0, 1, False), ("fp16", 33, 0, 0, False), ("fp16", 8, capi.W_FRAG8, 2, True), ("bf16", 8, capi.W_FRAG16, 0, False)]


def _form_id(f):
    return f"{f[0]}-B{f[1]}-w{f[2]}-a{f[3]}" + ("-fp8w" if f[4] else "")


def _planes(B, st):
    """the test's caches as KV8 planes (CPU): [k codes, k scales, v codes, v scales], each uint8 [layers, B, nkv, KV_LMAX, 64 | 2]"""
    from tcavt_amd import quant

    key = ("planes", B, st)
    if key not in _cache:
        tok, pos, kc, vc = S._inputs(B, st)
        q = [quant.kv8_quantize(c[li]) for c in (kc, vc) for li in range(kc.shape[0])]
        nL = kc.shape[0]
        _cache[key] = (tok, pos, [torch.stack([q[i][j] for i in range(s, s + nL)]) for s, j in ((0, 0), (0, 1), (nL, 0), (nL, 1))])
    return _cache[key]


def _dequant(planes):
    """per layer float64 [B, KV_LMAX, nkv, 64] of K and of V"""
    from tcavt_amd import quant

    nL, B, nkv = planes[0].shape[:3]
    view = lambda c, s: [quant.kv8_dequantize(c[li], s[li], torch.float64).view(B, -1, nkv, 64) for li in range(nL)]
    return view(planes[0], planes[1]), view(planes[2], planes[3])


def _prepared(kind, fp8):
    from oracle import decode as D

    pkey = ("wp", kind, fp8)
    if pkey not in _cache:
        cfg = S._cfg()
        _cache[pkey] = D.prepare(S._weights(cfg), cfg, S.CONTRACTS[kind][2], weight_map=S._fp8_map if fp8 else None)
    return _cache[pkey]


def _oracle(kind, fp8, tok, pos, planes):
    from oracle import decode as D

    cfg = S._cfg()
    Wp = _prepared(kind, fp8)
    kd, vd = _dequant(planes)
    with torch.no_grad():
        logits, _ = D.decode_step(Wp, cfg, D.token_embeds(Wp, tok), pos, kd, vd, S.CONTRACTS[kind][2])
    return logits


def _reference(kind, B, fp8):
    key = ("ref", kind, B, fp8)
    if key not in _cache:
        tok, pos, planes = _planes(B, S.CONTRACTS[kind][0])
        _cache[key] = _oracle(kind, fp8, tok, pos, planes)
    return _cache[key]


def test_reference_gaps_cover_the_rows():
    """from the reference alone: at every form the rows with a top-two gap above twice the bar are >= 90 %"""
    for kind, B, _, _, fp8 in _forms():
        qual, _ = S._qualifying(_reference(kind, B, fp8))
        assert float(qual.sum()) >= 0.9 * B, (kind, B, fp8, int(qual.sum()))


# ---------------------------------------------------------------------------------------------------------------------------
# one step on the test's own buffers

class _Step:
    """buffers of a decode step with guarded KV8 planes; run(tok, pos) launches one tcavt_llama_decode_step and asserts everything that
    needs no reference"""

    def __init__(self, kind, dev, B, wl, al, fp8, planes):
        from tcavt_amd import capi

        self.capi, self.kind, self.dev, self.B = capi, kind, dev, B
        m = S._model(kind, dev)
        ll = S._cfg().llama
        LW = m.mllm.llama_wrapper
        PL, P = LW._prepared(), m.mllm._prepared()
        st = LW.storage
        self.st, self.ll = st, ll
        H, I, nq, nkv, V, nL = ll.hidden, ll.inter, ll.n_q_heads, ll.n_kv_heads, ll.vocab, ll.layers
        self.what = f"kv8 {kind}{' fp8 weights' if fp8 else ''} B={B} w_layout={wl} act_layout={al}"
        self.bufs = []
        for p in planes:
            buf = torch.full((p.numel() + 2 * _GB,), 0xA5, dtype=torch.uint8, device=dev)
            buf[_GB:-_GB] = p.reshape(-1).to(dev)
            self.bufs.append(buf)
        Br = B if al == 0 else 8 if al == 2 else 16 if B <= 16 else 32
        z = lambda *shape, dt=st: torch.zeros(*shape, dtype=dt, device=dev)
        self.w = dict(h16=z(Br, H), part=z(B, H // 16, dt=F32), qkv=z(B, (nq + 2 * nkv) * 64), att=z(Br, nq * 64), act=z(Br, I), t=z(B, 64),
                      x16=z(Br, H))
        if not LW.stream16:
            self.w["h"] = z(B, H, dt=F32)
        self.logits = torch.full((B + 2, V), float("nan"), dtype=F32, device=dev)
        self.flags = torch.zeros(3, dtype=torch.int32, device=dev)
        self.tok = torch.zeros(B, dtype=torch.int64, device=dev)
        self.pos = torch.zeros(B, dtype=torch.int32, device=dev)
        self.cos, self.sin = LW._rope_tables(KV_LMAX, dev)
        a = self.a = capi.DecodeArgs()
        for k_, v_ in self.w.items():
            setattr(a, k_, v_.data_ptr())
        a.layers, a.gamma_final = PL.carr, PL.g_final.data_ptr()
        self.keep = None
        if wl != 0:
            self.keep = LW.decode_weights("fp8" if fp8 else "fp16")
            a.layers, a.table_packed, a.w_layout = self.keep.carr, self.keep.table.data_ptr(), wl
        a.act_layout = al
        a.rope_cos, a.rope_sin, a.rope_L = self.cos.data_ptr(), self.sin.data_ptr(), KV_LMAX
        a.table, a.txt_mod = PL.table.data_ptr(), P.txt.data_ptr()
        a.cur_tok, a.pos = self.tok.data_ptr(), self.pos.data_ptr()
        a.kv8_k_codes, a.kv8_k_scales, a.kv8_v_codes, a.kv8_v_scales = (b[_GB:].data_ptr() for b in self.bufs)
        a.kv_lmax = KV_LMAX
        a.logits, a.bad_id_flag, a.nonfinite_flag = self.logits[1:].data_ptr(), self.flags.data_ptr(), self.flags[2:3].data_ptr()
        self.lp = torch.zeros(B * H, dtype=F32, device=dev)
        a.lora_part, a.lora_rank = self.lp.data_ptr(), LW.lora_r
        a.n_layers, a.B, a.H, a.I, a.nq, a.nkv, a.V = nL, B, H, I, nq, nkv, V
        a.dtype16 = capi.F16 if st == F16 else capi.BF16
        a.rms_eps, a.lora_scale = ll.rms_eps, LW.lora_alpha / LW.lora_r
        a.stream_scale = float(LW.stream_scale)

    def planes(self):
        """the four planes as the GPU holds them (CPU copies, [layers, B, nkv, KV_LMAX, per])"""
        ll = self.ll
        return [b[_GB:-_GB].view(ll.layers, self.B, ll.n_kv_heads, KV_LMAX, per).cpu().clone() for b, per in zip(self.bufs, _PER)]

    def run(self, tok, pos):
        from tcavt_amd import quant

        capi, B, ll, dev, what = self.capi, self.B, self.ll, self.dev, self.what
        nq, nkv, nL = ll.n_q_heads, ll.n_kv_heads, ll.layers
        w = nkv * 64
        self.tok.copy_(tok)
        self.pos.copy_(pos.to(torch.int32))
        before = [b.clone() for b in self.bufs]
        self.logits.fill_(float("nan"))
        rc = capi.lib().tcavt_llama_decode_step(ctypes.byref(self.a), capi.stream_ptr())
        torch.cuda.synchronize()
        capi.check(rc, what)
        assert self.flags.tolist() == [0, 0, 0], f"{what}: bad_id / nonfinite flags {self.flags.tolist()}"
        assert torch.equal(self.tok.cpu(), tok) and torch.equal(self.pos.cpu().long(), pos.long()), f"{what}: cur_tok / pos modified"
        assert bool(torch.isnan(self.logits[0]).all()) and bool(torch.isnan(self.logits[B + 1]).all()), f"{what}: write outside logits"
        got = self.logits[1:B + 1]
        assert torch.isfinite(got).all(), f"{what}: non-finite logits"
        at = torch.zeros(B, KV_LMAX, dtype=torch.bool, device=dev)
        at[torch.arange(B, device=dev), self.pos.long()] = True
        at = at[None, :, None, :].expand(nL, B, nkv, KV_LMAX)
        qkv = self.w["qkv"].cpu()
        newq = quant.kv8_quantize(qkv[:, None, nq * 64:nq * 64 + w]) + quant.kv8_quantize(qkv[:, None, nq * 64 + w:])  # [B, nkv, 1, per]
        for buf, old, nw, nm, per in zip(self.bufs, before, newq, _NAMES, _PER):
            assert torch.equal(buf[:_GB], old[:_GB]) and torch.equal(buf[-_GB:], old[-_GB:]), f"{what}: write into the guards of {nm}"
            now, was = buf[_GB:-_GB].view(nL, B, nkv, KV_LMAX, per), old[_GB:-_GB].view(nL, B, nkv, KV_LMAX, per)
            same = (now == was).all(-1)
            assert bool(same[~at].all()), f"{what}: a {nm} row other than pos[b] was written"
            last = now[nL - 1][at[0]].view(B, nkv, per).cpu()
            assert torch.equal(last, nw.view(B, nkv, per)), f"{what}: the last layer's {nm} row pos[b] is not quantize_mx of the qkv buffer's k | v"
        return got.clone()


def _check_logits(got, ref, what):
    got = got.cpu().double()
    e = (got - ref).norm(dim=-1) / ref.norm(dim=-1)
    qual, amax = S._qualifying(ref)
    print(f"[kv8 step] {what}: logits rel worst {e.max().item():.2e} (bar {LOGIT_BAR:.0e}); {int(qual.sum())} of {ref.shape[0]} rows qualify")
    _MEASURED.append((what, e.max().item()))
    assert bool((e < LOGIT_BAR).all()), f"{what}: logits rel {e.tolist()}"
    assert float(qual.sum()) >= 0.9 * ref.shape[0]
    assert torch.equal(got.argmax(-1)[qual], amax[qual]), f"{what}: arg-max differs on a qualifying row"


@pytest.mark.parametrize("form", range(7), ids=lambda i: _form_id(_forms()[i]))
def test_single_step(gpu, form):
    kind, B, wl, al, fp8 = _forms()[form]
    tok, pos, planes = _planes(B, S.CONTRACTS[kind][0])
    st = _Step(kind, gpu["device"], B, wl, al, fp8, planes)
    got = st.run(tok, pos)
    _check_logits(got, _reference(kind, B, fp8), st.what)


STEP_POS = [62, 0, 130, 196, 63, 1, 100, 17, 127, 191]
STEP_SEED = 77


def _step_inputs():
    """planes for STEP_POS (random rows below pos[b]; decoys at and behind it, which the steps overwrite before they read them) and the
    three steps' tokens"""
    from tcavt_amd import quant

    ll = S._cfg().llama
    B, w = len(STEP_POS), ll.n_kv_heads * ll.head_dim
    g = torch.Generator().manual_seed(STEP_SEED)
    pos = torch.tensor(STEP_POS)
    kc = torch.randn(ll.layers, B, KV_LMAX, w, generator=g)
    vc = torch.randn(ll.layers, B, KV_LMAX, w, generator=g)
    j = torch.arange(KV_LMAX)
    behind = (j[None, :] >= pos[:, None])[None, :, :, None]
    src = j[None, :] % pos.clamp_min(1)[:, None]
    kc = torch.where(behind, 4 * torch.gather(kc, 2, src[None, :, :, None].expand_as(kc)), kc).to(F16)
    vc = torch.where(behind, 30000.0 * (torch.randint(0, 2, vc.shape, generator=g) * 2 - 1).float(), vc).to(F16)
    q = [[quant.kv8_quantize(c[li]) for li in range(ll.layers)] for c in (kc, vc)]
    planes = [torch.stack([q[i][li][jj] for li in range(ll.layers)]) for i, jj in ((0, 0), (0, 1), (1, 0), (1, 1))]
    toks = [torch.randint(0, ll.vocab, (B,), generator=g) for _ in range(3)]
    return pos, planes, toks


def test_consecutive_steps(gpu):
    """append-then-read across launches: rows 62, 63, 64 of sample 0 are written by steps 1 .. 3 and read by the steps after them"""
    from tcavt_amd import capi

    kind, B = "fp16", len(STEP_POS)
    pos, planes, toks = _step_inputs()
    st = _Step(kind, gpu["device"], B, capi.W_FRAG16, 1, False, planes)
    for step in range(3):
        tok = toks[step]
        ref = _oracle(kind, False, tok, pos, st.planes())  # the cache as the GPU left it
        got = st.run(tok, pos)
        _check_logits(got, ref, f"{st.what} step {step} pos {pos.tolist()}")
        pos = pos + 1
    assert pos.tolist()[0] == 65


# ---------------------------------------------------------------------------------------------------------------------------
# refusals, the stack, the model

def test_both_cache_types_are_refused(gpu):
    from tcavt_amd import capi

    dev = gpu["device"]
    tok, pos, planes = _planes(8, F16)
    st = _Step("fp16", dev, 8, capi.W_FRAG16, 2, False, planes)
    dummy = torch.zeros(64, dtype=F16, device=dev)
    st.a.k_cache = st.a.v_cache = dummy.data_ptr()
    before = [b.clone() for b in st.bufs]
    rc = capi.lib().tcavt_llama_decode_step(ctypes.byref(st.a), capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 1 and "exclude each other" in _last_error()
    assert all(torch.equal(b, o) for b, o in zip(st.bufs, before)) and bool(torch.isnan(st.logits).all())


def _last_error():
    from tcavt_amd import capi

    msg = capi.lib().tcavt_last_error()
    return msg.decode() if msg else ""


def _batch(cfg, lens, Lt, seed):
    from tcavt_amd import synth

    b = synth.make_batch(cfg, len(lens), text_len=Lt, seed=seed, ragged=False)
    for i, n in enumerate(lens):
        b["input_ids"][i, n:] = 0
        b["attention_mask"][i, n:] = 0
    return {k: torch.from_numpy(np.asarray(b[k])) for k in ("vision_emb", "input_ids", "attention_mask")}


def _prefill(m, g, cache, Lmax):
    """generate_batch's prefill on the model's own workspaces: embeddings, kv_len, decoder_stack with the given cache -> final16"""
    from tcavt_amd import ops

    mm = m.mllm
    LW, ws, P = mm.llama_wrapper, mm._ws, mm._prepared()
    PL = LW._prepared()
    dev = g["vision_emb"].device
    B, Lt = g["input_ids"].shape
    Nq, H = mm.qformer.num_query_tokens, mm.llama_hidden_size
    L = Nq + Lt
    with torch.no_grad():
        img = mm._image_tokens(g["vision_emb"])
        flags = torch.zeros(3, dtype=torch.int32, device=dev)
        h16, part = LW.norm_inputs(B * L, dev)
        ops.embed_fuse(PL.table, g["input_ids"], img, P.vis, P.txt, None, flags[0:1], h16=h16, part=part, npart=LW.norm_npart(B * L),
                       stream_scale=LW.stream_scale)
        kv_len = torch.zeros(B, dtype=torch.int32, device=dev)
        ops.mask_to_kvlen(g["attention_mask"].to(torch.int64).contiguous(), Nq, kv_len, flags[1:2])
        final16 = torch.zeros(B * L, H, dtype=LW.storage, device=dev)
        LW.decoder_stack(None, kv_len, B, L, out_bf16=final16, kv_cache=cache + (Lmax,), nonfinite_flag=flags[2:3])
        torch.cuda.synchronize()
    assert flags.tolist() == [0, 0, 0]
    return final16, L


def test_stack_stores_quantised(gpu):
    """decoder_stack with a 16-bit and with an 8-bit cache: planes == kv8_quantize of the 16-bit cache for l < L, rows beyond L untouched,
    the stack's output bit-equal; both cache types together are refused"""
    from tcavt_amd import capi, quant

    dev = gpu["device"]
    m = S._model("fp16", dev)
    cfg = S._cfg()
    ll = cfg.llama
    g = {k: v.to(dev) for k, v in _batch(cfg, [20, 9], 20, 3).items()}
    B, nL, nkv = 2, ll.layers, ll.n_kv_heads
    Lmax = 16 + 20 + 4
    kc = torch.full((nL, B, Lmax, nkv * 64), float("nan"), dtype=F16, device=dev)
    vc = kc.clone()
    out16, L = _prefill(m, g, (kc, vc), Lmax)
    assert L == 36
    bufs = [torch.full((nL * B * nkv * Lmax * per + 2 * _GB,), 0xA5, dtype=torch.uint8, device=dev) for per in _PER]
    planes = tuple(b[_GB:-_GB] for b in bufs)
    out8, _ = _prefill(m, g, planes, Lmax)
    assert torch.equal(S._bits(out16), S._bits(out8)), "the stack's output depends on the cache type"
    assert bool(torch.isnan(kc[:, :, L:]).all()) and bool(torch.isfinite(kc[:, :, :L]).all())
    for c16, (ci, si), nm in ((kc, (0, 1), "k"), (vc, (2, 3), "v")):
        for li in range(nL):
            wc, wsb = quant.kv8_quantize(c16[li, :, :L].cpu())
            gc = planes[ci].view(nL, B, nkv, Lmax, 64)[li].cpu()
            gs = planes[si].view(nL, B, nkv, Lmax, 2)[li].cpu()
            assert torch.equal(gc[:, :, :L], wc) and torch.equal(gs[:, :, :L], wsb), f"layer {li} {nm}: planes are not kv8_quantize of the 16-bit cache"
            assert bool((gc[:, :, L:] == 0xA5).all()) and bool((gs[:, :, L:] == 0xA5).all()), f"layer {li} {nm}: rows beyond L written"
    for b in bufs:
        assert bool((b[:_GB] == 0xA5).all()) and bool((b[-_GB:] == 0xA5).all())
    # both cache types in one call: refused before anything is launched
    a = capi.LlamaStackArgs()
    lay = (capi.LlamaLayer * 1)()
    for n in ("w_qkv", "w_o", "w_gu", "w_d"):
        setattr(lay[0], n, 256)
    a.layers = lay
    for n in ("gamma_final", "rope_cos", "rope_sin", "h16", "part", "kv_len", "qkv", "att", "act", "out16"):
        setattr(a, n, 256)
    a.k_cache, a.v_cache = kc.data_ptr(), vc.data_ptr()
    a.kv8_k_codes, a.kv8_k_scales, a.kv8_v_codes, a.kv8_v_scales = (p.data_ptr() for p in planes)
    a.n_layers, a.B, a.L, a.H, a.I, a.nq, a.nkv, a.dtype16, a.kv_lmax = 1, 2, 36, 256, 512, 8, 2, capi.F16, Lmax
    a.npart_in = capi.lib().tcavt_norm_npart(72, 256, 512)
    assert capi.lib().tcavt_llama_stack_forward(ctypes.byref(a), capi.stream_ptr()) == 1 and "exclude each other" in _last_error()


def test_generate_batch_fp8_cache(gpu):
    dev = gpu["device"]
    m = S._model("fp16", dev)
    cfg = S._cfg()
    g = {k: v.to(dev) for k, v in _batch(cfg, [20, 9, 14, 1], 20, 5).items()}
    kw = dict(max_new_tokens=8, input_ids=g["input_ids"], attention_mask=g["attention_mask"], do_sample=False)

    def gen(**extra):
        out = m.mllm.generate_batch(g["vision_emb"], None, **kw, **extra).cpu().clone()
        m.mllm.check_flags()
        return out

    ref16 = gen()
    eager = gen(kv_cache="fp8", use_graph=False)
    graph = gen(kv_cache="fp8", use_graph=True)
    again = gen(kv_cache="fp8", use_graph=True)
    assert tuple(eager.shape) == (4, 8)
    assert torch.equal(eager[:, 0], ref16[:, 0]), "token 1 comes from the prefill's logits: it cannot depend on the cache type"
    assert torch.equal(eager, graph), "eager and hipGraph replay differ"
    assert torch.equal(graph, again), "two runs differ"
    print(f"[kv8 generate] greedy tokens that differ from the fp16-cache run: {int((eager != ref16).sum())} of {eager.numel()}")
    w8 = gen(kv_cache="fp8", decode_weights="fp8")
    assert tuple(w8.shape) == (4, 8) and torch.equal(w8[:, 0], ref16[:, 0])
    assert torch.equal(gen(), ref16), "the fp16-cache path changed after an fp8-cache run"
    with pytest.raises(ValueError, match="'fp16' or 'fp8'"):
        gen(kv_cache="fp4")


def test_report_measured(gpu):
    """(runs last in file order) the measured logit errors of this session, per form"""
    for what, e in _MEASURED:
        print(f"kv8 decode_step  {what:72s} worst logits rel {e:.2e}")
