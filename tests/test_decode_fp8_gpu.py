"""The opt-in FP8 (e4m3) weight stream of the decode step: tcavt_pack_weight8, tcavt_gemm_args.w_layout = W_FRAG8, and
generate_batch(decode_weights="fp8").

Row scales are powers of two, so the FP8 path has nothing to be approximately equal to: code * 2^k is a 16-bit number, the
accumulator times 2^k is exact, and an output column sees one weight row only.  Every check below is therefore an equality
with the existing fragment-major 16-bit path run on the dequantised matrix -- except one reported quality figure on weights
that were NOT rounded to the format first."""
import ctypes
import functools
import os

import pytest
import torch

from tests.util import load_generation_case, rel_err

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


# ---------------------------------------------------------------------------------------------------------------------
# the pack kernel against its definition (quant.py)
# ---------------------------------------------------------------------------------------------------------------------
def _next_up(x):
    return (x.view(torch.int16) + 1).view(x.dtype)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [256, 1280])
def test_pack_kernel_matches_the_definition(gpu, K, dt):
    """Codes and scale bytes of tcavt_pack_weight8 equal quant.pack: rows whose maximum sits exactly on and just above a
    scale boundary, an all-zero row, values in e4m3's subnormal range, exact ties between two codes (to even), rows of very
    different magnitude inside one 16-row block, a row with an inf.  The rounding is integer arithmetic in the kernel and in
    torch alike, so the comparison is exact, the sign of zero included."""
    from tcavt_amd import ops, quant

    dev = gpu["device"]
    N = 48
    g = torch.Generator().manual_seed(1000 + K)
    w = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-9, 4, (N, 1), generator=g).float())).to(dt)
    w[0] = w[0].float().clamp(-40, 40).to(dt)
    w[0, K - 1] = 56.0                                   # 448 * 2^-3: on the boundary, k = -3
    w[1] = w[0]
    w[1, K - 1] = _next_up(torch.tensor(56.0).to(dt))    # just above: k = -2
    w[2] = 0                                             # all zero: k = 0
    w[3] = w[3].float().clamp(-100, 100).to(dt)
    w[3, 0] = -256.0                                     # k = 0: the values below are encoded as they are
    planted = torch.tensor([17.0, 19.0, 21.0, 23.0, 25.0, 27.0, -17.0, 34.0, 38.0, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10,
                            2.0 ** -9, -(2.0 ** -9), 7 * 2.0 ** -9, 15 * 2.0 ** -10, 2.0 ** -6, 2.0 ** -11, -(2.0 ** -11), -0.0])
    w[3, 1:1 + len(planted)] = planted.to(dt)
    w[4] = (w[3].float() * 2.0 ** -5).to(dt)             # the same ties and subnormals under k = -5 (17 * 2^-5 between two codes)
    w[20] = (torch.randn(K, generator=g) * (3000.0 if dt == torch.float16 else 3.0e30)).to(dt)  # k > 0
    w[21] = (torch.randn(K, generator=g) * 2.0 ** -12).to(dt)
    w[40, 7] = float("inf")
    want = quant.pack(w)
    got = ops.pack_weight8(w.to(dev))
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and got.numel() == N * K + 4 * N
    got = got.cpu()
    codes_g, k_g = quant.unpack(got, N, K)
    codes_w, k_w = quant.unpack(want, N, K)
    assert torch.equal(got[N * K:], want[N * K:]), (k_g.tolist(), k_w.tolist())
    assert k_w[:5].tolist() == [-3, -2, 0, 0, -5] and k_w[20].item() > 0 and k_w[40].item() == 0
    bad = (codes_g != codes_w).nonzero()
    assert bad.numel() == 0, [(r, c, w[r, c].item(), codes_g[r, c].item(), codes_w[r, c].item()) for r, c in bad[:8].tolist()]
    assert torch.equal(got, want)
    f8 = codes_g[3, 1:5].view(torch.float8_e4m3fn).float().tolist()
    assert f8 == [16.0, 20.0, 20.0, 24.0] and codes_g[40].eq(0x7F).all() and codes_g[2].eq(0).all()
    # a view with a row stride (ldw > K) packs the same
    wide = torch.zeros(N, K + 64, dtype=dt, device=dev)
    wide[:, :K] = w.to(dev)
    assert torch.equal(ops.pack_weight8(wide[:, :K]).cpu(), want)


# ---------------------------------------------------------------------------------------------------------------------
# the skinny GEMM on FP8 weights against the 16-bit fragment-major path on the dequantised matrix
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(dt, N, K, seed):
    """A weight matrix for the kernel test, made once per (type, shape): rows of one 16-row block get different scales --
    the row maximum is planted between 8 and 448, so k runs over [-5, 0] -- and every non-zero dequantised weight is a normal
    fp16 number (checked): the equality must not rest on how an MFMA treats subnormal operands.  Returns (dequantised matrix,
    its pack_weight16 copy, the pack_weight8 copy of the ORIGINAL matrix), all on the device."""
    from tcavt_amd import ops, quant

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    peaks = torch.tensor([8.0, 448.0, 20.0, 100.0, 12.0, 300.0, 56.0, 57.0, 224.0, 31.0, 9.0, 440.0, 64.0, 130.0, 17.0, 250.0])
    peak = peaks[(torch.arange(N) * 7 + torch.arange(N) // 16) % 16]
    w = torch.randn(N, K, generator=g) * (peak / 4)[:, None]
    w = torch.maximum(torch.minimum(w, 0.9 * peak[:, None]), -0.9 * peak[:, None])
    w[torch.arange(N), torch.randint(0, K, (N,), generator=g)] = peak * (1 - 2 * (torch.arange(N) % 2).float())
    w = w.to(dt)
    codes, k = quant.quantize(w)
    assert k.min().item() == -5 and k.max().item() == 0 and all(len(set(k[b:b + 16].tolist())) >= 4 for b in range(0, N, 16))
    wq = quant.dequantize(codes, k, dt)
    nz = wq.float().abs()[wq != 0]
    assert nz.min().item() >= 2.0 ** -14 and torch.isfinite(wq.float()).all()
    assert torch.equal(quant.dequantize(*quant.quantize(wq), dt).view(torch.int16), wq.view(torch.int16))
    wq_d = wq.to(dev)
    return wq_d, ops.pack_weight16(wq_d), ops.pack_weight8(w.to(dev))


def _gemm(M, K, dt, x, w, wl, N, epi, out, xin=None, **kw):
    from tcavt_amd import capi, ops

    a = capi.GemmArgs()
    a.A, a.lda, a.W, a.ldw = (x if xin is None else xin).data_ptr(), K, w.data_ptr(), K
    a.C, a.ldc = (out.data_ptr() if out is not None else None), kw.pop("ldc", N)
    a.M, a.N, a.K, a.tile, a.epilogue, a.w_layout = M, N, K, 0, epi, wl
    a.in_dtype, a.out_dtype = ops._DT[dt], ops._DT[out.dtype] if out is not None else capi.F32
    for k_, v_ in kw.items():
        setattr(a, k_, v_.data_ptr() if torch.is_tensor(v_) else v_)
    capi.check(capi.lib().tcavt_gemm_bf16(ctypes.byref(a), capi.stream_ptr()), "gemm")
    return out


def _finite(*ts):
    return all(torch.isfinite(t.float()).all().item() for t in ts)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [1280, 256])
@pytest.mark.parametrize("M", [1, 8, 17, 32])
def test_skinny_gemm_fp8_weights_bit_equal(gpu, M, K, dt):
    """Every epilogue form of the decode step: W_FRAG8 on pack_weight8(w) == W_FRAG16 on pack_weight16(dequantize(w)), bit
    for bit.  K = 1280: five k-steps per wave (a partial batch of the load loop); K = 256: one."""
    from tcavt_amd import capi, ops

    dev = gpu["device"]
    g = torch.Generator().manual_seed(7000 + M + K)
    H = 512
    x = (torch.randn(M, K, generator=g) * 2.0 ** -8).to(dt).to(dev)
    part = (torch.rand(M, 8, generator=g) * 40 + 10).to(dev)
    W16, W8 = capi.W_FRAG16, capi.W_FRAG8
    run = functools.partial(_gemm, M, K, dt, x)
    rs = dict(rowscale_part=part, rowscale_npart=8, rowscale_h=K, rowscale_eps=1e-5)

    # q|k|v: RoPE + LoRA second source + row scale (the LoRA term is 16-bit and is not scaled)
    N = 384
    wq, p16, p8 = _weights(dt, N, K, 1)
    t2 = (torch.randn(M, 64, generator=g) * 0.25).to(dt).to(dev)
    w2 = (torch.randn(N, 64, generator=g) * 0.5).to(dt).to(dev)
    cos, sin = torch.rand(50, 32, generator=g).to(dev), torch.rand(50, 32, generator=g).to(dev)
    pos = torch.randint(0, 50, (M,), generator=g).to(torch.int32).to(dev)
    kw = dict(A2=t2, lda2=64, W2=w2, ldw2=64, K2=64, rope_cos=cos, rope_sin=sin, rope_L=50, rope_cols=320, rope_pos=pos, **rs)
    a_ = run(p16, W16, N, capi.EPI_ROPE | capi.EPI_ROWSCALE, torch.empty(M, N, dtype=dt, device=dev), **kw)
    b_ = run(p8, W8, N, capi.EPI_ROPE | capi.EPI_ROWSCALE, torch.empty(M, N, dtype=dt, device=dev), **kw)
    assert _finite(a_) and torch.equal(a_, b_) and a_.float().abs().max() > 0
    nolora = {k_: v_ for k_, v_ in kw.items() if k_ not in ("A2", "lda2", "W2", "ldw2", "K2")}
    c_ = run(p8, W8, N, capi.EPI_ROPE | capi.EPI_ROWSCALE, torch.empty(M, N, dtype=dt, device=dev), **nolora)
    assert not torch.equal(b_, c_)  # (the second source did take part)

    # gate|up: SiLU * up with row scale
    N = 512
    wq, p16, p8 = _weights(dt, N, K, 2)
    a_ = run(p16, W16, N, capi.EPI_SILU_MUL | capi.EPI_ROWSCALE, torch.empty(M, N // 2, dtype=dt, device=dev), ldc=N // 2, **rs)
    b_ = run(p8, W8, N, capi.EPI_SILU_MUL | capi.EPI_ROWSCALE, torch.empty(M, N // 2, dtype=dt, device=dev), ldc=N // 2, **rs)
    assert _finite(a_) and torch.equal(a_, b_) and a_.float().abs().max() > 0

    # o / down: residual + NORM_OUT -- in place on the 16-bit stream (fp16), fp32 stream + 16-bit copy (bf16)
    N = H
    wq, p16, p8 = _weights(dt, N, K, 3)
    res = torch.randn(M, N, generator=g).to(dev)
    outs = []
    for wt, wl in ((p16, W16), (p8, W8)):
        npart = ops.norm_npart(M, N, K)
        h16 = res.to(dt)
        pt = torch.zeros(M, npart, device=dev)
        if dt == torch.float16:
            run(wt, wl, N, capi.EPI_RESIDUAL | capi.EPI_NORM_OUT, None, norm_h16=h16, norm_part=pt)
            outs.append((h16, pt))
        else:
            c = run(wt, wl, N, capi.EPI_RESIDUAL | capi.EPI_NORM_OUT, torch.empty(M, N, device=dev), residual=res, ldr=N, norm_h16=h16,
                    norm_part=pt)
            outs.append((c, h16, pt))
    for u_, v_ in zip(*outs):
        assert _finite(u_) and torch.equal(u_, v_)
    assert not torch.equal(outs[0][0].float(), res.to(dt).float())

    # lm_head: plain fp32 output, both column-block forms (N < 8192; N >= 8192 with M > 16: two blocks per workgroup) -- and
    # against float64 on the dequantised matrix
    for N in (1008, 8192):
        wq, p16, p8 = _weights(dt, N, K, 4)
        a_ = run(p16, W16, N, 0, torch.empty(M, N, device=dev))
        b_ = run(p8, W8, N, 0, torch.empty(M, N, device=dev))
        assert _finite(a_) and torch.equal(a_, b_)
        assert rel_err(b_.cpu(), x.cpu().double() @ wq.cpu().double().T) < 1e-5

    # ---- fragment-major activations: blocks of 16 tokens, and one block of 8 for M <= 8
    Mr = 16 if M <= 16 else 32
    AF, AO = capi.ACT_A_FRAG16, capi.ACT_A_FRAG16 | capi.ACT_OUT_FRAG16

    def to_frag(t):
        pad = torch.zeros(Mr, t.shape[1], dtype=t.dtype, device=dev)
        pad[:M] = t
        return ops.pack_weight16(pad)

    def to_frag8(t):
        pad = torch.zeros(8, t.shape[1], dtype=t.dtype, device=dev)
        pad[:M] = t
        return pad.view(8, t.shape[1] // 32, 4, 8).permute(1, 2, 0, 3).contiguous().view(-1)

    forms = [(to_frag, AF, AO, Mr)] + ([(to_frag8, AF | capi.ACT_BLOCK8, AO | capi.ACT_BLOCK8, 8)] if M <= 8 else [])
    for frag, af, ao, mr in forms:
        xf = frag(x)
        wq, p16, p8 = _weights(dt, 512, K, 2)
        a_ = run(p16, W16, 512, capi.EPI_SILU_MUL | capi.EPI_ROWSCALE, torch.zeros(mr * 256, dtype=dt, device=dev), xin=xf, ldc=256, act_layout=ao, **rs)
        b_ = run(p8, W8, 512, capi.EPI_SILU_MUL | capi.EPI_ROWSCALE, torch.zeros(mr * 256, dtype=dt, device=dev), xin=xf, ldc=256, act_layout=ao, **rs)
        assert _finite(a_) and torch.equal(a_, b_) and a_.float().abs().max() > 0
        wq, p16, p8 = _weights(dt, 384, K, 1)
        a_ = run(p16, W16, 384, capi.EPI_ROPE | capi.EPI_ROWSCALE, torch.empty(M, 384, dtype=dt, device=dev), xin=xf, act_layout=af, **kw)
        b_ = run(p8, W8, 384, capi.EPI_ROPE | capi.EPI_ROWSCALE, torch.empty(M, 384, dtype=dt, device=dev), xin=xf, act_layout=af, **kw)
        assert _finite(a_) and torch.equal(a_, b_)
        wq, p16, p8 = _weights(dt, 1008, K, 4)
        a_ = run(p16, W16, 1008, 0, torch.empty(M, 1008, device=dev), xin=xf, act_layout=af)
        b_ = run(p8, W8, 1008, 0, torch.empty(M, 1008, device=dev), xin=xf, act_layout=af)
        assert _finite(a_) and torch.equal(a_, b_)
        wq, p16, p8 = _weights(dt, H, K, 3)
        res16 = torch.randn(M, H, generator=g).to(dev).to(dt)
        npart = ops.norm_npart(M, H, K)
        pair = []
        for wt, wl in ((p16, W16), (p8, W8)):
            h_, p_ = frag(res16), torch.zeros(M, npart, device=dev)
            run(wt, wl, H, capi.EPI_RESIDUAL | capi.EPI_NORM_OUT, None, xin=xf, norm_h16=h_, norm_part=p_, act_layout=ao)
            pair.append((h_, p_))
        assert _finite(*pair[0]) and torch.equal(pair[0][0], pair[1][0]) and torch.equal(pair[0][1], pair[1][1])
        assert not torch.equal(pair[0][0], frag(res16))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", [1, 17])
def test_skinny_gemm_fp8_weights_split_k_workspace_form(gpu, M, dt):
    """With a split-K workspace (tcavt_gemm_args.splitk_ws; TCAVT_DECODE_SPLITK=1 in the model) the FP8 form splits K over
    workgroups like the 16-bit form: the scaled partial sums go through the slabs, so the equality with the 16-bit split
    holds as it stands.  K = 2048: eight slices of one k-step per wave."""
    from tcavt_amd import capi, ops

    dev = gpu["device"]
    K, N = 2048, 512
    g = torch.Generator().manual_seed(7100 + M)
    x = (torch.randn(M, K, generator=g) * 2.0 ** -8).to(dt).to(dev)
    ws = torch.zeros(9 << 20, dtype=torch.uint8, device=dev)
    ws[16 << 10:] = 0x7F
    sk = dict(splitk_ws=ws, splitk_ws_bytes=ws.numel())
    wq, p16, p8 = _weights(dt, N, K, 5)
    res = torch.randn(M, N, generator=g).to(dev)
    outs = []
    for wt, wl, kw in ((p16, capi.W_FRAG16, sk), (p8, capi.W_FRAG8, sk), (p8, capi.W_FRAG8, {})):
        h16, pt = res.to(dt), torch.zeros(M, ops.norm_npart(M, N, K), device=dev)
        c = _gemm(M, K, dt, x, wt, wl, N, capi.EPI_RESIDUAL | capi.EPI_NORM_OUT, torch.empty(M, N, device=dev), residual=res, ldr=N,
                  norm_h16=h16, norm_part=pt, **kw)
        outs.append((c, h16, pt))
    torch.cuda.synchronize()
    for u_, v_ in zip(outs[0], outs[1]):
        assert _finite(u_) and torch.equal(u_, v_)
    assert int(ws[:16 << 10].view(torch.int32).abs().sum().item()) == 0      # tickets re-armed
    assert not torch.equal(outs[1][0], outs[2][0])                           # (the split did run: another summation order)
    assert rel_err(outs[1][0].cpu(), outs[2][0].cpu()) < 1e-5
    a_ = _gemm(M, K, dt, x, p16, capi.W_FRAG16, N, 0, torch.empty(M, N, device=dev), **sk)
    b_ = _gemm(M, K, dt, x, p8, capi.W_FRAG8, N, 0, torch.empty(M, N, device=dev), **sk)
    assert torch.equal(a_, b_) and rel_err(b_.cpu(), x.cpu().double() @ wq.cpu().double().T) < 1e-5


def test_fp8_weights_are_refused_outside_the_skinny_form(gpu):
    from tcavt_amd import capi, ops

    dev = gpu["device"]
    dt, K, N = torch.float16, 256, 512
    wq, p16, p8 = _weights(dt, N, K, 2)
    o = torch.empty(64, N, device=dev)
    for M, tile, k_ in ((64, 0, K), (8, 128, K)):
        xl = torch.zeros(M, K, dtype=dt, device=dev)
        a = capi.GemmArgs()
        a.A, a.lda, a.W, a.ldw, a.C, a.ldc, a.M, a.N, a.K, a.tile = xl.data_ptr(), K, p8.data_ptr(), K, o.data_ptr(), N, M, N, k_, tile
        a.in_dtype, a.out_dtype, a.w_layout = ops._DT[dt], capi.F32, capi.W_FRAG8
        assert capi.lib().tcavt_gemm_bf16(ctypes.byref(a), capi.stream_ptr()) != 0
        assert b"skinny form" in capi.lib().tcavt_last_error()
    a.M, a.tile, a.w_layout = 8, 0, 3  # no such layout
    assert capi.lib().tcavt_gemm_bf16(ctypes.byref(a), capi.stream_ptr()) != 0
    assert int(capi.lib().tcavt_pack_weight8_bytes(N, K)) == N * K + 4 * N
    assert capi.lib().tcavt_pack_weight8(wq.data_ptr(), K, capi.F16, p8.data_ptr(), N + 8, K, capi.stream_ptr()) != 0  # N % 16


# ---------------------------------------------------------------------------------------------------------------------
# the model: generate_batch(decode_weights="fp8")
# ---------------------------------------------------------------------------------------------------------------------
def _snap_prepared(LW):
    """Round the prepared matrices of the decoder (w_qkv, w_o, w_gu, w_d of every layer, and the tied table) to the FP8 format
    and back, IN PLACE, through the pack kernel (held to quant.py above) and quant.dequantize; fp16: anything below 2^-14
    becomes zero.  On such a model the two decode paths stream the same numbers.  The decode-weight caches are dropped."""
    from tcavt_amd import ops, quant

    P = LW._prepared()
    with torch.no_grad():
        for t in [w for d in P.layers for w in (d.w_qkv, d.w_o, d.w_gu, d.w_d)] + [P.table]:
            N, K = t.shape
            wq = quant.dequantize(*quant.unpack(ops.pack_weight8(t), N, K), t.dtype)
            if t.dtype == torch.float16:
                wq = torch.where(wq.abs() < 2.0 ** -14, torch.zeros_like(wq), wq)
            assert torch.isfinite(wq.float()).all()
            t.copy_(wq)
    LW._prep_dec = None
    LW._prep_dec8 = None


def _both(m, LW, g, N, B):
    """tokens and final logits of fp16 and fp8 decode weights: greedy; sampled with seed 7, eager; the same under graph replay"""
    V = LW.shape.vocab
    dev = g["vision_emb"].device
    res = {}
    for dw in ("fp16", "fp8"):
        r = []
        for kw in (dict(do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0), dict(do_sample=True, seed=7, use_graph=False),
                   dict(do_sample=True, seed=7, use_graph=True)):
            out = m.mllm.generate_batch(g["vision_emb"], None, max_new_tokens=N, input_ids=g["input_ids"], attention_mask=g["attention_mask"],
                                        decode_weights=dw, **kw).clone()
            r.append((out, m.mllm._ws.get("gen.logits", (B, V), torch.float32, dev).clone()))
        res[dw] = r
    torch.cuda.synchronize()
    m.mllm.check_flags()
    return res


def _same(res):
    """fp8 == fp16: tokens and final logits.  (The sampled runs' logits hold the -inf the processors wrote in place -- banned
    n-grams -- in both paths alike; NaN would fail the equality.)"""
    for i, ((tok_a, log_a), (tok_b, log_b)) in enumerate(zip(res["fp16"], res["fp8"])):
        assert torch.equal(tok_a, tok_b), i
        assert torch.equal(log_a, log_b) and not torch.isnan(log_a).any(), i
    assert torch.isfinite(res["fp16"][0][1]).all()  # greedy, no processors: untouched logits


def _tile(t, B):
    return {k: v.repeat((B + v.shape[0] - 1) // v.shape[0], *([1] * (v.dim() - 1)))[:B].contiguous() for k, v in t.items()}


@pytest.mark.parametrize("storage", ["fp16", "bf16"])
def test_generation_fp8_equals_fp16_on_snapped_weights(gpu, storage):
    """Tiny generation fixture with the prepared matrices rounded to the format: decode_weights="fp8" and "fp16" give the
    same tokens and the same final logits, bit for bit -- greedy, sampled (eager and graph replay), at the fixture's batch
    (one block of 8 tokens) and tiled to 17 (two token blocks).  fp16 storage: 16-bit stream, fragment-major activations,
    the partial-sum LoRA form; bf16: the fp32 residual stream."""
    from tcavt_amd import model

    fx, cfg, w, t = load_generation_case()
    dev = gpu["device"]
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(w, device=dev).eval()
    if storage == "bf16":
        m.set_storage(torch.bfloat16)
    LW = m.mllm.llama_wrapper
    assert LW.stream16 == (storage == "fp16") and LW.use_lora
    _snap_prepared(LW)
    for B in (t["input_ids"].shape[0], 17):
        g = {k: v.to(dev) for k, v in _tile(t, B).items()}
        res = _both(m, LW, g, 9, B)
        _same(res)
        assert torch.equal(res["fp8"][1][0], res["fp8"][2][0])  # eager == graph replay
    assert LW._prep_dec is not None and LW._prep_dec8 is not None and LW._prep_dec8.table.dtype == torch.uint8
    # the copies go when the prepared weights go
    LW._invalidate()
    assert LW._prep_dec is None and LW._prep_dec8 is None


@pytest.mark.timeout(600)
def test_generation_fp8_equals_fp16_full_size(gpu):
    """Llama-3.2-1B shape, synthetic weights, snapped, B = 32, 3 new tokens: K = 8192, the N = 16384 gate|up, the
    two-column-block lm_head at V = 128256, the token blocks on two workgroups -- same equalities."""
    from tcavt_amd import config, model, synth
    from tcavt_amd.weights import make_weights

    dev = gpu["device"]
    cfg = config.PRESETS["llama32_1b"](seq_len=6, out_len=12, use_lora=True)
    with torch.device(dev):
        m = model.MultiModalTrajectoryModel.from_config(cfg)
    m.load_weights(make_weights(cfg, seed=1, backend="torch", device=dev)).eval()
    LW = m.mllm.llama_wrapper
    _snap_prepared(LW)
    B = 32
    b = synth.make_batch(cfg, B, text_len=24, seed=5, ragged=True, min_text=12)
    g = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
    res = _both(m, LW, g, 3, B)
    _same(res)
    assert LW._prep_dec8.table.numel() == cfg.llama.vocab * cfg.llama.hidden + 4 * cfg.llama.vocab
    del m, res
    torch.cuda.empty_cache()


# rel_err of the last step's logits, fp8 against fp16 decode weights, tiny fixture, 7 greedy steps, weights as they are:
# measured on an MI355X, deterministic.  The bar is 1.5 x this.  The figure is large because it is not one of rounding alone: on
# this 2-layer random-weight fixture (arg-max margins of 0.1) the greedy continuations part ways within the 7 steps, after which
# the two runs score different sequences.
QUALITY_MEASURED = 6.8224e-01


def test_generation_fp8_quality_on_unsnapped_weights(gpu):
    """The one figure that is not an equality: what rounding the weights to e4m3 (3 mantissa bits, power-of-two row scales)
    does to the logits after 7 greedy steps on the tiny fixture.  > 0 proves the FP8 copies were really used."""
    from tcavt_amd import model

    fx, cfg, w, t = load_generation_case()
    dev = gpu["device"]
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(w, device=dev).eval()
    g = {k: v.to(dev) for k, v in t.items()}
    B, V = t["input_ids"].shape[0], cfg.llama.vocab
    logits = {}
    for dw in ("fp16", "fp8"):
        m.mllm.generate_batch(g["vision_emb"], None, max_new_tokens=7, input_ids=g["input_ids"], attention_mask=g["attention_mask"],
                              do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0, decode_weights=dw)
        logits[dw] = m.mllm._ws.get("gen.logits", (B, V), torch.float32, dev).clone().cpu()
    m.mllm.check_flags()
    e = rel_err(logits["fp8"], logits["fp16"])
    print(f"[fp8 decode weights] tiny fixture, 7 greedy steps: rel_err of the last logits vs fp16 weights = {e:.4e}")
    assert 0 < e <= 1.5 * QUALITY_MEASURED, e


def test_generation_fp8_refusals(gpu):
    """No silent fallback: B = 33, TCAVT_DECODE_ROWMAJOR=1 and an unknown string raise."""
    from tcavt_amd import model

    fx, cfg, w, t = load_generation_case()
    dev = gpu["device"]
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(w, device=dev).eval()
    g = {k: v.to(dev) for k, v in t.items()}
    kw = dict(max_new_tokens=3, do_sample=False)
    g33 = {k: v.to(dev) for k, v in _tile(t, 33).items()}
    with pytest.raises(ValueError, match="B <= 32"):
        m.mllm.generate_batch(g33["vision_emb"], None, input_ids=g33["input_ids"], attention_mask=g33["attention_mask"], decode_weights="fp8", **kw)
    os.environ["TCAVT_DECODE_ROWMAJOR"] = "1"
    try:
        with pytest.raises(ValueError, match="TCAVT_DECODE_ROWMAJOR"):
            m.mllm.generate_batch(g["vision_emb"], None, input_ids=g["input_ids"], attention_mask=g["attention_mask"], decode_weights="fp8", **kw)
    finally:
        os.environ.pop("TCAVT_DECODE_ROWMAJOR", None)
    with pytest.raises(ValueError, match="fp16.*fp8"):
        m.mllm.generate_batch(g["vision_emb"], None, input_ids=g["input_ids"], attention_mask=g["attention_mask"], decode_weights="int8", **kw)
    with pytest.raises(ValueError, match="fp16.*fp8"):
        m.mllm.llama_wrapper.decode_weights("fp4")
    # B = 33 on fp16 weights keeps working as before (row-major weights)
    out = m.mllm.generate_batch(g33["vision_emb"], None, input_ids=g33["input_ids"], attention_mask=g33["attention_mask"], **kw)
    assert tuple(out.shape) == (33, 3)
