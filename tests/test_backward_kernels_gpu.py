"""Backward kernels of the default train step (csrc/backward.hip, csrc/small.hip) against plain float64 references, at
the shapes where their code paths switch: multi-block column sums, multi-partial LayerNorm reduces, 2- to 8-way split-K,
both small-attention backward kernels, and the elementwise / small-reduction glue.

The reductions are called through the C entry points with a caller-owned workspace filled with NaN: a finite, correct
result shows that every partial the reduce reads was written first.  A second call over different garbage must give the
same bits, and a workspace one element short of the documented size must be refused before any launch, with the output
left as it was.

Bars: relative Frobenius error <= 1e-6 against float64 for fp32 sums and GEMMs (the inputs are exact in double, so this
is the fp32 rounding of the kernel alone); exact where the kernel only selects, adds two numbers or converts."""
import ctypes
import math

import pytest
import torch

from tests.util import load_case, rel_err

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ERR_ARG = 1  # TCAVT_ERR_ARG (include/tcavt.h)
NAN = float("nan")


def _rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _lib():
    from tcavt_amd import capi

    return capi.lib()


def _stream():
    from tcavt_amd import capi

    return capi.stream_ptr()


def _ok(rc, what):
    from tcavt_amd import capi

    capi.check(rc, what)
    torch.cuda.synchronize()


def _garbage(ws, seed):
    """Refill a workspace with finite junk of a large magnitude (a partial read before it is written shows up)."""
    ws.copy_((torch.randn(ws.numel(), generator=_gen(seed)) * 1e6).to(ws.device))


# ---------------------------------------------------------------------------------------------------------------------
# colsum: out[n] (+)= sum_m g[m][n]; 128 rows per block, partials reduced by 16 waves in order
# ---------------------------------------------------------------------------------------------------------------------
COLSUM_CASES = [(1, 1), (1, 65), (127, 63), (128, 64), (129, 65), (129, 2048), (2048, 1), (2048, 768), (2048, 2048),
                (16 * 128 * 3 + 5, 63), (16 * 128 * 3 + 5, 768), (2368, 192)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N", COLSUM_CASES)
def test_colsum_against_float64(gpu, M, N, dtype):
    from tcavt_amd import capi

    dev, lib = gpu["device"], _lib()
    gen = _gen(M * 4099 + N)
    dt = capi.F32 if dtype == torch.float32 else capi.BF16
    nb = -(-M // 128)
    worst = 0.0
    for ld in (N, N + 13):  # packed, and a strided ld > N
        # columns with a nonzero mean keep the sums well conditioned (a zero-mean column of 2048 values can sum to ~1,
        # and the fp32 rounding of its partial sums then reads as a few 1e-6 relative)
        g = (torch.randn(M, ld, generator=gen) + 0.5).to(dtype)
        ref = g[:, :N].double().sum(0)  # bf16 and fp32 values are exact in double
        gd = g.to(dev)
        ws = torch.full((nb * N,), NAN, device=dev)
        out = torch.full((N,), NAN, device=dev)
        _ok(lib.tcavt_colsum(_p(gd), ld, dt, _p(out), M, N, 0, _p(ws), ws.numel(), _stream()), "colsum")
        assert torch.isfinite(out).all(), "colsum read a workspace partial it never wrote"
        e = _rel(out, ref)
        worst = max(worst, e)
        assert e <= 1e-6, (ld, e)
        # same bits over a different garbage workspace
        _garbage(ws, M + N)
        out2 = torch.full((N,), NAN, device=dev)
        _ok(lib.tcavt_colsum(_p(gd), ld, dt, _p(out2), M, N, 0, _p(ws), ws.numel(), _stream()), "colsum")
        assert torch.equal(out, out2)
        # accumulate onto a nonzero out
        init = torch.randn(N, generator=gen)
        acc = init.to(dev)
        ws.fill_(NAN)
        _ok(lib.tcavt_colsum(_p(gd), ld, dt, _p(acc), M, N, 1, _p(ws), ws.numel(), _stream()), "colsum accumulate")
        e = _rel(acc, init.double() + ref)
        worst = max(worst, e)
        assert e <= 1e-6, ("accumulate", ld, e)
        # a workspace one element short of ceil(M / 128) * N is refused before any launch; out is left unchanged
        before = acc.clone()
        rc = lib.tcavt_colsum(_p(gd), ld, dt, _p(acc), M, N, 1, _p(ws), nb * N - 1, _stream())
        torch.cuda.synchronize()
        assert rc == ERR_ARG and torch.equal(acc, before)
    print(f"[colsum {M}x{N} {dtype}] rel err max {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------
# layernorm_bwd: 16 rows per block (4 per wave), [4 waves][2][D] LDS slices, two fixed-order reduces
# ---------------------------------------------------------------------------------------------------------------------
def _ln_ref(x, gamma, gy, eps=1e-5):
    xd = x.double().requires_grad_(True)
    gd = gamma.double().requires_grad_(True)
    bd = torch.zeros_like(gd, requires_grad=True)
    y = torch.nn.functional.layer_norm(xd, (x.shape[1],), gd, bd, eps)
    y.backward(gy.double())
    return xd.grad, gd.grad, bd.grad


LN_CASES = [(1, 64), (15, 100), (16, 768), (17, 2048), (17, 64), (2048, 64), (2048, 100), (2048, 768), (2048, 2048),
            (4100, 64), (4100, 768), (4100, 2048)]


@pytest.mark.parametrize("M,D", LN_CASES)
def test_layernorm_bwd_against_float64_autograd(gpu, M, D):
    dev, lib = gpu["device"], _lib()
    gen = _gen(M * 31 + D)
    x = torch.randn(M, D, generator=gen) * 1.5 + 0.3
    gamma = torch.randn(D, generator=gen)
    gy = torch.randn(M, D, generator=gen)
    rgx, rgg, rgb = _ln_ref(x, gamma, gy)
    gg0, gb0 = torch.randn(D, generator=gen), torch.randn(D, generator=gen)  # ggamma, gbeta accumulate onto these
    nb = -(-M // 16)
    xd, gmd, gyd = x.to(dev), gamma.to(dev), gy.to(dev)
    ws = torch.full((nb * 2 * D,), NAN, device=dev)

    def run(ws):
        gx = torch.full((M, D), NAN, device=dev)
        gg, gb = gg0.to(dev), gb0.to(dev)
        _ok(lib.tcavt_layernorm_bwd(_p(xd), _p(gmd), _p(gyd), 1e-5, _p(gx), _p(gg), _p(gb), M, D, _p(ws), ws.numel(),
                                    _stream()), "layernorm_bwd")
        return gx, gg, gb

    gx, gg, gb = run(ws)
    for t in (gx, gg, gb):
        assert torch.isfinite(t).all(), "layernorm_bwd read a workspace partial it never wrote"
    e = (_rel(gx, rgx), _rel(gg, gg0.double() + rgg), _rel(gb, gb0.double() + rgb))
    print(f"[layernorm_bwd M={M} D={D}] rel err gx {e[0]:.2e} ggamma {e[1]:.2e} gbeta {e[2]:.2e}")
    assert max(e) <= 1e-6, e
    _garbage(ws, M + D)
    gx2, gg2, gb2 = run(ws)
    assert torch.equal(gx, gx2) and torch.equal(gg, gg2) and torch.equal(gb, gb2)
    # one element short of ceil(M / 16) * 2 * D: refused, outputs untouched
    b = (gx.clone(), gg.clone(), gb.clone())
    rc = lib.tcavt_layernorm_bwd(_p(xd), _p(gmd), _p(gyd), 1e-5, _p(gx), _p(gg), _p(gb), M, D, _p(ws), nb * 2 * D - 1,
                                 _stream())
    torch.cuda.synchronize()
    assert rc == ERR_ARG and torch.equal(gx, b[0]) and torch.equal(gg, b[1]) and torch.equal(gb, b[2])


def test_layernorm_bwd_large_mean_offset(gpu):
    """x with mean 50 and std 0.1 (mean / std = 500): the variance is taken about the mean in a second pass; a one-pass
    E[x^2] - E[x]^2 would lose every digit of it in fp32.  What remains is the fp32 rounding of the mean itself (~1 ulp
    of 50 plus the sum's own rounding, a few 1e-6, shifts every xhat by a few 1e-5): ggamma = sum gy xhat carries that
    shift in full (bar 3e-4), gx at first order times |mean(gy gamma)| + |mean(gy gamma xhat)| ~ 2 / sqrt(D) (bar 2e-5);
    gbeta does not see x (1e-6).  Measured: gx 1.3e-6, ggamma 2.5e-5, gbeta 1.1e-7.  A one-pass E[x^2] - E[x]^2 misses
    the first two by orders of magnitude."""
    dev, lib = gpu["device"], _lib()
    M, D = 2048, 768
    gen = _gen(50)
    x = torch.randn(M, D, generator=gen) * 0.1 + 50.0
    gamma = torch.randn(D, generator=gen)
    gy = torch.randn(M, D, generator=gen)
    rgx, rgg, rgb = _ln_ref(x, gamma, gy)
    nb = -(-M // 16)
    ws = torch.full((nb * 2 * D,), NAN, device=dev)
    gx = torch.empty(M, D, device=dev)
    gg, gb = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    xd, gmd, gyd = x.to(dev), gamma.to(dev), gy.to(dev)
    _ok(lib.tcavt_layernorm_bwd(_p(xd), _p(gmd), _p(gyd), 1e-5, _p(gx), _p(gg), _p(gb), M, D, _p(ws), ws.numel(),
                                _stream()), "layernorm_bwd")
    e = (_rel(gx, rgx), _rel(gg, rgg), _rel(gb, rgb))
    print(f"[layernorm_bwd mean 50 std 0.1] rel err gx {e[0]:.2e} ggamma {e[1]:.2e} gbeta {e[2]:.2e}")
    assert e[0] <= 2e-5 and e[1] <= 3e-4 and e[2] <= 1e-6, e


def test_layernorm_bwd_refuses_d_beyond_lds(gpu):
    """D = 2048 fills the 64 KiB of LDS ([4 waves][2][D] floats); D = 2049 is refused before any launch."""
    dev, lib = gpu["device"], _lib()
    M, D = 16, 2049
    x = torch.randn(M, D, device=dev)
    gamma = torch.ones(D, device=dev)
    gx = torch.full((M, D), 7.0, device=dev)
    gg, gb = torch.full((D,), 7.0, device=dev), torch.full((D,), 7.0, device=dev)
    ws = torch.zeros(2 * D, device=dev)
    rc = lib.tcavt_layernorm_bwd(_p(x), _p(gamma), _p(x), 1e-5, _p(gx), _p(gg), _p(gb), M, D, _p(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    assert rc == ERR_ARG
    assert (gx == 7.0).all() and (gg == 7.0).all() and (gb == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# gemm_f32_strided: split-K over up to 8 workspace slices, reduce in slice order + ACCUM / BIAS / RESIDUAL epilogue
# ---------------------------------------------------------------------------------------------------------------------
def _gemm_operands(form, Mo, No, Kc, gen, dev):
    """The two operand forms backward.py issues.  Returns (A, rsA, csA, W, rsW, csW, float64 reference of C[Mo][No]).
    gW: C[n][k] = sum_m gy[m][n] x[m][k]   (A = gy^T: rsA = 1; W = x^T: rsW = 1; contraction over the rows m)
    gx: C[m][k] = sum_n gy[m][n] W[n][k]   (A = gy row-major; W^T: rsW = 1)"""
    if form == "gW":
        gy = torch.randn(Kc, Mo + 3, generator=gen)  # padded leading dimensions
        x = torch.randn(Kc, No + 5, generator=gen)
        ref = gy[:, :Mo].double().T @ x[:, :No].double()
        A, W = gy.to(dev), x.to(dev)
        return A, 1, A.stride(0), W, 1, W.stride(0), ref
    gy = torch.randn(Mo, Kc + 3, generator=gen)
    w = torch.randn(Kc, No + 5, generator=gen)
    ref = gy[:, :Kc].double() @ w[:, :No].double()
    A, W = gy.to(dev), w.to(dev)
    return A, A.stride(0), 1, W, 1, W.stride(0), ref


def _gemm(A, rsA, csA, W, rsW, csW, C, ldc, Mo, No, Kc, flags, ws=None, ws_elems=0, bias=None, res=None, ldr=0):
    _ok(_lib().tcavt_gemm_f32_strided(_p(A), rsA, csA, _p(W), rsW, csW, _p(bias), _p(res), ldr, _p(C), ldc, Mo, No, Kc, flags,
                                      _p(ws), ws_elems, _stream()), "gemm_f32_strided")


def _slices_written(ws, Mo, No):
    """Number of leading workspace slices the launch overwrote (the rest still hold NaN)."""
    sl = ws.view(-1, Mo * No)
    fin = torch.isfinite(sl).all(1).cpu().tolist()
    nan = torch.isnan(sl).all(1).cpu().tolist()
    n = sum(fin)
    assert fin == [True] * n + [False] * (len(fin) - n), "split-K slices written out of order / partially"
    assert all(nan[n:]), "a slice beyond the split count was touched"
    return n


# (Mo, No, Kc, splits with a full 8-slice workspace): tiles = ceil(Mo/64) ceil(No/64) < 128 and Kc >= 512 split,
# min(Kc // 256, 8) ways, halved while tiles * splits > 512; Kc need not be a multiple of 16 or 256
GEMM_SPLIT_CASES = [(64, 192, 600, 2), (100, 70, 1000, 3), (128, 128, 1100, 4), (128, 256, 2047, 7), (256, 768, 2048, 8),
                    (64, 2048, 2048, 8), (2048, 64, 2368, 8), (768, 512, 2048, 4), (192, 64, 2048, 8)]


@pytest.mark.parametrize("form", ["gW", "gx"])
@pytest.mark.parametrize("Mo,No,Kc,splits", GEMM_SPLIT_CASES)
def test_gemm_f32_strided_split_k(gpu, form, Mo, No, Kc, splits):
    from tcavt_amd.capi import EPI_ACCUM, EPI_BIAS, EPI_RESIDUAL

    dev = gpu["device"]
    gen = _gen(Mo * 7 + No * 3 + Kc + (form == "gx"))
    A, rsA, csA, W, rsW, csW, ref = _gemm_operands(form, Mo, No, Kc, gen, dev)
    args = (A, rsA, csA, W, rsW, csW)
    MN = Mo * No
    ws = torch.full((8 * MN,), NAN, device=dev)
    errs = {}

    def check(name, got, want, bar=1e-6):
        assert torch.isfinite(got).all(), name
        errs[name] = e = _rel(got, want)
        assert e <= bar, (name, e)

    # plain, full workspace: the expected number of slices is written, the result is finite and correct
    C = torch.full((Mo, No), NAN, device=dev)
    _gemm(*args, C, No, Mo, No, Kc, 0, ws, ws.numel())
    assert _slices_written(ws, Mo, No) == splits
    check("plain", C, ref)
    # the unsplit result at the same shape (a workspace too small for 1 slice: cap 0) agrees within the fp32 bar
    ws1 = torch.full((MN,), NAN, device=dev)
    C1 = torch.full((Mo, No), NAN, device=dev)
    _gemm(*args, C1, No, Mo, No, Kc, 0, ws1, MN - 1)
    assert torch.isnan(ws1).all()
    check("unsplit", C1, ref)
    check("split vs unsplit", C, C1.double())
    # same bits over a different garbage workspace
    _garbage(ws, Kc)
    C2 = torch.full((Mo, No), NAN, device=dev)
    _gemm(*args, C2, No, Mo, No, Kc, 0, ws, ws.numel())
    assert torch.equal(C, C2)
    # ACCUM onto a nonzero C, which is a column block of a wider buffer (ldc > No): the sentinel columns survive
    C0 = torch.randn(Mo, No, generator=gen)
    wide = torch.full((Mo, No + 7), 3.25, device=dev)
    wide[:, :No] = C0.to(dev)
    ws.fill_(NAN)
    _gemm(*args, wide, No + 7, Mo, No, Kc, EPI_ACCUM, ws, ws.numel())
    assert _slices_written(ws, Mo, No) == splits
    check("accum ldc>N", wide[:, :No], C0.double() + ref)
    assert (wide[:, No:] == 3.25).all(), "ldc > N: columns beyond N were written"
    # BIAS + RESIDUAL from a separate (padded) buffer
    bias = torch.randn(No, generator=gen)
    res = torch.randn(Mo, No + 2, generator=gen)
    Cb = torch.full((Mo, No), NAN, device=dev)
    ws.fill_(NAN)
    _gemm(*args, Cb, No, Mo, No, Kc, EPI_BIAS | EPI_RESIDUAL, ws, ws.numel(), bias=bias.to(dev), res=res.to(dev), ldr=No + 2)
    check("bias+residual", Cb, ref + bias.double() + res[:, :No].double())
    # RESIDUAL aliasing C (in-place residual add), with BIAS
    Cr = C0.to(dev)
    ws.fill_(NAN)
    _gemm(*args, Cr, No, Mo, No, Kc, EPI_BIAS | EPI_RESIDUAL, ws, ws.numel(), bias=bias.to(dev), res=Cr, ldr=No)
    assert _slices_written(ws, Mo, No) == splits
    check("residual aliases C", Cr, ref + bias.double() + C0.double())
    # a workspace of fewer slices than Kc // 256: the cap applies (3 slices' worth minus one element -> 2 slices, or 1)
    if splits >= 3:
        ws.fill_(NAN)
        Cc = C0.to(dev)
        _gemm(*args, Cc, No, Mo, No, Kc, EPI_ACCUM, ws, 3 * MN - 1)
        assert _slices_written(ws, Mo, No) == 2
        check("capped accum", Cc, C0.double() + ref)
    # no workspace: at most 2 splits through atomics into the zeroed C, none under ACCUM; reproducible either way
    Cn = torch.full((Mo, No), NAN, device=dev)
    _gemm(*args, Cn, No, Mo, No, Kc, EPI_BIAS, bias=bias.to(dev))
    check("ws=NULL", Cn, ref + bias.double())
    Cn2 = torch.full((Mo, No), NAN, device=dev)
    _gemm(*args, Cn2, No, Mo, No, Kc, EPI_BIAS, bias=bias.to(dev))
    assert torch.equal(Cn, Cn2)
    Ca = C0.to(dev)
    _gemm(*args, Ca, No, Mo, No, Kc, EPI_ACCUM)
    check("ws=NULL accum", Ca, C0.double() + ref)
    Ca2 = C0.to(dev)
    _gemm(*args, Ca2, No, Mo, No, Kc, EPI_ACCUM)
    assert torch.equal(Ca, Ca2)
    print(f"[gemm_f32_strided {form} {Mo}x{No} K={Kc} splits={splits}] " +
          " ".join(f"{k} {v:.1e}" for k, v in errs.items()))


def test_gemm_f32_strided_no_split_forms(gpu):
    """Shapes that never split (>= 128 output tiles, or K < 512) write no workspace; ACCUM / residual-aliasing-C / ldc > N
    in the single-pass epilogue."""
    from tcavt_amd.capi import EPI_ACCUM, EPI_BIAS, EPI_RESIDUAL

    dev = gpu["device"]
    for form, Mo, No, Kc in (("gx", 2048, 2048, 64), ("gW", 64, 2048, 511), ("gW", 1024, 1024, 2048)):
        gen = _gen(Mo + No + Kc)
        A, rsA, csA, W, rsW, csW, ref = _gemm_operands(form, Mo, No, Kc, gen, dev)
        ws = torch.full((8 * Mo * No,), NAN, device=dev)
        C0 = torch.randn(Mo, No, generator=gen)
        wide = torch.full((Mo, No + 3), -1.5, device=dev)
        wide[:, :No] = C0.to(dev)
        _gemm(A, rsA, csA, W, rsW, csW, wide, No + 3, Mo, No, Kc, EPI_ACCUM, ws, ws.numel())
        assert torch.isnan(ws).all()
        e = _rel(wide[:, :No], C0.double() + ref)
        assert e <= 1e-6 and (wide[:, No:] == -1.5).all(), (form, Mo, No, Kc, e)
        bias = torch.randn(No, generator=gen)
        Cr = C0.to(dev)
        _gemm(A, rsA, csA, W, rsW, csW, Cr, No, Mo, No, Kc, EPI_BIAS | EPI_RESIDUAL, ws, ws.numel(), bias=bias.to(dev), res=Cr,
              ldr=No)
        e2 = _rel(Cr, ref + bias.double() + C0.double())
        print(f"[gemm_f32_strided unsplit {form} {Mo}x{No} K={Kc}] accum {e:.1e} residual=C {e2:.1e}")
        assert e2 <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# mha_bwd: LDS-staged kernel when 2 Lq Lk 4 + 2 (Lq + Lk)(dh + 1) 4 <= 64 KiB, the unstaged one otherwise
# ---------------------------------------------------------------------------------------------------------------------
def _mha_bwd_ref(q, k, v, go, key_len, scale):
    """float64 autograd of softmax(q k^T scale, keys j >= key_len masked) v per (sample, head); q [B,nh,Lq,dh].
    key_len 0: the forward (tcavt_mha) writes zeros, so every gradient of that sample is zero."""
    B, nh, Lq, dh = q.shape
    Lk = k.shape[2]
    kl = key_len.clamp(min=1)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    s = qd @ kd.transpose(-1, -2) * scale
    mask = torch.arange(Lk)[None, :] >= kl[:, None]
    p = torch.softmax(s.masked_fill(mask[:, None, None, :], float("-inf")), -1)
    o = p @ vd
    keep = (key_len > 0).double()[:, None, None, None]
    (o * keep).backward(go.double())
    return qd.grad, kd.grad, vd.grad


def _mha_case(gpu, B, Lq, Lk, nh, dh, key_len, pad, seed):
    from tcavt_amd import ops

    dev = gpu["device"]
    gen = _gen(seed)
    E = nh * dh
    scale = 1.0 / math.sqrt(dh)
    q = torch.randn(B, nh, Lq, dh, generator=gen)
    k = torch.randn(B, nh, Lk, dh, generator=gen)
    v = torch.randn(B, nh, Lk, dh, generator=gen)
    go = torch.randn(B, nh, Lq, dh, generator=gen)
    kl = torch.tensor(key_len, dtype=torch.int32)
    rq, rk, rv = _mha_bwd_ref(q, k, v, go, kl.long(), scale)
    tok = lambda t: t.permute(0, 2, 1, 3).reshape(B * t.shape[2], E)  # [B, L, nh*dh] rows
    # q | k | v packed in one row of width 3E + pad (as the encoder's qkv), dO with its own padded ld, the gradients into
    # one [rows, 3E + pad] buffer whose pad columns hold a sentinel
    ldqkv, ldo, ldg = 3 * E + pad, E + pad, 3 * E + pad
    rows = B * max(Lq, Lk)
    qkv = torch.zeros(rows, ldqkv)
    qkv[:B * Lq, :E], qkv[:B * Lk, E:2 * E], qkv[:B * Lk, 2 * E:3 * E] = tok(q), tok(k), tok(v)
    god = torch.zeros(B * Lq, ldo)
    god[:, :E] = tok(go)
    qkv, god = qkv.to(dev), god.to(dev)
    g = torch.full((rows, ldg), 5.5, device=dev)
    ops.mha_bwd(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], god, g[:, :E], g[:, E:2 * E], g[:, 2 * E:], B, Lq, Lk, nh, dh,
                scale, key_len=kl.to(dev), ldq=ldqkv, ldk=ldqkv, ldv=ldqkv, ldo=ldo, ldg=ldg)
    torch.cuda.synchronize()
    gc = g.cpu()
    if pad:
        assert (gc[:, 3 * E:] == 5.5).all(), "mha_bwd wrote into the pad columns"
    e = (_rel(gc[:B * Lq, :E], tok(rq)), _rel(gc[:B * Lk, E:2 * E], tok(rk)), _rel(gc[:B * Lk, 2 * E:3 * E], tok(rv)))
    for b, n in enumerate(key_len):
        if n == 0:  # zero gradients exactly, as the forward's zero output
            assert (gc[b * Lq:(b + 1) * Lq, :E] == 0).all() and (gc[b * Lk:(b + 1) * Lk, E:3 * E] == 0).all()
        elif n < Lk:  # masked keys get exactly zero key / value gradients
            assert (gc[b * Lk + n:(b + 1) * Lk, E:3 * E] == 0).all()
    return e


# (B, Lq, Lk, nh, dh, pad, staged): lane-polygon encoder (staged), Q-Former self-attention (staged), one whose staging does
# not fit (2*90*90*4 = 64800 bytes of P / dS alone)
MHA_CASES = [(32, 64, 64, 4, 16, 5, True), (16, 32, 32, 8, 96, 3, True), (3, 90, 90, 2, 24, 1, False),
             (4, 64, 64, 2, 64, 0, False)]


@pytest.mark.parametrize("B,Lq,Lk,nh,dh,pad,staged", MHA_CASES)
def test_mha_bwd_against_float64_autograd(gpu, B, Lq, Lk, nh, dh, pad, staged):
    """gq, gk, gv against float64 autograd; ragged key_len with 1, Lk and 0 (zero output in the forward, so zero
    gradients); padded leading dimensions whose pad columns must survive."""
    lds = 2 * Lq * Lk * 4
    assert (lds + 2 * (Lq + Lk) * (dh + 1) * 4 <= 65536) == staged  # which kernel the launcher picks
    g = _gen(B * Lq + dh)
    key_len = [Lk, 1, 0, Lk - 1] + torch.randint(1, Lk + 1, (B - 4,), generator=g).tolist() if B >= 4 else [Lk, 1, 0][:B]
    e = _mha_case(gpu, B, Lq, Lk, nh, dh, key_len[:B], pad, B * 1000 + Lq * 10 + dh)
    print(f"[mha_bwd B={B} L={Lq}x{Lk} nh={nh} dh={dh} {'LDS-staged' if staged else 'unstaged'}] rel err "
          f"gq {e[0]:.2e} gk {e[1]:.2e} gv {e[2]:.2e}")
    assert max(e) <= 1e-6, e


def test_mha_bwd_refuses_scores_beyond_64k(gpu):
    dev, lib = gpu["device"], _lib()
    Lq = Lk = 91  # 2 * 91 * 91 * 4 = 66248 bytes
    t = torch.zeros(Lq, 16, device=dev)
    out = torch.full((Lq, 16), 2.0, device=dev)
    rc = lib.tcavt_mha_bwd(_p(t), 16, _p(t), 16, _p(t), 16, _p(t), 16, _p(out), _p(out), _p(out), 16, None, 1, Lq, Lk, 1, 16,
                           0.25, 0.0, 0, 0, _stream())
    torch.cuda.synchronize()
    assert rc == ERR_ARG and (out == 2.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# elementwise and small reductions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ydt", [torch.float32, torch.bfloat16])
def test_relu_bwd_exact(gpu, ydt):
    from tcavt_amd import ops

    dev = gpu["device"]
    gen = _gen(3)
    n = 4099
    g = torch.randn(n, generator=gen)
    y = torch.randn(n, generator=gen)
    y[::7] = 0.0
    y[1::7] = -0.0
    y[2::11] = 1e-30  # a tiny positive
    y = y.to(ydt)
    gd = g.to(dev)
    ops.relu_bwd(gd, y.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(gd.cpu(), torch.where(y.float() > 0, g, torch.zeros_like(g)))


def test_add_inplace_exact_odd_n(gpu):
    from tcavt_amd import ops

    dev = gpu["device"]
    gen = _gen(4)
    for n in (1, 255, 257, 100003):
        a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        ad = a.to(dev)
        ops.add_inplace(ad, b.to(dev))
        torch.cuda.synchronize()
        assert torch.equal(ad.cpu(), a + b), n


def test_mse_grad(gpu):
    """g = 2 (pred - gt) r^2 / (B To) per coordinate.  The kernel takes the difference in pixels, (pred r + mn) -
    (gt r + mn), as the reference training loop does; with mn ~ 3000 that difference carries the rounding of two
    pixel-space values, so each element is held to 4 ulp of those magnitudes rather than to a relative bar."""
    from tcavt_amd import ops

    dev = gpu["device"]
    gen = _gen(5)
    B, To = 37, 30
    pred = torch.rand(B, 2, To, generator=gen)
    gt = torch.rand(B, 2, To, generator=gen)
    mn = torch.rand(B, 2, generator=gen) * 3000 + 500
    ns = torch.stack([mn[:, 0], mn[:, 0] + 50 + torch.rand(B, generator=gen) * 400,
                      mn[:, 1], mn[:, 1] + 1 + torch.rand(B, generator=gen) * 100], 1)
    g = torch.full((B, 2, To), NAN, device=dev)
    ops.mse_grad(pred.to(dev), gt.to(dev), ns.to(dev), g, B, To)
    torch.cuda.synchronize()
    r = torch.stack([ns[:, 1] - ns[:, 0], ns[:, 3] - ns[:, 2]], 1).double()[:, :, None]
    m = torch.stack([ns[:, 0], ns[:, 2]], 1).double()[:, :, None]
    ref = 2 * (pred.double() - gt.double()) * r * r / (B * To)
    eps = 2.0 ** -23
    tol = 4 * eps * (m.abs() + r * (pred.double().abs() + gt.double().abs())) * 2 * r / (B * To) + 4 * eps * ref.abs()
    err = (g.cpu().double() - ref).abs()
    print(f"[mse_grad] max err / tol {(err / tol).max().item():.2f}")
    assert (err <= tol).all()


def test_masked_mean_bwd_exact(gpu):
    from tcavt_amd import ops

    dev = gpu["device"]
    B, P, D = 6, 64, 64
    lens = torch.tensor([0, 1, 17, 63, 64, 100], dtype=torch.int32)  # 0, interior, P - 1, P, beyond P (clamped to P)
    gemb = torch.randn(B, D, generator=_gen(6))
    genc = torch.full((B, P, D), NAN, device=dev)
    ops.masked_mean_bwd(gemb.to(dev), lens.to(dev), genc, B, P, D)
    torch.cuda.synchronize()
    ref = torch.zeros(B, P, D)
    for b in range(B):
        n = min(int(lens[b]), P)
        if n:
            ref[b, :n] = gemb[b] / float(n)  # one correctly rounded fp32 division, as the kernel
    assert torch.equal(genc.cpu(), ref)


def test_poly_embed_bwd(gpu):
    """B * P = 2368 > 256 rows per block-stride loop; pixel coordinates up to 3839 as the data has them."""
    from tcavt_amd import ops

    dev = gpu["device"]
    gen = _gen(7)
    B, P, D = 37, 64, 64
    g = torch.randn(B, P, D, generator=gen)
    poly = torch.rand(B, P, 2, generator=gen) * 3839
    gw = torch.full((D, 2), NAN, device=dev)
    gb = torch.full((D,), NAN, device=dev)
    gpos = torch.full((P + 3, D), 9.0, device=dev)  # rows beyond P untouched
    ops.poly_embed_bwd(g.to(dev), poly.to(dev), gw, gb, gpos, B, P, D)
    torch.cuda.synchronize()
    gd, pd = g.double(), poly.double()
    e = (_rel(gw, torch.einsum("bpd,bpk->dk", gd, pd)), _rel(gb, gd.sum((0, 1))), _rel(gpos[:P], gd.sum(0)))
    print(f"[poly_embed_bwd] rel err gw {e[0]:.2e} gb {e[1]:.2e} gpos {e[2]:.2e}")
    assert max(e) <= 1e-6 and (gpos[P:] == 9.0).all()


def test_conv1x1_bwd(gpu):
    from tcavt_amd import ops

    dev, lib = gpu["device"], _lib()
    gen = _gen(8)
    B, C, T = 37, 64, 18
    gxp = torch.randn(B, T, C, generator=gen)  # token-major
    for F in (1, 2, 3, 4):
        x = torch.randn(B, F, T, generator=gen)
        gw = torch.full((C, F), NAN, device=dev)
        gb = torch.full((C,), NAN, device=dev)
        ops.conv1x1_bwd(gxp.to(dev), x.to(dev), gw, gb, B, C, T, F)
        torch.cuda.synchronize()
        e = (_rel(gw, torch.einsum("btc,bft->cf", gxp.double(), x.double())), _rel(gb, gxp.double().sum((0, 1))))
        assert max(e) <= 1e-6, (F, e)
    x = torch.zeros(B, 5, T, device=dev)
    gw = torch.full((C, 5), 2.0, device=dev)
    gb = torch.full((C,), 2.0, device=dev)
    gxpd = gxp.to(dev)
    rc = lib.tcavt_conv1x1_bwd(_p(gxpd), _p(x), _p(gw), _p(gb), B, C, T, 5, _stream())
    torch.cuda.synchronize()
    assert rc == ERR_ARG and (gw == 2.0).all() and (gb == 2.0).all()


def _nlinear_ref(in_tok, W, bias, g_bcs):
    """out[b][c][s] = sum_t W[c][s][t] (in[b][t][c] - in[b][T-1][c]) + bias[c][s] + in[b][T-1][c]; float64 autograd."""
    x = in_tok.double().requires_grad_(True)
    Wd = W.double().requires_grad_(True)
    bd = bias.double().requires_grad_(True)
    u = x - x[:, -1:, :]
    out = torch.einsum("cst,btc->bcs", Wd, u) + bd[None] + x[:, -1, :][:, :, None]
    out.backward(g_bcs.double())
    return Wd.grad, bd.grad, x.grad


@pytest.mark.parametrize("B,C,T,S,layout,with_gin", [
    (32, 64, 18, 30, "bcs", True),   # LTSF decoder: g [B][C][To]       (backward.py: strides (C*To, To, 1))
    (37, 64, 18, 18, "bsc", True),   # LTSF encoder: g token-major [B][T][C] (strides (T*C, 1, C))
    (37, 64, 18, 30, "bcs", False),  # gin = NULL: weight / bias gradients only
    (5, 8, 1, 7, "bsc", True),       # T = 1: u == 0, gin[T-1] = sum_s g
    (96, 4, 64, 64, "bcs", True),    # (B (T + S) + S T) * 4 = 65536 bytes of LDS exactly
])
def test_nlinear_bwd_against_float64_autograd(gpu, B, C, T, S, layout, with_gin):
    from tcavt_amd import ops

    dev = gpu["device"]
    gen = _gen(B * C + T * S)
    in_tok = torch.randn(B, T, C, generator=gen)
    W = torch.randn(C, S, T, generator=gen) / math.sqrt(T)
    bias = torch.randn(C, S, generator=gen)
    g_bcs = torch.randn(B, C, S, generator=gen)
    rW, rb, rin = _nlinear_ref(in_tok, W, bias, g_bcs)
    if layout == "bcs":
        gd, strides = g_bcs.contiguous().to(dev), (C * S, S, 1)
    else:
        gd, strides = g_bcs.permute(0, 2, 1).contiguous().to(dev), (S * C, 1, C)
    gW = torch.full((C, S, T), NAN, device=dev)
    gbias = torch.full((C, S), NAN, device=dev)
    gin = torch.full((B, T, C), NAN, device=dev) if with_gin else None
    ops.nlinear_bwd(in_tok.to(dev), W.to(dev), gd, strides, gW, gbias, gin, B, C, T, S)
    torch.cuda.synchronize()
    e = [_rel(gbias, rb)] + ([_rel(gin, rin)] if with_gin else [])
    if T > 1:
        e.append(_rel(gW, rW))
    else:
        assert (gW.cpu() == 0).all()  # u == 0 identically
    print(f"[nlinear_bwd B={B} C={C} T={T} S={S} {layout} gin={with_gin}] rel err " + " ".join(f"{x:.2e}" for x in e))
    assert max(e) <= 1e-6, e


def test_nlinear_bwd_refuses_lds_beyond_64k(gpu):
    dev, lib = gpu["device"], _lib()
    B, C, T, S = 97, 4, 64, 64  # (97 * 128 + 4096) * 4 = 66048 bytes
    t = torch.zeros(B * T * C + C * S * T, device=dev)
    gW = torch.full((C * S * T,), 3.0, device=dev)
    rc = lib.tcavt_nlinear_bwd(_p(t), _p(t), _p(t), S * C, 1, C, _p(gW), _p(gW), None, B, C, T, S, _stream())
    torch.cuda.synchronize()
    assert rc == ERR_ARG and (gW == 3.0).all()


def test_out_head_bwd(gpu):
    from tcavt_amd import ops

    dev = gpu["device"]
    gen = _gen(9)
    B, To, C, F = 32, 30, 64, 2
    g = torch.randn(B, F, To, generator=gen)
    fused = torch.randn(B, To, C, generator=gen)
    w = torch.randn(F, C, generator=gen)
    gf = torch.full((B, To, C), NAN, device=dev)
    gw = torch.full((F, C), NAN, device=dev)
    gb = torch.full((F,), NAN, device=dev)
    ops.out_head_bwd(g.to(dev), fused.to(dev), w.to(dev), gf, gw, gb, B, To, C, F)
    torch.cuda.synchronize()
    gd = g.double()
    e = (_rel(gf, torch.einsum("bfs,fc->bsc", gd, w.double())), _rel(gw, torch.einsum("bfs,bsc->fc", gd, fused.double())),
         _rel(gb, gd.sum((0, 2))))
    print(f"[out_head_bwd] rel err gf {e[0]:.2e} gw {e[1]:.2e} gb {e[2]:.2e}")
    assert max(e) <= 1e-6, e


def _bf16_ulp(x):
    """Spacing of bf16 at |x| (8 significant bits)."""
    x = x.abs().double().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(x)) - 7)


def test_softmax_bwd_rows_padded(gpu):
    """dS = scale P (dP - sum_c P dP) for c < n_valid, exact zeros up to n_out, nothing beyond (padded ldp / ldd / lds).
    bf16 output within 1 bf16 ulp of the float64 value (the fp32 intermediate may land on the other side of a tie), plus
    the fp32 rounding bound of the row's dot product where dP - dot cancels."""
    from tcavt_amd import ops

    dev = gpu["device"]
    gen = _gen(10)
    rows, n_valid, n_out, ldp, ldd, lds = 61, 100, 128, 136, 132, 140
    P = torch.softmax(torch.randn(rows, n_valid, generator=gen) * 2, -1).half()
    dP = torch.randn(rows, n_valid, generator=gen)
    Pb = torch.zeros(rows, ldp, dtype=torch.float16)
    Pb[:, :n_valid] = P
    dPb = torch.zeros(rows, ldd)
    dPb[:, :n_valid] = dP
    dS = torch.full((rows, lds), 7.0, dtype=torch.bfloat16, device=dev)
    scale = 0.125
    ops.softmax_bwd_rows(Pb.to(dev), dPb.to(dev), dS, scale, rows, n_valid, n_out, ldp, ldd, lds)
    torch.cuda.synchronize()
    got = dS.cpu()
    Pd = P.double()
    ref = scale * Pd * (dP.double() - (Pd * dP.double()).sum(1, keepdim=True))
    err = (got[:, :n_valid].double() - ref).abs()
    dot_err = n_valid * 2.0 ** -24 * (Pd * dP.double()).abs().sum(1, keepdim=True)
    tol = _bf16_ulp(ref) + scale * Pd * dot_err
    assert (err <= tol).all(), (err / tol).max().item()
    assert (got[:, n_valid:n_out] == 0).all() and not torch.signbit(got[:, n_valid:n_out].float()).any()
    assert (got[:, n_out:] == 7.0).all()


@pytest.mark.parametrize("f16_in", [True, False])
def test_transpose16_batched_exact(gpu, f16_in):
    """out[c][r] = in[r][c] per batch item, rows [rows, rows_pad) zero; fp16 -> bf16 conversion is round-to-nearest-even
    (bit-equal to torch's .bfloat16() of the fp16 value); bf16 -> bf16 is a copy."""
    from tcavt_amd import ops

    dev = gpu["device"]
    gen = _gen(11)
    batch, rows, cols, rows_pad, ld_in, ld_out = 3, 100, 70, 128, 72, 130
    s_in, s_out = rows * ld_in + 5, cols * ld_out + 3
    src = torch.randn(batch * s_in, generator=gen) * 4
    src[:64] = 1.0 + torch.arange(64) * 2.0 ** -10  # fp16 values between bf16 neighbours, ties included
    x = src.half() if f16_in else src.bfloat16()
    out = torch.full((batch * s_out,), 3.0, dtype=torch.bfloat16, device=dev)
    ops.transpose16(x.to(dev), out, rows, cols, rows_pad, ld_in=ld_in, ld_out=ld_out, batch=batch, s_in=s_in, s_out=s_out)
    torch.cuda.synchronize()
    got = out.cpu()
    for z in range(batch):
        blk = x[z * s_in:z * s_in + rows * ld_in].view(rows, ld_in)[:, :cols]
        want = blk.float().bfloat16().T if f16_in else blk.T
        o = got[z * s_out:z * s_out + cols * ld_out].view(cols, ld_out)
        assert torch.equal(o[:, :rows].view(torch.int16), want.contiguous().view(torch.int16)), z
        assert (o[:, rows:rows_pad].view(torch.int16) == 0).all(), z
        assert (o[:, rows_pad:] == 3.0).all(), z


def test_transpose_f32_bf16_exact(gpu):
    from tcavt_amd import ops

    dev = gpu["device"]
    gen = _gen(12)
    rows, cols, rows_pad, ld_in = 100, 70, 128, 75
    x = torch.randn(rows, ld_in, generator=gen) * 10
    ties = 1.0 + torch.arange(32, dtype=torch.float64) * 2.0 ** -8  # every other one halfway between bf16 neighbours
    x[0, :32] = ties.float()
    x[1, :32] = -ties.float()
    out = torch.full((cols, rows_pad + 6), 3.0, dtype=torch.bfloat16, device=dev)
    ops.transpose_f32_bf16(x.to(dev), out, rows, cols, rows_pad)
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[:, :rows].view(torch.int16), x[:, :cols].bfloat16().T.contiguous().view(torch.int16))
    assert (got[:, rows:rows_pad].view(torch.int16) == 0).all()
    assert (got[:, rows_pad:] == 3.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the trainable stages at the train step's batch (B = 32: M = 2048 polygon rows; B = 37: M = 2368, not a multiple of 128).
# The lane-polygon encoder and the LTSF head have the same dimensions in the tiny and the full preset; only B differs.
# ---------------------------------------------------------------------------------------------------------------------
RED_BUFS = ("bw.po.red", "bw.lt.red", "bw.xa.red")  # the reduction workspaces of the C backward stages


def _poison_reduction_workspaces(bw):
    n = 0
    for (name, _, _), t in bw.ws._bufs.items():
        if name in RED_BUFS:
            t.fill_(NAN)
            n += 1
    return n


def _train_batch(cfg, B, seed):
    """synth.make_batch with ragged polygon lengths that include 0, 1 and the maximum of 64 points."""
    import numpy as np
    from tcavt_amd import synth

    b = synth.make_batch(cfg, B, text_len=24, seed=seed)
    P = cfg.max_polygon_points
    rng = np.random.default_rng(seed)
    for i, n in ((0, 0), (1, P), (2, 1), (B - 1, P), (B // 2, 0)):
        b["lane_polygon_len"][i] = n
        b["lane_polygon"][i] = 0.0
        b["lane_polygon"][i, :n] = rng.uniform(0.0, 3839.0, (n, 2)).astype(np.float32)
    return {k: torch.from_numpy(v) for k, v in b.items()}


def _polygon_oracle(weights, cfg, polygon, lens, g_emb, relu_masks):
    """fp32 oracle autograd of the encoder, with the ReLU decisions of the HIP forward: a pre-activation
    within fp32 rounding of zero (|pre| < 1e-5, e.g. 5e-8 at one of the 4.8M units of B = 37) may fall on either side in
    two fp32 forwards, and one flipped unit moves its weight-gradient row by |g| |x|, 2.5e-4 of the whole tensor there.
    The backward is what is under test: every decision that differs from the oracle's own must be such a tie (checked on
    the valid rows).  -> (gradients, number of ties)"""
    from oracle import forward as O

    W = {k: torch.from_numpy(v).clone() for k, v in weights.items()}
    names = [k for k in W if k.startswith("lane_polygon_encoder.")]
    for k in names:
        W[k].requires_grad_(True)
    P = polygon.shape[1]
    valid = (torch.arange(P)[None, :] < lens.long().clamp(max=P)[:, None])[..., None]
    relu, calls, ties = torch.relu, [], []

    def relu_hip_mask(x):
        mask = relu_masks[len(calls)].view(x.shape)
        calls.append(1)
        flip = ((x > 0) != mask) & valid
        assert (x.detach()[flip].abs() < 1e-5).all(), "a ReLU decision differs from the oracle's beyond fp32 rounding"
        ties.append(int(flip.sum()))
        return x * torch.where(valid, mask, x.detach() > 0)

    torch.relu = relu_hip_mask
    try:
        emb = O.lane_polygon_encoder(W, cfg, polygon, lens)
    finally:
        torch.relu = relu
    assert len(calls) == cfg.lane_polygon_layers
    (emb * g_emb).sum().backward()
    return {k: W[k].grad for k in names}, sum(ties)


def _polygon_hip(gpu, cfg, weights, polygon, lens, g_emb, monkeypatch, py):
    """The HIP polygon-encoder backward twice from one forward, the reduction workspace poisoned with NaN in between;
    -> (gradients of the first run, of the second run, stage results, the forward's ReLU masks per layer)."""
    from tcavt_amd import backward, model, training

    dev = gpu["device"]
    if py:
        monkeypatch.setenv("TCAVT_PY_TLAYERS", "1")
    else:
        monkeypatch.delenv("TCAVT_PY_TLAYERS", raising=False)
    used = []
    orig = backward.Backward._polygon_stage
    monkeypatch.setattr(backward.Backward, "_polygon_stage", lambda self, *a, **k: used.append(orig(self, *a, **k)) or used[-1])
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights, device=dev).eval()
    tr = training.Trainer(m)
    names = [k for k in tr.book.g if k.startswith("lane_polygon_encoder.")]
    runs = []
    with torch.no_grad():
        m.lane_polygon_encoder(polygon.to(dev), lens.to(dev))
        masks = [(s["f"] > 0).cpu() for s in m.lane_polygon_encoder.saved.layers]
        for _ in range(2):
            tr.book.grads.zero_()
            tr.bw.polygon(g_emb.to(dev))
            torch.cuda.synchronize()
            runs.append({k: tr.book.g[k].cpu().clone() for k in names})
            _poison_reduction_workspaces(tr.bw)
    return runs[0], runs[1], used, masks


@pytest.mark.parametrize("py", [False, True], ids=["c_stage", "python_composition"])
@pytest.mark.parametrize("B", [32, 37])
def test_polygon_encoder_backward_at_train_batch(gpu, B, py, monkeypatch):
    """test_polygon_encoder_backward_is_exact_fp32 (same 2e-4 bar) at the train step's batch, where the weight gradients
    split K 8 ways, colsum has 16+ row blocks and every LayerNorm reduce wave adds 8+ partials; both the C stage
    (tcavt_tlayer_stack_backward) and the per-launch Python composition.  A repeat over a NaN-poisoned reduction workspace
    gives the same bits."""
    from tcavt_amd import config
    from tcavt_amd.weights import make_weights

    cfg = config.tiny()
    weights = make_weights(cfg, 3)
    t = _train_batch(cfg, B, seed=B)
    g_emb = torch.randn(B, cfg.lane_polygon_d_model, generator=_gen(B + 1))
    g1, g2, used, masks = _polygon_hip(gpu, cfg, weights, t["lane_polygon"], t["lane_polygon_len"], g_emb, monkeypatch, py)
    ref, ties = _polygon_oracle(weights, cfg, t["lane_polygon"], t["lane_polygon_len"], g_emb, masks)
    assert used == [not py, not py]
    errs = sorted(((rel_err(g1[k], ref[k]), k) for k in ref), reverse=True)
    print(f"[polygon bwd B={B} {'python' if py else 'C stage'}] max rel err {errs[0][0]:.2e} ({errs[0][1]}); "
          f"{ties} ReLU ties taken from the HIP forward")
    for k in ref:
        assert torch.isfinite(g1[k]).all(), k
        assert torch.equal(g1[k], g2[k]), ("not reproducible over a poisoned workspace", k)
    for e, k in errs:
        assert e < 2e-4, (k, e)


@pytest.mark.parametrize("B", [32, 37])
def test_ltsf_backward_at_train_batch(gpu, B):
    """test_ltsf_backward_from_fixed_hidden_states (same bars) at B = 32 / 37, L = 256 hidden-state rows, To = 30, with a
    small decoder of hidden size 2048, so that the absorbed cross-attention runs at its production width.  The backward
    runs twice from one forward with the reduction workspaces poisoned in between: the same bits."""
    import numpy as np
    from oracle import forward as O
    from tcavt_amd import config, model, ops, training
    from tcavt_amd.config import LlamaShape
    from tcavt_amd.weights import make_weights

    dev = gpu["device"]
    cfg = config.tiny(out_len=30)
    cfg.llama = LlamaShape(hidden=2048, inter=512, layers=1, n_q_heads=32, n_kv_heads=8, vocab=512)
    weights = make_weights(cfg, 4)
    t = _train_batch(cfg, B, seed=B + 100)
    gen = _gen(B + 10)
    L, H = 256, cfg.llama.hidden
    fh = torch.randn(B, L, H, generator=gen)
    poly = torch.randn(B, cfg.lane_polygon_d_model, generator=gen)
    W = {k: torch.from_numpy(v).clone() for k, v in weights.items()}
    names = [k for k in W if k.startswith("ltsf.")]
    for k in names:
        W[k].requires_grad_(True)
    poly_r = poly.clone().requires_grad_(True)
    out = O.ltsf_forward(W, cfg, t["traj_emb"], poly_r, fh, O._rounder("fp16")) + t["traj_emb"][:, :, -1:]
    dp, dg = O.denorm(out, t["norm_stat"]), O.denorm(t["target_traj"], t["norm_stat"])
    loss = torch.nn.functional.mse_loss(dp[:, 0], dg[:, 0]) + torch.nn.functional.mse_loss(dp[:, 1], dg[:, 1])
    loss.backward()

    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights, device=dev).eval()
    tr = training.Trainer(m)
    runs = []
    with torch.no_grad():
        x = t["traj_emb"].to(dev)
        fh_b = torch.zeros(B * L + 64, H, dtype=m.storage, device=dev)
        ops.cast16(fh.to(dev).view(B * L, H), out=fh_b)
        dec = m.ltsf(x, poly.to(dev), fh.to(dev), final_hidden_bf16=fh_b, _fuse_last_residual=True)
        g_out = torch.empty_like(dec)
        ops.mse_grad(dec, t["target_traj"].to(dev), t["norm_stat"].to(dev), g_out, B, cfg.out_len)
        for _ in range(2):
            tr.book.grads.zero_()
            g_poly = tr.bw.ltsf(g_out, x)
            torch.cuda.synchronize()
            runs.append(({k: tr.book.g[k].cpu().clone() for k in names}, g_poly.cpu().clone()))
            assert _poison_reduction_workspaces(tr.bw) >= 1
    (g1, gp1), (g2, gp2) = runs
    for k in names:
        assert torch.isfinite(g1[k]).all(), k
        assert torch.equal(g1[k], g2[k]), ("not reproducible over poisoned workspaces", k)
    assert torch.equal(gp1, gp2)
    errs = sorted(((rel_err(g1[k], W[k].grad), k) for k in names), reverse=True)
    e_poly = rel_err(gp1, poly_r.grad)
    med = float(np.median([e for e, _ in errs]))
    print(f"[ltsf grads B={B} H={H}] max {errs[0][0]:.2e} ({errs[0][1]}), median {med:.2e}, g_poly_emb {e_poly:.2e}")
    for e, k in errs:
        assert e < 3e-2, (k, e)
    assert med < 5e-3 and e_poly < 2e-2


@pytest.mark.parametrize("case", ["b1", "one_token", "no_polygons", "max_polygon"])
def test_edge_case_batches_backward(gpu, case, monkeypatch):
    """The backward counterpart of test_edge_case_batches_match_oracle on the same degenerate batches: the polygon-encoder
    stage within 2e-4 of oracle autograd from a fixed upstream gradient; a whole training step's gradient book finite,
    and exactly zero wherever the oracle's fp32 autograd gradient is exactly zero (every encoder weight when no sample
    has a polygon)."""
    from oracle import forward as O
    from tcavt_amd import model, synth, training
    from tcavt_amd.weights import trainable_keys

    dev = gpu["device"]
    cfg, weights, _ = load_case("tiny_6_12_lora_ragged")
    B, Lt = (1, 24) if case == "b1" else (3, 1) if case == "one_token" else (3, 24)
    b = synth.make_batch(cfg, B, text_len=Lt, seed=7, ragged=(case not in ("one_token",)), min_text=1)
    if case == "no_polygons":
        b["lane_polygon_len"][:] = 0
    if case == "max_polygon":
        b["lane_polygon_len"][:] = b["lane_polygon"].shape[1]
    t = {k: torch.from_numpy(v) for k, v in b.items()}
    # polygon-encoder stage from a fixed upstream gradient
    g_emb = torch.randn(B, cfg.lane_polygon_d_model, generator=_gen(11))
    g1, g2, _, masks = _polygon_hip(gpu, cfg, weights, t["lane_polygon"], t["lane_polygon_len"], g_emb, monkeypatch, False)
    ref, _ = _polygon_oracle(weights, cfg, t["lane_polygon"], t["lane_polygon_len"], g_emb, masks)
    for k in ref:
        assert torch.equal(g1[k], g2[k]), k
        if ref[k].abs().max() == 0:
            assert g1[k].abs().max().item() == 0, k
        else:
            assert rel_err(g1[k], ref[k]) < 2e-4, (k, rel_err(g1[k], ref[k]))
    # a whole step
    W = {k: torch.from_numpy(v).clone() for k, v in weights.items()}
    names = trainable_keys(W)
    for k in names:
        W[k].requires_grad_(True)
    loss, _ = O.model_forward(W, cfg, t["traj_emb"], t["vision_emb"], t["lane_polygon"], t["lane_polygon_len"],
                              t["input_ids"], t["attention_mask"], y=t["target_traj"], norm_stat=t["norm_stat"],
                              contract="fp32")
    loss.backward()
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(weights, device=dev).eval()
    tr = training.Trainer(m)
    g = {k: v.to(dev) for k, v in t.items()}
    loss_h, _ = tr.forward_backward(g["traj_emb"], g["vision_emb"], g["lane_polygon"], g["lane_polygon_len"],
                                    g["target_traj"], g["norm_stat"], g["input_ids"], g["attention_mask"], g["labels"])
    torch.cuda.synchronize()
    assert torch.isfinite(loss_h).all() and torch.isfinite(tr.book.grads).all()
    zeros = [k for k in names if W[k].grad is None or W[k].grad.abs().max() == 0]
    if case == "no_polygons":
        assert all(k in zeros for k in ref)
    for k in zeros:
        assert tr.book.g[k].abs().max().item() == 0, k
    print(f"[edge backward {case}] {len(zeros)} exactly-zero oracle gradients, all exactly zero on the HIP path")
